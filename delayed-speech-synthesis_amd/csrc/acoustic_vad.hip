// csrc/acoustic_vad.hip -- acoustic voice-activity labels for a list of trials (Part 7 of include/dss_hip.h).
//
// What the reference computes per trial with EnergyBasedVad.from_wav (local/common.py:582-649) and MelFilterBank
// (common.py:475-514), as prepare_corpus.get_vad_labels drives it (prepare_corpus.py:78-116): frames of N samples every
// `shift` samples, x / 2^15 times the window, the magnitude of the N-point real DFT, the mel filter bank, log(mel + 1e-7),
// coefficient 0 of the type-2 DCT over the bands (= 2 * their sum) as the frame's log energy; then per trial the threshold
// energy_threshold + energy_mean_scale * mean(log energy) and a vote over the frames [i - context, i + context).
//
// The reference's arithmetic is numpy's pocketfft and BLAS, not a fixed C sequence, so results are held to it to ~1e-12 on
// the log energy (tests/test_gpu_acoustic_vad.py), not bit for bit; the library is built with -ffp-contract=off, so every
// fused multiply-add here is written out (__builtin_fma, the fp64 MFMA).  Everything is float64.  Both kernels are pure
// functions of their trial: the same trial gives the same bits alone or in any list, run after run (every sum in a fixed
// order; the one atomic of this file is the integer max of the peak kernel, which has no order to depend on).
//
// Opt-in, the trial's audio is first prepared as prepare_corpus.py:63-69 prepares it (loudness through pydub's two gains; the
// arithmetic is avad_gain.h): a peak launch in front, the energy kernel's GAIN instantiation, and a kernel that writes the
// prepared int16 audio out when the caller wants it (what the reference hands its feature encoder).
#include "acoustic_vad.h"
#include "avad_gain.h"

#define AVAD_THREADS 256

typedef double avad_d4 __attribute__((ext_vector_type(4)));

// ---- log energy ------------------------------------------------------------------------------------------------------
// A workgroup takes AVAD_TILE_FRAMES consecutive frames of ONE trial.  Their samples ((TILE - 1) * shift + N of them; frames
// overlap N / shift-fold) are staged in LDS once, coalesced 2-byte loads widened to 32 bits on the way in.  The DFT is a
// matrix product on v_mfma_f64_16x16x4_f64: A = 16 windowed frames x 4 samples, B = 4 samples x 16 bins of cos (and of sin)
// gathered from ONE table of cos / sin(2 pi j / N) in LDS at index (bin * sample) mod N, kept by adding 4 * bin per step --
// no sincos in the loop and no N x N twiddle matrix anywhere.  A wave owns a block of 16 bins at a time and both 16-frame
// tiles, so one gathered (cos, sin) pair feeds four MFMAs.  Lane l holds A[frame l & 15][sample l >> 4] and
// B[sample l >> 4][bin l & 15]; of the f64 result, register r of lane l is [frame (l >> 4) + 4 r][bin l & 15].
// Magnitudes go to LDS, then every (frame, band) pair sums the nonzero run of its band's column in bin order, takes
// log(. + 1e-7), and one lane per frame adds the bands in order.
//
// GAIN = true is the same kernel on the PREPARED audio of a normalised call (avad_gain.h): a trial flagged `normalize` has every
// sample scaled twice, by the factor of its peak (peaks[], avad_peak_kernel) and by the post gain, on its way into LDS; all that
// follows sees the integers it would see had the prepared audio been handed over.  GAIN = false reads nothing of that.
template <bool GAIN>
__global__ void __launch_bounds__(AVAD_THREADS)
avad_energy_kernel(const short *__restrict__ audio, const DssAvadTrialDesc *__restrict__ desc, const DssAvadTile *__restrict__ tiles,
                   DssAvadDev p, double *__restrict__ log_energy, const int *__restrict__ peaks)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const int N = p.N, shift = p.shift, bins = p.bins, bands = p.bands;
    const int span = (AVAD_TILE_FRAMES - 1) * shift + N;
    double2 *tw = reinterpret_cast<double2 *>(lds);                  // [N] (cos, sin)
    double *win = lds + 2 * N;                                       // [N]
    double *mag = win + N;                                           // [TILE][bins]
    int *xs = reinterpret_cast<int *>(mag + AVAD_TILE_FRAMES * bins);   // [span] samples; later [TILE][bands] log mel as double
    double *logmel = reinterpret_cast<double *>(xs);

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const DssAvadTile tile = tiles[blockIdx.x];
    const DssAvadTrialDesc d = desc[tile.trial];
    const int frame0 = tile.frame0;

    for (int j = tid; j < N; j += AVAD_THREADS) {
        tw[j] = reinterpret_cast<const double2 *>(p.tw)[j];
        win[j] = p.win[j];
    }
    // sample s of the trial: zero in front of `lead`, audio[first + s - lead] behind it; nothing is read at or past n
    const long long s0 = (long long)frame0 * shift;
    if (GAIN && d.normalize) {
        const double gain = p.gain[peaks[d.index]], post = p.post_gain;
        for (int t = tid; t < span; t += AVAD_THREADS) {
            const long long s = s0 + t;
            xs[t] = (s >= d.lead && s < d.n) ? (int)avad_prepared(audio[d.first + (s - d.lead)], gain, post) : 0;
        }
    } else {
        for (int t = tid; t < span; t += AVAD_THREADS) {
            const long long s = s0 + t;
            xs[t] = (s >= d.lead && s < d.n) ? (int)audio[d.first + (s - d.lead)] : 0;
        }
    }
    __syncthreads();

    const int row = lane & 15, kq = lane >> 4;
    const int *x0 = xs + row * shift + kq;
    const int *x1 = x0 + 16 * shift;
    const double *wq = win + kq;
    const int nblk = (bins + 15) >> 4;
    for (int blk = wave; blk < nblk; blk += AVAD_THREADS / 64) {
        const int bin = blk * 16 + row;
        const bool live = bin < bins;
        const int b = live ? bin : 0;
        int idx = (int)(((long long)b * kq) % N);
        const int step = (int)((4LL * b) % N);
        avad_d4 re0 = {0.0, 0.0, 0.0, 0.0}, im0 = re0, re1 = re0, im1 = re0;
        for (int k = 0; k < N; k += 4) {
            const double2 t = tw[idx];
            const double w = wq[k];
            const double a0 = (double)x0[k] * w;
            const double a1 = (double)x1[k] * w;
            re0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, t.x, re0, 0, 0, 0);
            im0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, t.y, im0, 0, 0, 0);
            re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, t.x, re1, 0, 0, 0);
            im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, t.y, im1, 0, 0, 0);
            idx += step;
            if (idx >= N) idx -= N;
        }
        if (live) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = kq + 4 * r;
                mag[f * bins + bin] = __builtin_sqrt(__builtin_fma(re0[r], re0[r], im0[r] * im0[r]));
                mag[(f + 16) * bins + bin] = __builtin_sqrt(__builtin_fma(re1[r], re1[r], im1[r] * im1[r]));
            }
        }
    }
    __syncthreads();                                                  // magnitudes complete; the samples are no longer needed

    for (int q = tid; q < AVAD_TILE_FRAMES * bands; q += AVAD_THREADS) {
        const int f = q & (AVAD_TILE_FRAMES - 1), band = q / AVAD_TILE_FRAMES;
        const int lo = p.band_lo[band], o = p.band_off[band], cnt = p.band_off[band + 1] - o;
        const double *m = mag + f * bins + lo;
        double acc = 0.0;
        for (int j = 0; j < cnt; ++j) acc = __builtin_fma(m[j], p.mel_w[o + j], acc);
        logmel[f * bands + band] = log(acc + 0.0000001);
    }
    __syncthreads();
    if (tid < AVAD_TILE_FRAMES && frame0 + tid < d.W) {
        const double *lm = logmel + tid * bands;
        double s = 0.0;
        for (int band = 0; band < bands; ++band) s += lm[band];
        log_energy[d.out_frame + frame0 + tid] = 2.0 * s;
    }
}

// ---- threshold and vote --------------------------------------------------------------------------------------------------
// The sum of a trial's log energies in the order dss_avad_vote_host uses too: 256 strided running sums, then a halving
// tree over them.
__global__ void __launch_bounds__(AVAD_THREADS)
avad_vote_kernel(const DssAvadTrialDesc *__restrict__ desc, const double *__restrict__ log_energy, DssAvadDev p,
                 unsigned char *__restrict__ labels, double *__restrict__ threshold)
{
    __shared__ double part[AVAD_THREADS];
    const int tid = threadIdx.x;
    const DssAvadTrialDesc d = desc[blockIdx.x];
    const int W = d.W;
    const double *le = log_energy + d.out_frame;
    double s = 0.0;
    for (int i = tid; i < W; i += AVAD_THREADS) s += le[i];
    part[tid] = s;
    __syncthreads();
    for (int o = AVAD_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) part[tid] += part[tid + o];
        __syncthreads();
    }
    double thr = p.threshold;
    if (p.mean_scale != 0.0) thr += p.mean_scale * part[0] / (double)W;
    if (tid == 0 && threshold) threshold[d.index] = thr;
    for (int i = tid; i < W; i += AVAD_THREADS) {
        int num = 0, den = 0;
        for (int t2 = i - p.context; t2 < i + p.context; ++t2) {
            if (t2 >= 0 && t2 < W) {
                ++den;
                if (le[t2] > thr) ++num;
            }
        }
        const bool voiced = (double)num >= (double)den * p.proportion;
        labels[d.out_frame + i] = (voiced && !d.silence) ? 1 : 0;
    }
}

size_t dss_avad_energy_lds_bytes(int N, int shift, int bins, int bands)
{
    const size_t span = (size_t)(AVAD_TILE_FRAMES - 1) * shift + N;
    size_t tail = span * sizeof(int);
    const size_t lm = (size_t)AVAD_TILE_FRAMES * bands * sizeof(double);
    if (lm > tail) tail = lm;
    tail = (tail + 15) & ~(size_t)15;
    return ((size_t)3 * N + (size_t)AVAD_TILE_FRAMES * bins) * sizeof(double) + tail;
}

// ---- peak and prepared audio -----------------------------------------------------------------------------------------------
// max |x| over a trial's cut audio[first .. first + n): a workgroup takes AVAD_PEAK_TILE samples of one trial -- 16-byte loads
// where the address allows (`first` may be odd: the samples in front of the first aligned address and behind the last full
// vector are read one by one) --, reduces them in registers and LDS and joins the trial's other tiles through one integer
// atomicMax into peaks[trial], which the host zeroed on the same stream.  Integer max has no order: the same bits on every run.
__device__ static inline int avad_abs_pair(unsigned w)
{
    const int a = avad_abs16((short)(w & 0xffffu)), b = avad_abs16((short)(w >> 16));
    return a > b ? a : b;
}

__global__ void __launch_bounds__(AVAD_THREADS)
avad_peak_kernel(const short *__restrict__ audio, const DssAvadPeakTile *__restrict__ tiles, int *__restrict__ peaks)
{
    __shared__ int part[AVAD_THREADS / 64];
    const int tid = threadIdx.x;
    const DssAvadPeakTile tile = tiles[blockIdx.x];
    const short *x = audio + tile.first;
    const int cnt = tile.n;
    int head = (int)(((16u - (unsigned)((size_t)x & 15u)) & 15u) >> 1);
    if (head > cnt) head = cnt;
    const int nvec = (cnt - head) >> 3;
    int m = 0;
    if (tid < head) m = avad_abs16(x[tid]);
    const uint4 *xv = reinterpret_cast<const uint4 *>(x + head);
    for (int i = tid; i < nvec; i += AVAD_THREADS) {
        const uint4 v = xv[i];
        const int a = avad_abs_pair(v.x), b = avad_abs_pair(v.y), c = avad_abs_pair(v.z), e = avad_abs_pair(v.w);
        const int ab = a > b ? a : b, ce = c > e ? c : e;
        const int q = ab > ce ? ab : ce;
        m = m > q ? m : q;
    }
    for (int i = head + 8 * nvec + tid; i < cnt; i += AVAD_THREADS) {
        const int a = avad_abs16(x[i]);
        m = m > a ? m : a;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(m, o);
        m = m > other ? m : other;
    }
    if ((tid & 63) == 0) part[tid >> 6] = m;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < AVAD_THREADS / 64; ++w) m = m > part[w] ? m : part[w];
        atomicMax(peaks + tile.index, m);
    }
}

// The prepared trials themselves, int16, trial after trial in list order: `lead` zeros, then the first n - lead samples of the
// cut, scaled as the energy kernel scales them when the trial is flagged.  A workgroup writes AVAD_PEAK_TILE samples of one trial.
__global__ void __launch_bounds__(AVAD_THREADS)
avad_prepare_kernel(const short *__restrict__ audio, const DssAvadTrialDesc *__restrict__ desc, const DssAvadTile *__restrict__ tiles,
                    DssAvadDev p, const int *__restrict__ peaks, short *__restrict__ prepared)
{
    const int tid = threadIdx.x;
    const DssAvadTile tile = tiles[blockIdx.x];
    const DssAvadTrialDesc d = desc[tile.trial];
    const int s0 = tile.frame0;                                       // first sample of the tile, not a frame
    const int s1 = d.n - s0 < AVAD_PEAK_TILE ? d.n : s0 + AVAD_PEAK_TILE;
    short *out = prepared + d.out_sample;
    const short *in = audio + d.first - d.lead;
    if (d.normalize) {
        const double gain = p.gain[peaks[d.index]], post = p.post_gain;
        for (int s = s0 + tid; s < s1; s += AVAD_THREADS) out[s] = s >= d.lead ? avad_prepared(in[s], gain, post) : (short)0;
    } else {
        for (int s = s0 + tid; s < s1; s += AVAD_THREADS) out[s] = s >= d.lead ? in[s] : (short)0;
    }
}

int dss_launch_avad_peak(const short *d_audio, const DssAvadPeakTile *d_tiles, int n_tiles, int *d_peaks, hipStream_t s)
{
    if (n_tiles <= 0) return DSS_OK;
    hipLaunchKernelGGL(avad_peak_kernel, dim3((unsigned)n_tiles), dim3(AVAD_THREADS), 0, s, d_audio, d_tiles, d_peaks);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

int dss_launch_avad_prepare(const DssAvadDev &v, const short *d_audio, const DssAvadTrialDesc *d_desc, const DssAvadTile *d_tiles,
                            int n_tiles, const int *d_peaks, short *d_prepared, hipStream_t s)
{
    if (n_tiles <= 0) return DSS_OK;
    hipLaunchKernelGGL(avad_prepare_kernel, dim3((unsigned)n_tiles), dim3(AVAD_THREADS), 0, s, d_audio, d_desc, d_tiles, v, d_peaks,
                       d_prepared);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// d_peaks == NULL: the plain kernel on the audio as it is; else the prepared audio of the trials flagged `normalize`
int dss_launch_avad_energy(const DssAvadDev &v, const short *d_audio, const DssAvadTrialDesc *d_desc, const DssAvadTile *d_tiles,
                           int n_tiles, double *d_log_energy, const int *d_peaks, hipStream_t s)
{
    if (n_tiles <= 0) return DSS_OK;
    const size_t bytes = dss_avad_energy_lds_bytes(v.N, v.shift, v.bins, v.bands);
    if (bytes > AVAD_LDS_LIMIT || (v.N & 3) || v.bands > AVAD_MAX_BANDS) {
        dss_set_error("acoustic VAD: a window of %d samples with %d bands does not fit the energy kernel", v.N, v.bands);
        return DSS_EINVAL;
    }
    if (d_peaks) {
        DSS_HIP_CHECK(hipFuncSetAttribute((const void *)avad_energy_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(avad_energy_kernel<true>, dim3((unsigned)n_tiles), dim3(AVAD_THREADS), bytes, s, d_audio, d_desc, d_tiles, v,
                           d_log_energy, d_peaks);
    } else {
        DSS_HIP_CHECK(hipFuncSetAttribute((const void *)avad_energy_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        hipLaunchKernelGGL(avad_energy_kernel<false>, dim3((unsigned)n_tiles), dim3(AVAD_THREADS), bytes, s, d_audio, d_desc, d_tiles, v,
                           d_log_energy, d_peaks);
    }
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

int dss_launch_avad_vote(const DssAvadDev &v, const DssAvadTrialDesc *d_desc, int n_trials, const double *d_log_energy,
                         unsigned char *d_labels, double *d_threshold, hipStream_t s)
{
    if (n_trials <= 0) return DSS_OK;
    hipLaunchKernelGGL(avad_vote_kernel, dim3((unsigned)n_trials), dim3(AVAD_THREADS), 0, s, d_desc, d_log_energy, v, d_labels,
                       d_threshold);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
