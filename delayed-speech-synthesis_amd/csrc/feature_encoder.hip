// csrc/feature_encoder.hip -- the LPC feature encoder over a trial list (gfx950): Part 16 of include/dss_hip.h.
//
// The method is this project's statement of the published encoder (tests/feature_encoder_reference.py is the
// binding definition): per 160-sample frame 18 Bark cepstral coefficients, the pitch feature and correlation, 16 LPC taps.  One
// fresh encoder per trial.  Three launches on one stream:
//
//  (A) fenc_spectrum_kernel, one workgroup per FENC_TILE_FRAMES frames of one trial.  The pre-emphasised samples the tile's
//      windows cover are staged in LDS once (overlapping windows re-read LDS); the 320 x 161 DFT of 16 frames is spec_item
//      (spectral_frame.h) on v_mfma_f64_16x16x4_f64; band energies, log and floor, DCT in fp64, rounded to float32 once at the
//      store; then the decoder's own lpc_from_cepstrum (lpc_chain.h, fp32) on that float32 cepstrum.  Writes outputs 0..17 and
//      20..35; the taps in the output rows are what (B) reads.
//  (B) fenc_scores_kernel, one workgroup per frame, one lag per lane.  The frame's residual stretch and 256 samples of history
//      are recomputed from the audio with the OWNING frames' taps (frames i - 2 .. i), nothing is carried between workgroups.
//      Writes the damped scores and the sub-frame weight to the (sub-frames, 256) fp64 scratch.
//  (C) fenc_track_kernel, one workgroup per trial, serial over its sub-frames: the max-plus recursion with one state per lane,
//      the argmax as a workgroup reduction with the first index winning ties.  Writes outputs 18 and 19.
//
// Sums whose order decides equal bits with the reference for equal inputs (DCT, residual, track) add their terms in its order;
// the build forbids contraction.
#include "feature_encoder.h"
#include "spectral_frame.h"

#define FENC_XROWS (FENC_TILE_FRAMES * FENC_FRAME + FENC_FRAME)      // samples the windows of a tile cover
#define FENC_RS (FENC_XROWS | 1)
#define FENC_PW 163                                                   // stride of a frame's power spectrum in LDS
#define FENC_PREEMPH ((double)0.85f)

static_assert(FENC_TILE_FRAMES == 16, "one MFMA tile of frames; the LPC passes take them eight at a time");

__constant__ int c_fenc_edges[DSS_NB_BANDS] = {0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 136, 160};

__device__ __forceinline__ double fenc_preemph(const short *__restrict__ s, long long t, long long n)
{
    if (t < 0 || t >= n) return 0.0;
    const double prev = t > 0 ? (double)s[t - 1] : 0.0;
    return (double)s[t] + (-FENC_PREEMPH) * prev;
}

// ---- (A) ---------------------------------------------------------------------------------------------------------------
// LDS, in doubles: [tw 640 | win 320 | mean 16] [xs FENC_RS] [pw 16 x FENC_PW].  Behind the DFT the first region holds the LPC
// chain's per-frame scratch (floats), the second the band values, the float32 cepstrum and the chain's cosine table.
#define FENC_R0 976
#define FENC_LDS (FENC_R0 + FENC_RS + FENC_TILE_FRAMES * FENC_PW)

__global__ void __launch_bounds__(FENC_THREADS)
fenc_spectrum_kernel(DssFencDev v, const short *__restrict__ audio, const DssFencTrial *__restrict__ desc,
                     const DssFencTile *__restrict__ tiles, float *__restrict__ out36)
{
    __shared__ __attribute__((aligned(16))) double lds[FENC_LDS];
    const DssFencTile tile = tiles[blockIdx.x];
    const DssFencTrial d = desc[tile.trial];
    const short *s = audio + d.first;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;

    SpecLds L;
    L.tw = reinterpret_cast<double2 *>(lds);
    L.win = lds + 640;
    L.mean = lds + 960;
    L.xs = lds + FENC_R0;
    L.extra = L.xs + FENC_RS;
    double *pw = L.extra;
    DssSpecDev p = {};
    p.nperseg = FENC_WINDOW; p.hop = FENC_FRAME; p.nfft = FENC_WINDOW; p.bins = FENC_BINS; p.nblk = (FENC_BINS + 15) / 16;
    p.K4 = FENC_WINDOW; p.sh = FENC_FRAME;
    DssSpecGeom g = {};
    g.F = FENC_TILE_FRAMES; g.f_shift = 4; g.CG = 1; g.cg_shift = 0; g.NB = 1; g.rows = FENC_XROWS; g.RS = FENC_RS;

    for (int j = tid; j < FENC_WINDOW; j += FENC_THREADS) {
        L.tw[j] = reinterpret_cast<const double2 *>(v.tw)[j];
        L.win[j] = (double)v.window[j];
    }
    if (tid < FENC_TILE_FRAMES) L.mean[tid] = 0.0;
    const long long t0 = (long long)tile.frame0 * FENC_FRAME - FENC_FRAME;
    for (int r = tid; r < FENC_RS; r += FENC_THREADS) L.xs[r] = r < FENC_XROWS ? fenc_preemph(s, t0 + r, d.n) : 0.0;
    __syncthreads();

    // the DFT of the tile's 16 frames: a wave owns one block of 16 bins at a time
    for (int blk = wave; blk < p.nblk; blk += FENC_THREADS / 64) {
        spec_d4 re0, im0, re1, im1;
        spec_item(L, p, g, 0, blk, 0, re0, im0, re1, im1);
        const int bin = blk * 16 + row;
        if (bin < FENC_BINS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const double re = re0[r] / (double)FENC_WINDOW, im = im0[r] / (double)FENC_WINDOW;
                pw[(kq + 4 * r) * FENC_PW + bin] = re * re + im * im;
            }
        }
    }
    __syncthreads();                                   // tw, win and xs are dead from here on

    double *eb = lds + FENC_R0;                                                        // [16][18] band energies, then Ly
    float *cep32 = reinterpret_cast<float *>(eb + FENC_TILE_FRAMES * DSS_NB_BANDS);    // [16][18]
    float(*ck_lds)[LPC_CK_STRIDE] = reinterpret_cast<float(*)[LPC_CK_STRIDE]>(cep32 + FENC_TILE_FRAMES * DSS_NB_BANDS);
    static_assert((FENC_TILE_FRAMES * DSS_NB_BANDS * 3 + 160 * LPC_CK_STRIDE) / 2 <= FENC_RS, "the second region holds them");
    lpc_chain_load_ck(v.lpc, ck_lds, tid, FENC_THREADS);
    for (int it = tid; it < FENC_TILE_FRAMES * DSS_NB_BANDS; it += FENC_THREADS) {    // band energies: the triangular partition
        const int f = it / DSS_NB_BANDS, i = it - f * DSS_NB_BANDS;
        const double *q = pw + f * FENC_PW;
        double e = 0.0;
        if (i > 0) {
            const int lo = c_fenc_edges[i - 1], width = c_fenc_edges[i] - lo;
            for (int j = 0; j < width; ++j) e += ((double)j / (double)width) * q[lo + j];
        }
        if (i < DSS_NB_BANDS - 1) {
            const int lo = c_fenc_edges[i], width = c_fenc_edges[i + 1] - lo;
            for (int j = 0; j < width; ++j) e += (1.0 - (double)j / (double)width) * q[lo + j];
        } else {
            e += q[FENC_WINDOW / 2];                    // the last edge belongs wholly to the last band
        }
        if (i == 0 || i == DSS_NB_BANDS - 1) e *= 2.0;
        eb[it] = e;
    }
    __syncthreads();
    if (tid < FENC_TILE_FRAMES) {                                                     // log and floor: sequential over the bands
        double *e = eb + tid * DSS_NB_BANDS;
        double log_max = -2.0, follow = -2.0;
        for (int i = 0; i < DSS_NB_BANDS; ++i) {
            double ly = log10(1e-2 + e[i]);
            ly = fmax(log_max - 8.0, fmax(follow - 2.5, ly));
            e[i] = ly;
            log_max = fmax(log_max, ly);
            follow = fmax(follow - 2.5, ly);
        }
    }
    __syncthreads();
    for (int it = tid; it < FENC_TILE_FRAMES * DSS_NB_BANDS; it += FENC_THREADS) {    // DCT, the bands added in ascending order
        const int f = it / DSS_NB_BANDS, j = it - f * DSS_NB_BANDS;
        const double *ly = eb + f * DSS_NB_BANDS;
        double sum = 0.0;
        for (int i = 0; i < DSS_NB_BANDS; ++i) sum = sum + ly[i] * (double)v.lpc.dct_table[i * DSS_NB_BANDS + j];
        double c = sum * v.idct_scale;
        if (j == 0) c -= 4.0;
        const float c32 = (float)c;
        cep32[it] = c32;
        if (tile.frame0 + f < d.frames) out36[(d.out + tile.frame0 + f) * FENC_OUT + j] = c32;
    }
    __syncthreads();

    // the decoder's lpc_from_cepstrum on the float32 cepstrum: 32 lanes per frame, eight frames per pass
    float *fs = reinterpret_cast<float *>(lds);
    const int sub = tid >> 5, l = tid & 31;
    float *cs = fs + sub * 220, *exs = cs + 20, *as = cs + 40, *xr = cs + 60;
    static_assert(8 * 220 <= 2 * FENC_R0, "the first region holds the chain's scratch");
    for (int pass = 0; pass < FENC_TILE_FRAMES / 8; ++pass) {
        const int f = pass * 8 + sub;
        __syncthreads();
        if (l < DSS_NB_BANDS) cs[l] = l == 0 ? cep32[f * DSS_NB_BANDS] + 4 : cep32[f * DSS_NB_BANDS + l];
        __syncthreads();
        float lpc[DSS_LPC_ORDER];
        lpc_chain_frame(v.lpc, v.idct_scale, ck_lds, cs, exs, xr, as, l, lpc);
        if (l == 0 && tile.frame0 + f < d.frames) {
            float *dst = out36 + (d.out + tile.frame0 + f) * FENC_OUT + 20;
#pragma unroll
            for (int i = 0; i < DSS_LPC_ORDER; ++i) dst[i] = lpc[i];
        }
    }
}

// ---- (B) ---------------------------------------------------------------------------------------------------------------
// Frame i of a trial: e over t = 160 i - 336 .. 160 i + 80 (416 samples: 256 of history, the frame's 160), from r over one
// sample more and x over sixteen more.  Sample t takes the taps of frame (t + 80) / 160; before t = -80 everything is zero.
#define FENC_NE 416
#define FENC_NR (FENC_NE + 1)
#define FENC_NX (FENC_NR + DSS_LPC_ORDER)

__global__ void __launch_bounds__(FENC_THREADS)
fenc_scores_kernel(const short *__restrict__ audio, const DssFencTrial *__restrict__ desc, const DssFencTile *__restrict__ tiles,
                   const float *__restrict__ out36, double *__restrict__ scores)
{
    __shared__ double xs[FENC_NX], rs[FENC_NR], es[FENC_NE], xcs[FENC_LAGS];
    __shared__ float lp[3][DSS_LPC_ORDER];
    const DssFencTile tile = tiles[blockIdx.x / FENC_TILE_FRAMES];
    const DssFencTrial d = desc[tile.trial];
    const int i = tile.frame0 + (int)(blockIdx.x % FENC_TILE_FRAMES);
    if (i >= d.frames) return;
    const short *s = audio + d.first;
    const int q = threadIdx.x;
    const long long tb = (long long)i * FENC_FRAME - (FENC_NE - FENC_FRAME / 2 + 1);      // t of rs[0]: 160 i - 337

    if (q < 3 * DSS_LPC_ORDER) {
        const int fr = i - 2 + q / DSS_LPC_ORDER;
        lp[q / DSS_LPC_ORDER][q % DSS_LPC_ORDER] = fr >= 0 ? out36[(d.out + fr) * FENC_OUT + 20 + q % DSS_LPC_ORDER] : 0.f;
    }
    for (int m = q; m < FENC_NX; m += FENC_THREADS) xs[m] = fenc_preemph(s, tb - DSS_LPC_ORDER + m, d.n);
    __syncthreads();
    for (int k = q; k < FENC_NR; k += FENC_THREADS) {
        const long long t = tb + k;
        double acc = 0.0;
        if (t >= -(FENC_FRAME / 2)) {
            const float *a = lp[(int)((t + FENC_FRAME / 2) / FENC_FRAME) - (i - 2)];
            acc = xs[k + DSS_LPC_ORDER];
            for (int j = 0; j < DSS_LPC_ORDER; ++j) acc = acc + (double)a[j] * xs[k + DSS_LPC_ORDER - 1 - j];
        }
        rs[k] = acc;
    }
    __syncthreads();
    for (int m = q; m < FENC_NE; m += FENC_THREADS) es[m] = rs[m + 1] + 0.7 * rs[m];
    __syncthreads();

    double xc[2], aa[2];
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        const double *A = es + FENC_LAGS + 80 * u, *B = es + 80 * u + q;      // lag 256 - q: the sub-frame shifted back
        double ab = 0.0, bb = 0.0, a2 = 0.0;
        for (int k = 0; k < 80; ++k) {
            const double a = A[k], b = B[k];
            ab += a * b;
            bb += b * b;
            a2 += a * a;
        }
        double x = 2.0 * ab / fmax(1.0, 1.0 + a2 + bb);
        xcs[q] = x;
        __syncthreads();
        if (q < 192) {                                                         // sub-harmonic damping, on the undamped values
            const double h = fmax(fmax(xcs[(256 + q) / 2], xcs[(256 + q + 2) / 2]), xcs[(256 + q - 1) / 2]);
            if (x < 1.1 * h) x *= 0.8;
        }
        __syncthreads();
        xc[u] = x;
        aa[u] = a2;
    }
    const double tot = aa[0] + aa[1] + 1e-15;
    double *dst = scores + (2 * (d.out + i)) * FENC_LAGS + q;
    dst[0] = q == FENC_LAGS - 1 ? 2.0 * aa[0] / tot : xc[0];
    dst[FENC_LAGS] = q == FENC_LAGS - 1 ? 2.0 * aa[1] / tot : xc[1];
}

// ---- (C) ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FENC_THREADS)
fenc_track_kernel(const DssFencTrial *__restrict__ desc, const double *__restrict__ scores, float *__restrict__ out36)
{
    __shared__ double P[FENC_TRACK], red_v[FENC_THREADS / 64];
    __shared__ int red_i[FENC_THREADS / 64], bp[FENC_TRACK];
    const DssFencTrial d = desc[blockIdx.x];
    const int q = threadIdx.x, lane = q & 63, wave = q >> 6;
    const bool on = q < FENC_TRACK;
    if (on) P[q] = 0.0;
    double p_all = 0.0;
    int best = 0;
    __syncthreads();
    for (int sf = 0; sf < 2 * d.frames; ++sf) {
        const double *row = scores + (2 * d.out + sf) * FENC_LAGS;
        const double g = row[FENC_LAGS - 1];
        double pn = -INFINITY;
        int ptr = best;
        if (on) {
            double prev = p_all - 6.0;
#pragma unroll
            for (int dd = -4; dd <= 4; ++dd) {
                if (q + dd >= 0 && q + dd < FENC_TRACK) {
                    const double c = P[q + dd] - 0.02 * (double)(dd * dd);
                    if (c > prev) { prev = c; ptr = q + dd; }
                }
            }
            pn = prev + g * row[q];
        }
        // argmax over the workgroup, the first index on ties
        double bv = pn;
        int bi = q;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double ov = __shfl_down(bv, off, 64);
            const int oi = __shfl_down(bi, off, 64);
            if (ov > bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
        }
        if (lane == 0) { red_v[wave] = bv; red_i[wave] = bi; }
        __syncthreads();
        bv = red_v[0]; bi = red_i[0];
#pragma unroll
        for (int w = 1; w < FENC_THREADS / 64; ++w)
            if (red_v[w] > bv) { bv = red_v[w]; bi = red_i[w]; }              // a later wave's indices are larger: ties keep the earlier
        if (on) {
            P[q] = pn - bv;
            if (sf & 1) bp[q] = ptr;
        }
        p_all = bv;
        best = bi;
        __syncthreads();
        if ((sf & 1) && q == 0) {
            const int q1 = best, q0 = bp[q1];
            int period2 = (256 - q0) + (256 - q1);
            period2 = period2 < 66 ? 66 : (period2 > 510 ? 510 : period2);
            const double *r0 = row - FENC_LAGS;
            float *dst = out36 + (d.out + (sf >> 1)) * FENC_OUT;
            dst[18] = (float)(0.01 * (double)(period2 - 200));
            dst[19] = (float)((r0[FENC_LAGS - 1] * r0[q0] + g * row[q1]) / 2.0 - 0.5);
        }
    }
}

int dss_launch_fenc(const DssFencDev &v, const short *d_audio, const DssFencTrial *d_desc, int n_trials, const DssFencTile *d_tiles,
                    int n_tiles, float *d_out36, double *d_scores, hipStream_t s, const hipEvent_t *stamps)
{
    if (n_tiles < 1) return DSS_OK;
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[0], s));
    hipLaunchKernelGGL(fenc_spectrum_kernel, dim3(n_tiles), dim3(FENC_THREADS), 0, s, v, d_audio, d_desc, d_tiles, d_out36);
    DSS_HIP_CHECK(hipGetLastError());
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[1], s));
    hipLaunchKernelGGL(fenc_scores_kernel, dim3((unsigned)n_tiles * FENC_TILE_FRAMES), dim3(FENC_THREADS), 0, s, d_audio, d_desc, d_tiles,
                       d_out36, d_scores);
    DSS_HIP_CHECK(hipGetLastError());
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[2], s));
    hipLaunchKernelGGL(fenc_track_kernel, dim3(n_trials), dim3(FENC_THREADS), 0, s, d_desc, d_scores, d_out36);
    DSS_HIP_CHECK(hipGetLastError());
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[3], s));
    return DSS_OK;
}
