// csrc/contamination.hip -- lagged correlations between the spectrogram of the audio and the spectrograms of every ECoG channel
// (Part 12 of include/dss_hip.h): the sums from which the acoustic contamination analysis takes its Pearson correlations.
//
// With A[t][i] the magnitude of kept bin i of audio frame t less a per-bin constant, N_c[t][j] the magnitude of kept bin j of
// frame t of channel c, k[t] the frame mask and lag l in -L .. L, one call gives, over the frames t with 0 <= t + l < W,
//     n[l]        = sum k[t] k[t+l]                sa[l][i] = sum k[t] k[t+l] A[t+l][i]       saa[l][i] = sum k[t] k[t+l] A[t+l][i]^2
//     sb[l][c][j] = sum k[t] k[t+l] N_c[t][j]      sbb[l][c][j] = sum k[t] k[t+l] N_c[t][j]^2
//     sab[l][c][i][j] = sum k[t] k[t+l] A[t+l][i] N_c[t][j].
// The frames are those of spectral.hip (spectral_frame.h): same staging, same DFT on v_mfma_f64_16x16x4_f64, no detrending, and
// the magnitude without scipy's scale factor, which no correlation sees.  Everything is float64; the library is built with
// -ffp-contract=off, so every fused multiply-add is written out.  No atomics: partial sums per workgroup in one fixed order, then
// one finishing pass that adds them in order, so a result does not depend on scheduling.
//
// Launches of a call:
//   contam_audio_kernel     the audio's kept bins, frame after frame, as aud[t][32]: places 0 .. B hold k[t] |X|, place B holds
//                           k[t] itself, the rest zeros (B <= 31).  W x 32 doubles; kept for the call.
//   contam_shift_kernel     the mean of every kept bin over the kept frames, 256 strided sums and a tree, both in fixed order.
//   contam_center_kernel    aud[t][i] -= shift[i] on the kept frames: sab - sa sb / n then does not cancel on the audio side.
//   contam_audio_sums_kernel  n, sa, saa: one workgroup per lag.
//   contam_corr_kernel      grid (chunks of frame tiles, channels, Z lag groups), four waves.  Per tile of 32 frames the workgroup
//                           stages the channel's rows (spec_stage) and the audio frames tile .. tile + 31 shifted by each of its
//                           lags as aw[frame][48]; waves 0 and 1 take the DFT of bin blocks 0 and 1 (spec_item) and leave the
//                           masked magnitudes in LDS in the accumulator's own layout, [register][lane]; then every wave contracts
//                           them with the audio at its own `lgn` <= 8 lags: M = 32 audio places x N = 32 neural bins x K = 32
//                           frames, four MFMAs per (lag, 4 frames).  Register r of lane l of spec_item's result is [frame
//                           (l >> 4) + 4 r][bin l & 15], which is the B operand of K block r as it stands; the A operand is
//                           aw[frame (l >> 4) + 4 r + lag][place l & 15].  Row B of the result (the mask riding along) is sb.
//                           sbb is taken beside the MFMAs on the vector unit, per lane, and its four K positions are added in the
//                           finishing pass.  The accumulators (36 VGPRs per lag) stay in registers across the chunk's tiles.
//   contam_finish_kernel    adds the chunks' records in chunk order.
#include "contamination.h"
#include "spectral_frame.h"

__device__ __forceinline__ double contam_mag(double re, double im) { return __builtin_sqrt(__builtin_fma(re, re, im * im)); }

__global__ void __launch_bounds__(SPEC_THREADS)
contam_audio_kernel(const double *__restrict__ audio, long long T, int W, const unsigned char *__restrict__ keep, DssContamDev v,
                    double *__restrict__ aud)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const DssSpecDev &p = v.spec;
    const DssSpecGeom &g = v.geom;
    const SpecLds L = spec_lds(lds, p, g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, kq = lane >> 4;
    const long long f0 = (long long)blockIdx.x * CONTAM_F;
    const DssSpecTrial d = {0, T, 0, W, 0};

    spec_load_tables(L, p);
    spec_stage(L, p, g, audio, 1, 1, d, f0, 0);
    __syncthreads();
    spec_means(L, p, g);
    __syncthreads();
    if (wave >= CONTAM_PAD / 16) return;
    spec_d4 re0, im0, re1, im1;
    spec_item(L, p, g, 0, wave, v.bin_lo, re0, im0, re1, im1);
    const int col = wave * 16 + row;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const long long f = f0 + kq + 4 * r;
        if (f < W) {
            const double k = keep[f] ? 1.0 : 0.0;
            aud[f * CONTAM_PAD + col] = col < v.B ? k * contam_mag(re0[r], im0[r]) : (col == v.B ? k : 0.0);
        }
        if (f + 16 < W) {
            const double k = keep[f + 16] ? 1.0 : 0.0;
            aud[(f + 16) * CONTAM_PAD + col] = col < v.B ? k * contam_mag(re1[r], im1[r]) : (col == v.B ? k : 0.0);
        }
    }
}

// grid (CONTAM_PAD): place blockIdx.x.  Thread i adds frames i, i + 256, ... in order; then a tree over the 256 sums.
__global__ void __launch_bounds__(SPEC_THREADS)
contam_shift_kernel(const double *__restrict__ aud, int W, int B, double *__restrict__ shift, double *__restrict__ out_shift)
{
    __shared__ double sv[SPEC_THREADS], sn[SPEC_THREADS];
    const int col = blockIdx.x, tid = threadIdx.x;
    double a = 0.0, n = 0.0;
    for (long long t = tid; t < W; t += SPEC_THREADS) {
        a += aud[t * CONTAM_PAD + col];
        n += aud[t * CONTAM_PAD + B];
    }
    sv[tid] = a; sn[tid] = n;
    __syncthreads();
    for (int s = SPEC_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) { sv[tid] += sv[tid + s]; sn[tid] += sn[tid + s]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double m = (col < B && sn[0] > 0.0) ? sv[0] / sn[0] : 0.0;
        shift[col] = m;
        if (col < B) out_shift[col] = m;
    }
}

__global__ void __launch_bounds__(SPEC_THREADS)
contam_center_kernel(double *__restrict__ aud, int W, int B, const double *__restrict__ shift)
{
    const long long q = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
    const long long t = q / CONTAM_PAD;
    const int col = (int)(q - t * CONTAM_PAD);
    if (t >= W || col >= B) return;
    if (aud[t * CONTAM_PAD + B] != 0.0) aud[q] -= shift[col];
}

// grid (nlag), 1024 threads: thread (place, one of 32 strides) adds its frames in order, then thread `place` adds the 32 strides.
__global__ void __launch_bounds__(CONTAM_AUD_THREADS)
contam_audio_sums_kernel(const double *__restrict__ aud, int W, int B, int L, double *__restrict__ out_n, double *__restrict__ out_sa,
                         double *__restrict__ out_saa)
{
    __shared__ double s1[CONTAM_AUD_THREADS], s2[CONTAM_AUD_THREADS];
    const int li = blockIdx.x, lag = li - L, tid = threadIdx.x, col = tid & (CONTAM_PAD - 1), sub = tid / CONTAM_PAD;
    double a = 0.0, aa = 0.0;
    for (long long t = sub; t < W; t += CONTAM_AUD_THREADS / CONTAM_PAD) {
        const long long t2 = t + lag;
        if (t2 < 0 || t2 >= W) continue;
        const double k = aud[t * CONTAM_PAD + B], x = aud[t2 * CONTAM_PAD + col];
        a = __builtin_fma(k, x, a);
        aa = __builtin_fma(k * x, x, aa);
    }
    s1[tid] = a; s2[tid] = aa;
    __syncthreads();
    if (tid >= CONTAM_PAD) return;
    a = 0.0; aa = 0.0;
    for (int s = 0; s < CONTAM_AUD_THREADS / CONTAM_PAD; ++s) { a += s1[s * CONTAM_PAD + col]; aa += s2[s * CONTAM_PAD + col]; }
    if (col < B) { out_sa[(long long)li * B + col] = a; out_saa[(long long)li * B + col] = aa; }
    else if (col == B) out_n[li] = a;
}

__global__ void __launch_bounds__(SPEC_THREADS)
contam_corr_kernel(const double *__restrict__ x, int ld, int C, long long T, int W, const double *__restrict__ aud, DssContamDev v,
                   int tiles_per_chunk, double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const DssSpecDev &p = v.spec;
    const DssSpecGeom &g = v.geom;
    const SpecLds L = spec_lds(lds, p, g);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, kq = lane >> 4;
    const int B = v.B, nlz = CONTAM_WAVES * v.lgn, awrows = CONTAM_F + nlz - 1;
    double *aw = L.extra;                            // [awrows][CONTAM_AS]: audio frames tile + first lag of the group ..
    double *mg = aw + awrows * CONTAM_AS;            // [2 blocks][8 registers][64 lanes]
    const int c = blockIdx.y, zlag0 = blockIdx.z * nlz, li0 = zlag0 + wave * v.lgn;
    const int nl = max(0, min(v.lgn, v.nlag - li0));
    const DssSpecTrial d = {0, T, 0, W, 0};
    const int n_tiles = (W + CONTAM_F - 1) / CONTAM_F;
    const int tile0 = blockIdx.x * tiles_per_chunk, tile1 = min(n_tiles, tile0 + tiles_per_chunk);

    const spec_d4 zero = {0.0, 0.0, 0.0, 0.0};
    spec_d4 acc[CONTAM_LG][4];
    double sq[CONTAM_LG][2];
#pragma unroll
    for (int j = 0; j < CONTAM_LG; ++j) {
        acc[j][0] = zero; acc[j][1] = zero; acc[j][2] = zero; acc[j][3] = zero;
        sq[j][0] = 0.0; sq[j][1] = 0.0;
    }

    spec_load_tables(L, p);
    for (int tile = tile0; tile < tile1; ++tile) {
        const long long f0 = (long long)tile * CONTAM_F;
        __syncthreads();                             // the tile before is done with xs, mean, aw and mg
        spec_stage(L, p, g, x, ld, C, d, f0, c);
        for (int q = threadIdx.x; q < awrows * CONTAM_PAD; q += SPEC_THREADS) {
            const int r = q / CONTAM_PAD, col = q - r * CONTAM_PAD;
            const long long t2 = f0 + zlag0 - v.L + r;
            aw[r * CONTAM_AS + col] = (t2 >= 0 && t2 < W) ? aud[t2 * CONTAM_PAD + col] : 0.0;
        }
        __syncthreads();
        spec_means(L, p, g);
        __syncthreads();
        if (wave < CONTAM_PAD / 16) {
            spec_d4 re0, im0, re1, im1;
            spec_item(L, p, g, 0, wave, v.bin_lo, re0, im0, re1, im1);
            const bool live = wave * 16 + row < B;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const long long f = f0 + kq + 4 * r;
                const bool k0 = live && f < W && aud[f * CONTAM_PAD + B] != 0.0;
                const bool k1 = live && f + 16 < W && aud[(f + 16) * CONTAM_PAD + B] != 0.0;
                mg[(wave * 8 + r) * 64 + lane] = k0 ? contam_mag(re0[r], im0[r]) : 0.0;
                mg[(wave * 8 + 4 + r) * 64 + lane] = k1 ? contam_mag(re1[r], im1[r]) : 0.0;
            }
        }
        __syncthreads();
        double b[2][8], bb[2][8];
#pragma unroll
        for (int kb = 0; kb < 8; ++kb) {
            b[0][kb] = mg[kb * 64 + lane];
            b[1][kb] = mg[(8 + kb) * 64 + lane];
            bb[0][kb] = b[0][kb] * b[0][kb];
            bb[1][kb] = b[1][kb] * b[1][kb];
        }
#pragma unroll
        for (int j = 0; j < CONTAM_LG; ++j) {
            if (j < nl) {
                const double *a = aw + (wave * v.lgn + j + kq) * CONTAM_AS;
#pragma unroll
                for (int kb = 0; kb < 8; ++kb) {
                    const double *ap = a + (4 * (kb & 3) + 16 * (kb >> 2)) * CONTAM_AS;
                    const double a0 = ap[row], a1 = ap[16 + row], km = ap[B];
                    acc[j][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[0][kb], acc[j][0], 0, 0, 0);
                    acc[j][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[1][kb], acc[j][1], 0, 0, 0);
                    acc[j][2] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[0][kb], acc[j][2], 0, 0, 0);
                    acc[j][3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[1][kb], acc[j][3], 0, 0, 0);
                    sq[j][0] = __builtin_fma(km, bb[0][kb], sq[j][0]);
                    sq[j][1] = __builtin_fma(km, bb[1][kb], sq[j][1]);
                }
            }
        }
    }

    const size_t rec = contam_record(B);
#pragma unroll
    for (int j = 0; j < CONTAM_LG; ++j) {
        if (j < nl) {
            double *o = partial + (((size_t)blockIdx.x * v.nlag + li0 + j) * C + c) * rec;
#pragma unroll
            for (int mn = 0; mn < 4; ++mn) {
                const int ncol = (mn & 1) * 16 + row;
                if (ncol >= B) continue;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int arow = (mn >> 1) * 16 + kq + 4 * q;
                    if (arow < B) o[arow * B + ncol] = acc[j][mn][q];
                    else if (arow == B) o[B * B + ncol] = acc[j][mn][q];
                }
            }
#pragma unroll
            for (int nb = 0; nb < 2; ++nb)
                if (nb * 16 + row < B) o[B * B + B + kq * B + nb * 16 + row] = sq[j][nb];
        }
    }
}

// One thread per value of sab, sb and sbb: the chunks' records in chunk order (sbb: the four K positions of a chunk in order).
__global__ void __launch_bounds__(SPEC_THREADS)
contam_finish_kernel(const double *__restrict__ partial, int chunks, long long pairs, int B, double *__restrict__ out_sb,
                     double *__restrict__ out_sbb, double *__restrict__ out_sab)
{
    const long long per = (long long)B * B + 2 * B, e = (long long)blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (e >= pairs * per) return;
    const long long lc = e / per;
    const int k = (int)(e - lc * per);
    const size_t rec = contam_record(B);
    double s = 0.0;
    if (k < B * B + B) {
        for (int ch = 0; ch < chunks; ++ch) s += partial[((size_t)ch * pairs + lc) * rec + k];
        if (k < B * B) out_sab[lc * B * B + k] = s;
        else out_sb[lc * B + k - B * B] = s;
    } else {
        const int col = k - B * B - B;
        for (int ch = 0; ch < chunks; ++ch)
            for (int q = 0; q < 4; ++q) s += partial[((size_t)ch * pairs + lc) * rec + B * B + B + q * B + col];
        out_sbb[lc * B + col] = s;
    }
}

// ---- host side of the launches --------------------------------------------------------------------------------------------
bool dss_contam_shape(int nperseg, int hop, int bin_lo, int n_bins, int max_lag, DssContamDev *v)
{
    DssSpecDev &d = v->spec;
    d.nperseg = nperseg; d.hop = hop; d.nfft = nperseg; d.bins = nperseg / 2 + 1; d.nblk = (d.bins + 15) / 16;
    d.K4 = (nperseg + 3) & ~3; d.sh = hop < d.K4 ? hop : d.K4;
    d.mode = DSS_SPEC_MAGNITUDE; d.detrend = 0; d.odd = nperseg & 1; d.scale = 1.0;
    DssSpecGeom &g = v->geom;
    g.F = CONTAM_F; g.f_shift = 5; g.CG = 1; g.cg_shift = 0; g.NB = 1;
    const long long rows = (long long)(CONTAM_F - 1) * d.sh + d.K4;
    v->bin_lo = bin_lo; v->B = n_bins; v->L = max_lag; v->nlag = 2 * max_lag + 1;
    v->Z = (v->nlag + CONTAM_WAVES * CONTAM_LG - 1) / (CONTAM_WAVES * CONTAM_LG);
    v->lgn = (v->nlag + CONTAM_WAVES * v->Z - 1) / (CONTAM_WAVES * v->Z);
    const long long spec = 2LL * d.nfft + d.K4 + CONTAM_F + (rows | 1);
    const long long all = spec + (long long)(CONTAM_F + CONTAM_WAVES * v->lgn - 1) * CONTAM_AS + 16 * 64;
    if (all * (long long)sizeof(double) > SPEC_LDS_SOFT) return false;
    g.rows = (int)rows; g.RS = (int)(rows | 1);
    g.lds_bytes = (unsigned)(spec * sizeof(double));
    v->lds_bytes = (unsigned)(all * sizeof(double));
    return true;
}

void dss_contam_layout(const DssContamDev &v, int C, long long off[8])
{
    const long long nl = v.nlag, B = v.B;
    off[0] = 0;                       // n
    off[1] = off[0] + nl;             // shift
    off[2] = off[1] + B;              // sa
    off[3] = off[2] + nl * B;         // saa
    off[4] = off[3] + nl * B;         // sb
    off[5] = off[4] + nl * C * B;     // sbb
    off[6] = off[5] + nl * C * B;     // sab
    off[7] = off[6] + nl * C * B * B;
}

int dss_launch_contam(const DssContamDev &v, const double *d_x, int ld, int C, const double *d_audio, long long T, int W,
                      const unsigned char *d_keep, double *d_aud, double *d_shift, double *d_partial, int chunks, int tiles_per_chunk,
                      double *d_out, hipStream_t s)
{
    long long off[8];
    dss_contam_layout(v, C, off);
    const int n_tiles = (W + CONTAM_F - 1) / CONTAM_F;
    DSS_HIP_CHECK(hipFuncSetAttribute((const void *)contam_audio_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.geom.lds_bytes));
    hipLaunchKernelGGL(contam_audio_kernel, dim3((unsigned)n_tiles), dim3(SPEC_THREADS), v.geom.lds_bytes, s, d_audio, T, W, d_keep, v, d_aud);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(contam_shift_kernel, dim3(CONTAM_PAD), dim3(SPEC_THREADS), 0, s, d_aud, W, v.B, d_shift, d_out + off[1]);
    DSS_HIP_CHECK(hipGetLastError());
    const long long cells = (long long)W * CONTAM_PAD;
    hipLaunchKernelGGL(contam_center_kernel, dim3((unsigned)((cells + SPEC_THREADS - 1) / SPEC_THREADS)), dim3(SPEC_THREADS), 0, s, d_aud, W,
                       v.B, d_shift);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(contam_audio_sums_kernel, dim3((unsigned)v.nlag), dim3(CONTAM_AUD_THREADS), 0, s, d_aud, W, v.B, v.L, d_out + off[0],
                       d_out + off[2], d_out + off[3]);
    DSS_HIP_CHECK(hipGetLastError());
    DSS_HIP_CHECK(hipFuncSetAttribute((const void *)contam_corr_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)v.lds_bytes));
    hipLaunchKernelGGL(contam_corr_kernel, dim3((unsigned)chunks, (unsigned)C, (unsigned)v.Z), dim3(SPEC_THREADS), v.lds_bytes, s,
                       d_x, ld, C, T, W, d_aud, v, tiles_per_chunk, d_partial);
    DSS_HIP_CHECK(hipGetLastError());
    const long long pairs = (long long)v.nlag * C, vals = pairs * ((long long)v.B * v.B + 2 * v.B);
    hipLaunchKernelGGL(contam_finish_kernel, dim3((unsigned)((vals + SPEC_THREADS - 1) / SPEC_THREADS)), dim3(SPEC_THREADS), 0, s, d_partial,
                       chunks, pairs, v.B, d_out + off[4], d_out + off[5], d_out + off[6]);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
