// csrc/spectral.hip -- spectrograms of the trials of a recording, and two reductions over them (Part 11 of include/dss_hip.h).
//
// What scipy.signal.spectrogram(x, fs, window, nperseg, noverlap, nfft, detrend, mode) gives per trial and channel, as the
// reference's per-electrode spectral analysis calls it (eval/suppl_fig_2.py:41-92, eval/figure_2ab.py:30-31): frames of
// `nperseg` rows every `hop` rows with no padding, the frame's mean removed, times the window, the DFT at bins 0 .. nfft / 2 of
// the frame zero-padded to nfft, then the one-sided power density or the magnitude.  scipy's arithmetic is pocketfft, not a fixed
// C sequence, so parity is a tolerance (tests/test_gpu_spectral.py derives it); the library is built with -ffp-contract=off, so
// every fused multiply-add here is written out (__builtin_fma, the fp64 MFMA).  Everything is float64.  All three kernels are
// pure functions of their arguments: no atomics, every sum in one fixed order, and a frame's value does not depend on the list
// it came in.
//
// The frame arithmetic is shared (spec_stage, spec_means, spec_item).  A workgroup stages the rows that F consecutive frames of
// ONE trial cover, for CG channels, in LDS as xs[channel][row] (row-segment loads of CG doubles, coalesced; overlapping frames
// then re-read LDS, not HBM).  Frame f starts at row f * sh, sh = min(hop, K4) with K4 = 4 * ceil(nperseg / 4): frames that
// overlap share their rows, frames that do not are staged back to back.  The DFT is the product of avad_energy_kernel
// (acoustic_vad.hip) on v_mfma_f64_16x16x4_f64: A = 16 detrended, windowed frames x 4 samples, B = 4 samples x 16 bins of cos
// (and of sin) gathered from ONE table of cos / sin(2 pi j / nfft) in LDS at (bin * sample) mod nfft, advanced by 4 * bin per
// step.  Lane l holds A[frame l & 15][sample l >> 4] and B[sample l >> 4][bin l & 15]; of the f64 result, register r of lane l
// is [frame (l >> 4) + 4 r][bin l & 15].  Samples nperseg .. K4 - 1, frames beyond F and bins beyond nfft / 2 enter as zeros or
// are not stored.  A wave owns one (channel, block of 16 bins) at a time and both 16-frame halves of the tile, so one gathered
// (cos, sin) pair feeds four MFMAs.
#include "spectral_frame.h"

// scipy's scaling: |X|^2 * scale, doubled except at bin 0 and, for even nfft, the last bin; or |X| * sqrt(scale).
__device__ __forceinline__ double spec_value(const DssSpecDev &p, double re, double im, int bin)
{
    const double s = __builtin_fma(re, re, im * im);
    if (p.mode == DSS_SPEC_MAGNITUDE) return __builtin_sqrt(s) * p.scale;
    const double v = s * p.scale;
    return (bin == 0 || (bin == p.bins - 1 && !p.odd)) ? v : 2.0 * v;
}

// ---- spectrograms of a trial list ------------------------------------------------------------------------------------
// grid (tiles, channel groups).  out is (sum W_i, C, bins): frame after frame, trial after trial in list order.
__global__ void __launch_bounds__(SPEC_THREADS)
spec_trials_kernel(const double *__restrict__ x, int ld, int C, const DssSpecTrial *__restrict__ desc, const DssSpecTile *__restrict__ tiles,
                   DssSpecDev p, DssSpecGeom g, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const SpecLds L = spec_lds(lds, p, g);
    const DssSpecTile tile = tiles[blockIdx.x];
    const DssSpecTrial d = desc[tile.trial];
    const int c0 = blockIdx.y << g.cg_shift;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, kq = lane >> 4;

    spec_load_tables(L, p);
    spec_stage(L, p, g, x, ld, C, d, tile.frame0, c0);
    __syncthreads();
    spec_means(L, p, g);
    __syncthreads();

    const int live_c = min(g.CG, C - c0);
    for (int it = wave; it < live_c * p.nblk; it += SPEC_THREADS / 64) {
        const int c = it / p.nblk, blk = it - c * p.nblk;
        spec_d4 re0, im0, re1, im1;
        spec_item(L, p, g, c, blk, 0, re0, im0, re1, im1);
        const int bin = blk * 16 + row;
        if (bin < p.bins) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = tile.frame0 + kq + 4 * r;
                if (kq + 4 * r < g.F && f < d.W)
                    out[((d.out + f) * C + c0 + c) * p.bins + bin] = spec_value(p, re0[r], im0[r], bin);
                if (kq + 4 * r + 16 < g.F && f + 16 < d.W)
                    out[((d.out + f + 16) * C + c0 + c) * p.bins + bin] = spec_value(p, re1[r], im1[r], bin);
            }
        }
    }
}

// ---- the mean over trials of the frames around every trial's own onset --------------------------------------------------
// grid (ranges of F columns, channel groups, groups of NB bin blocks).  Column j of the (C, bins, J) result is the mean over
// the trials of frame desc[i].frame0 + j of trial i.  The workgroup walks the trials in list order; every lane keeps the
// running sums of the values it computes in LDS slots of its own, which start at zero and take the trials' values one after
// the other, then divides by the number of trials: sum_i in list order, / n.
__global__ void __launch_bounds__(SPEC_THREADS)
spec_locked_kernel(const double *__restrict__ x, int ld, int C, const DssSpecTrial *__restrict__ desc, int n_trials, int J, DssSpecDev p,
                   DssSpecGeom g, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const SpecLds L = spec_lds(lds, p, g);
    const int j0 = blockIdx.x << g.f_shift, c0 = blockIdx.y << g.cg_shift, blk0 = blockIdx.z * g.NB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, kq = lane >> 4;
    const int nb = min(g.NB, p.nblk - blk0), live_c = min(g.CG, C - c0);
    const int items = live_c * nb;
    double *acc = L.extra + lane;                    // [item][half][register][lane]

    spec_load_tables(L, p);
    for (int it = wave; it < items; it += SPEC_THREADS / 64)
#pragma unroll
        for (int r = 0; r < 8; ++r) acc[(it * 8 + r) * 64] = 0.0;

    for (int i = 0; i < n_trials; ++i) {
        const DssSpecTrial d = desc[i];
        __syncthreads();                             // the trial before is done with xs and mean
        spec_stage(L, p, g, x, ld, C, d, (long long)d.frame0 + j0, c0);
        __syncthreads();
        spec_means(L, p, g);
        __syncthreads();
        for (int it = wave; it < items; it += SPEC_THREADS / 64) {
            const int c = it / nb, blk = blk0 + (it - c * nb);
            spec_d4 re0, im0, re1, im1;
            spec_item(L, p, g, c, blk, 0, re0, im0, re1, im1);
            const int bin = blk * 16 + row;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[(it * 8 + r) * 64] += spec_value(p, re0[r], im0[r], bin);
                acc[(it * 8 + 4 + r) * 64] += spec_value(p, re1[r], im1[r], bin);
            }
        }
    }
    for (int it = wave; it < items; it += SPEC_THREADS / 64) {
        const int c = it / nb, blk = blk0 + (it - c * nb);
        const int bin = blk * 16 + row;
        if (bin >= p.bins) continue;
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int f = kq + 4 * (r & 3) + 16 * (r >> 2);
            if (f < g.F && j0 + f < J)
                out[((long long)(c0 + c) * p.bins + bin) * J + j0 + f] = acc[(it * 8 + r) * 64] / (double)n_trials;
        }
    }
}

// ---- the mean spectrum over every frame of every trial ---------------------------------------------------------------
// First launch, grid (trials, channel groups, groups of NB bin blocks): the sum over ONE trial's frames, in frame order.  A tile's
// values go to LDS as [channel][bin][frame]; then one thread per (channel, bin) adds the tile's frames, in order, to its running
// sum.  partial is (n_trials, C, bins) in list order.
__global__ void __launch_bounds__(SPEC_THREADS)
spec_mean_partial_kernel(const double *__restrict__ x, int ld, int C, const DssSpecTrial *__restrict__ desc, DssSpecDev p, DssSpecGeom g,
                         double *__restrict__ partial)
{
    extern __shared__ __attribute__((aligned(16))) double lds[];
    const SpecLds L = spec_lds(lds, p, g);
    const DssSpecTrial d = desc[blockIdx.x];
    const int c0 = blockIdx.y << g.cg_shift, blk0 = blockIdx.z * g.NB;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, row = lane & 15, kq = lane >> 4;
    const int nb = min(g.NB, p.nblk - blk0), live_c = min(g.CG, C - c0);
    const int items = live_c * nb, cols = items * 16, FP = g.F + 1;
    double *run = L.extra;                           // [item][16 bins]
    double *pt = run + g.CG * g.NB * 16;             // [item][16 bins][F + 1]

    spec_load_tables(L, p);
    for (int q = threadIdx.x; q < cols; q += SPEC_THREADS) run[q] = 0.0;

    for (int f0 = 0; f0 < d.W; f0 += g.F) {
        __syncthreads();                             // the tile before is done with xs, mean and pt
        spec_stage(L, p, g, x, ld, C, d, f0, c0);
        __syncthreads();
        spec_means(L, p, g);
        __syncthreads();
        for (int it = wave; it < items; it += SPEC_THREADS / 64) {
            const int c = it / nb, blk = blk0 + (it - c * nb);
            spec_d4 re0, im0, re1, im1;
            spec_item(L, p, g, c, blk, 0, re0, im0, re1, im1);
            const int bin = blk * 16 + row;
            double *o = pt + (it * 16 + row) * FP + kq;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (kq + 4 * r < g.F) o[4 * r] = spec_value(p, re0[r], im0[r], bin);
                if (kq + 4 * r + 16 < g.F) o[4 * r + 16] = spec_value(p, re1[r], im1[r], bin);
            }
        }
        __syncthreads();
        const int nf = min(g.F, d.W - f0);
        for (int q = threadIdx.x; q < cols; q += SPEC_THREADS) {
            const double *v = pt + q * FP;
            double s = run[q];
            for (int f = 0; f < nf; ++f) s += v[f];
            run[q] = s;
        }
    }
    __syncthreads();
    for (int q = threadIdx.x; q < cols; q += SPEC_THREADS) {
        const int it = q >> 4, c = it / nb, bin = (blk0 + it - c * nb) * 16 + (q & 15);
        if (bin < p.bins) partial[((long long)d.out * C + c0 + c) * p.bins + bin] = run[q];
    }
}

// Second launch: the trials' sums added in list order, over the number of frames.
__global__ void __launch_bounds__(SPEC_THREADS)
spec_mean_finish_kernel(const double *__restrict__ partial, int n_trials, int cols, double frames, double *__restrict__ out)
{
    const int q = blockIdx.x * SPEC_THREADS + threadIdx.x;
    if (q >= cols) return;
    double s = 0.0;
    for (int i = 0; i < n_trials; ++i) s += partial[(long long)i * cols + q];
    out[q] = s / frames;
}

// ---- host side of the launches --------------------------------------------------------------------------------------------
static size_t spec_lds_bytes(const DssSpecDev &v, int kind, int F, int CG, int NB)
{
    const size_t rows = (size_t)(F - 1) * v.sh + v.K4, RS = rows | 1;
    size_t n = (size_t)2 * v.nfft + v.K4 + (size_t)F * CG + (size_t)CG * RS;
    if (kind == SPEC_KIND_LOCKED) n += (size_t)CG * NB * 8 * 64;
    if (kind == SPEC_KIND_MEAN) n += (size_t)CG * NB * 16 * (F + 2);
    return n * sizeof(double);
}

bool dss_spec_pick_geom(const DssSpecDev &v, int C, int kind, DssSpecGeom *g)
{
    int cg_max = 1;
    while (cg_max < 16 && cg_max < C) cg_max <<= 1;
    // the first that fits, most frames first (the MFMA's 16 rows filled), then most bin blocks (the rows staged once), then channels.
    // Inside the limits of dss_spec_check_params the last candidate always fits: F = CG = 1 with NB = 1 (all nblk blocks for the
    // spectrograms, which keep nothing per block) asks for at most 2 * 2048 + 2048 + 1 + 2049 + 512 doubles = 69648 bytes.
    for (int F = 32; F >= 1; F >>= 1) {
        for (int NB = v.nblk;; NB = (NB + 1) / 2) {
            for (int CG = cg_max; CG >= 1; CG >>= 1) {
                const size_t bytes = spec_lds_bytes(v, kind, F, CG, NB);
                if (bytes > SPEC_LDS_SOFT) continue;
                g->F = F; g->CG = CG; g->NB = NB;
                g->f_shift = __builtin_ctz((unsigned)F); g->cg_shift = __builtin_ctz((unsigned)CG);
                g->rows = (F - 1) * v.sh + v.K4; g->RS = g->rows | 1;
                g->lds_bytes = (unsigned)bytes;
                return true;
            }
            if (NB == 1 || kind == SPEC_KIND_TRIALS) break;
        }
    }
    return false;
}

static int spec_grid_ok(long long y, long long z)
{
    if (y > 65535 || z > 65535) { dss_set_error("spectrogram: too many channels for one launch"); return DSS_EINVAL; }
    return DSS_OK;
}

int dss_launch_spec_trials(const DssSpecDev &v, const DssSpecGeom &g, const double *d_x, int ld, int C, const DssSpecTrial *d_desc,
                           const DssSpecTile *d_tiles, int n_tiles, double *d_out, hipStream_t s)
{
    if (n_tiles <= 0) return DSS_OK;
    const int groups = (C + g.CG - 1) / g.CG;
    if (spec_grid_ok(groups, 1)) return DSS_EINVAL;
    DSS_HIP_CHECK(hipFuncSetAttribute((const void *)spec_trials_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes));
    hipLaunchKernelGGL(spec_trials_kernel, dim3((unsigned)n_tiles, (unsigned)groups), dim3(SPEC_THREADS), g.lds_bytes, s, d_x, ld, C, d_desc,
                       d_tiles, v, g, d_out);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

int dss_launch_spec_locked(const DssSpecDev &v, const DssSpecGeom &g, const double *d_x, int ld, int C, const DssSpecTrial *d_desc,
                           int n_trials, int J, double *d_out, hipStream_t s)
{
    if (n_trials <= 0 || J <= 0) return DSS_OK;
    const int groups = (C + g.CG - 1) / g.CG, zs = (v.nblk + g.NB - 1) / g.NB;
    if (spec_grid_ok(groups, zs)) return DSS_EINVAL;
    DSS_HIP_CHECK(hipFuncSetAttribute((const void *)spec_locked_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes));
    hipLaunchKernelGGL(spec_locked_kernel, dim3((unsigned)((J + g.F - 1) / g.F), (unsigned)groups, (unsigned)zs), dim3(SPEC_THREADS),
                       g.lds_bytes, s, d_x, ld, C, d_desc, n_trials, J, v, g, d_out);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

int dss_launch_spec_mean(const DssSpecDev &v, const DssSpecGeom &g, const double *d_x, int ld, int C, const DssSpecTrial *d_desc,
                         int n_trials, long long total_frames, double *d_partial, double *d_out, hipStream_t s)
{
    if (n_trials <= 0) return DSS_OK;
    const int groups = (C + g.CG - 1) / g.CG, zs = (v.nblk + g.NB - 1) / g.NB;
    if (spec_grid_ok(groups, zs)) return DSS_EINVAL;
    const long long cols = (long long)C * v.bins;
    if (cols > 0x7fffffffLL) { dss_set_error("spectrogram: too many channels for one launch"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipFuncSetAttribute((const void *)spec_mean_partial_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds_bytes));
    hipLaunchKernelGGL(spec_mean_partial_kernel, dim3((unsigned)n_trials, (unsigned)groups, (unsigned)zs), dim3(SPEC_THREADS), g.lds_bytes, s,
                       d_x, ld, C, d_desc, v, g, d_partial);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(spec_mean_finish_kernel, dim3((unsigned)((cols + SPEC_THREADS - 1) / SPEC_THREADS)), dim3(SPEC_THREADS), 0, s,
                       d_partial, n_trials, (int)cols, (double)total_frames, d_out);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
