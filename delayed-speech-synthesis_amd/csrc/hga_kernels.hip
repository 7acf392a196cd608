// csrc/hga_kernels.hip -- high-gamma feature extraction on gfx950 (float64, bit-exact operation order).
//
// Replaces, for many streams at once:
//   scipy.signal.sosfilt x2 with carried state      local/units.py:151-152
//   WarmStartFrameBuffer.insert                     extensions/hga/hga_optimized.pyx:96-131
//   compute_log_power_features                      extensions/hga/hga_optimized.pyx:27-47
//
// ONE launch per call (hga_fused_kernel): the IIR cascades with their sections spread over the 16 lanes of a DPP row (a
// column advances one sample per step instead of one per 16 dependent biquads); the filtered samples of a tile go into an
// LDS ring instead of HBM, every window that has become complete is summed from the ring (a 50-term sequential sum per
// (window, channel) lane, exactly array_sum_and_power's order), and the last `overlap` rows are left in the row buffer
// for the next call.  Only the input, the W x C frames and 40 rows per column touch HBM: at 1024 streams x 1.04 s that
// removes the 545 MB write + read of the filtered rows which the three-launch form (hga_filter_kernel +
// hga_window_kernel + hga_overlap_kernel, kept as the fallback for window shapes whose ring would not fit LDS) needed.
// (A one-launch form with the front end inside helper waves, hga_stream_kernel, was built in round 3, was exact and 1.4-2x
// slower -- profiles/r3_hga_experiment.md -- and left the tree in round 4.)
// Built with -ffp-contract=off: every product and sum rounds separately, as in scipy's C loop and in
// the reference's Cython kernel, which is what makes the mean power bit-identical.
#include <stdlib.h>

#include "dss_common.h"

struct HgaSos { double k[2][8][6]; };

__device__ __forceinline__ int hga_win_start(int win, float ws, int sr)
{
    // pyx:43  int(round((win * window_shift) * sr)) -- float32 products, C round()
    return (int)round((double)((win * ws) * sr));
}
__device__ __forceinline__ int hga_win_stop(int start, float wl, int sr)
{
    // pyx:44  int(round(start_eeg + window_length * sr))
    return (int)round((double)(start + wl * sr));
}

// pyx:45-46 and local/common.py:367-376: a window's mean power over its rows, + 0.01, the log, ZScoreNormalization of channel c
__device__ __forceinline__ double hga_finish(double sum, int rows, int apply_log, const double *__restrict__ zs_mean,
                                             const double *__restrict__ zs_std, int c)
{
    const double pw = sum / (double)rows + 0.01;
    double o = apply_log ? log(pw) : pw;
    if (zs_mean) o = (o - zs_mean[c]) / zs_std[c];
    return o;
}

// ---- stage 1: the two IIR cascades, pipelined over their sections --------------------------------------------
// The 2*nsec (<= 16) second-order sections of one (stream, channel) column occupy the 16 lanes of one DPP row: at
// step k lane r filters sample k - r, taking its input from lane r-1's output of the previous step (row_shr:1), so
// the column advances one sample per step instead of one per 16 biquads.  Each section's arithmetic is exactly
// scipy's sosfilt inner loop (one product, one sum at a time).  A 256-thread block handles 16 consecutive columns,
// whose input samples are staged through LDS in tiles of HGA_TT rows with 128-byte row segments (xs, one row per step);
// lane 2*nsec-1 leaves the filtered sample of step k, sample k - (2*nsec-1), in ys.  Thread tid is section lane tid & 15
// of column tid >> 4 while it filters, and moves column tid & 15 whenever the block copies rows (16 * 8 bytes side by side).
#define HGA_TT 64
static_assert(HGA_TT == DSS_HGA_TT, "the ring of dss_hga_ring (dss_common.h) is sized for this tile");

// a thread as one lane of the section pipeline: where it sits, the section it holds and that section's state
struct HgaLane {
    int r, pib;                // section lane in the DPP row, column in the block
    int nsec2, f, q;           // sections of both cascades; this lane's cascade and section within it (0, 0 without one)
    bool has_sec, is_last;
    double b0, b1, b2, a1, a2;
    double z0, z1, y;
};

// before the kernel's first barrier: the lane's place, and the section coefficients by lane into coef (a kernel argument
// cannot be indexed per lane).  The kernel loads z0 / z1 from wherever its state lives.
__device__ __forceinline__ HgaLane hga_lane_setup(const HgaSos &sos, int nsec, double (*coef)[5])
{
    HgaLane l;
    const int tid = threadIdx.x;
    l.r = tid & 15;
    l.pib = tid >> 4;
    l.nsec2 = 2 * nsec;
    l.has_sec = l.r < l.nsec2;
    l.is_last = l.r == l.nsec2 - 1;
    l.f = l.has_sec ? l.r / nsec : 0;
    l.q = l.has_sec ? l.r - l.f * nsec : 0;
    if (tid < 16) {
        const int ff = tid < l.nsec2 ? tid / nsec : 0, qq = tid < l.nsec2 ? tid - ff * nsec : 0;
        coef[tid][0] = sos.k[ff][qq][0]; coef[tid][1] = sos.k[ff][qq][1]; coef[tid][2] = sos.k[ff][qq][2];
        coef[tid][3] = sos.k[ff][qq][4]; coef[tid][4] = sos.k[ff][qq][5];
    }
    l.y = 0.0;
    return l;
}
// behind that barrier
__device__ __forceinline__ void hga_lane_coef(HgaLane &l, const double (*coef)[5])
{
    l.b0 = coef[l.r][0]; l.b1 = coef[l.r][1]; l.b2 = coef[l.r][2]; l.a1 = coef[l.r][3]; l.a2 = coef[l.r][4];
}

// lanes 1..15 of every row receive their left neighbour's `y`; lane 0 (no neighbour) keeps `x`: the column's input
__device__ __forceinline__ double hga_shift_in(double x, double y)
{
    const unsigned long long ux = __builtin_bit_cast(unsigned long long, x), uy = __builtin_bit_cast(unsigned long long, y);
    const int lo = __builtin_amdgcn_update_dpp((int)(unsigned)ux, (int)(unsigned)uy, 0x111, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp((int)(unsigned)(ux >> 32), (int)(unsigned)(uy >> 32), 0x111, 0xf, 0xf, false);
    return __builtin_bit_cast(double, ((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}

// one step of one section: scipy _sosfilt's inner statement order
__device__ __forceinline__ void hga_biquad(HgaLane &l, double in)
{
    l.y = l.b0 * in + l.z0;                        // x_c = b0*x_n + zi0
    l.z0 = l.b1 * in - l.a1 * l.y + l.z1;          // zi0 = b1*x_n - a1*x_c + zi1
    l.z1 = l.b2 * in - l.a2 * l.y;                 // zi1 = b2*x_n - a2*x_c
}

// a step on which some lanes have no sample yet (pipeline filling) or no more (draining): predicated
__device__ __forceinline__ void hga_edge_step(HgaLane &l, const double (*xs)[16], double (*ys)[16], int k, int base, int n)
{
    const double in = hga_shift_in(xs[k - base][l.pib], l.y);
    const int t = k - l.r;
    if (l.has_sec && t >= 0 && t < n) {
        hga_biquad(l, in);
        if (l.is_last) ys[k - base][l.pib] = l.y;
    }
}

// steps base .. kend - 1 of a column of n samples, over the tile staged in xs
__device__ __forceinline__ void hga_tile_steps(HgaLane &l, const double (*xs)[16], double (*ys)[16], int base, int kend, int n)
{
    int k = base;
    for (; k < kend && (k < l.nsec2 - 1 || k >= n); ++k) hga_edge_step(l, xs, ys, k, base, n);
    // steady state: every section has a sample
    const int ksteady = min(kend, n);
    {
        const double *xp = &xs[k - base][l.pib];
        double xcur = *xp;
        // four steps per trip with constant LDS offsets (a DPP move is convergent: the compiler will not unroll a loop of
        // unknown length around it): per step 9 fp64 operations, 2 DPP moves, one LDS read, one LDS write.  The next
        // step's input is read a step ahead: its LDS latency hides under this step.
        double *const yl = &ys[k - base][l.pib];
        int kk = 0;
        for (; k + 4 <= ksteady; k += 4, kk += 4) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double xnext = xp[16 * (kk + u + 1)];
                hga_biquad(l, hga_shift_in(xcur, l.y));
                if (l.is_last) yl[16 * (kk + u)] = l.y;
                xcur = xnext;
            }
        }
        for (; k < ksteady; ++k, ++kk) {
            const double xnext = xp[16 * (kk + 1)];
            hga_biquad(l, hga_shift_in(xcur, l.y));
            if (l.is_last) yl[16 * kk] = l.y;
            xcur = xnext;
        }
    }
    for (; k < kend; ++k) hga_edge_step(l, xs, ys, k, base, n);      // draining steps at the end of the last tile(s)
}

__global__ void __launch_bounds__(256)
hga_filter_kernel(const double *__restrict__ data, double *__restrict__ zi, double *__restrict__ rowbuf,
                  HgaSos sos, int S, int C, int n, int nsec, int row0, int cap_rows, int zero_rows)
{
    __shared__ double xs[HGA_TT + 1][16];      // inputs of the tile's steps, one row segment of 16 columns per step (+1: read ahead)
    __shared__ double ys[HGA_TT][16];          // outputs produced at the tile's steps (sample k - (2*nsec-1) at step k)
    __shared__ double coef[16][5];
    const int tid = threadIdx.x;
    const long total = (long)S * C;
    const long pair0 = (long)blockIdx.x * 16;
    HgaLane l = hga_lane_setup(sos, nsec, coef);
    long pair = pair0 + l.pib;
    const bool valid = pair < total;
    if (!valid) pair = total - 1;
    const int s = (int)(pair / C), c = (int)(pair - (long)s * C);
    double *zp = zi + (size_t)s * 2 * 8 * 2 * C + c;
    l.z0 = zp[((l.f * 8 + l.q) * 2 + 0) * (size_t)C];
    l.z1 = zp[((l.f * 8 + l.q) * 2 + 1) * (size_t)C];
    // CASE 2 of the frame buffer (first chunk shorter than a frame): left zero padding, pyx:116
    if (valid) {
        double *col = rowbuf + (size_t)s * cap_rows * C + c;
        for (int k = l.r; k < zero_rows; k += 16) col[(size_t)k * C] = 0.0;
    }
    __syncthreads();
    hga_lane_coef(l, coef);
    const int steps = n + l.nsec2 - 1;
    for (int base = 0; base < steps; base += HGA_TT) {
        __syncthreads();                                   // previous tile fully consumed and written out
        for (int idx = tid; idx < HGA_TT * 16; idx += 256) {
            const int tt = idx >> 4, p = idx & 15;
            const long pp = pair0 + p;
            const int t = base + tt;
            double v = 0.0;
            if (t < n && pp < total) {
                const int sp = (int)(pp / C), cp = (int)(pp - (long)sp * C);
                v = data[((size_t)sp * n + t) * C + cp];
            }
            xs[tt][p] = v;
        }
        __syncthreads();
        const int kend = min(base + HGA_TT, steps);
        hga_tile_steps(l, xs, ys, base, kend, n);
        __syncthreads();
        // the tile's finished samples go out as 128-byte row segments
        for (int idx = tid; idx < HGA_TT * 16; idx += 256) {
            const int tt = idx >> 4, p = idx & 15;
            const long pp = pair0 + p;
            const int t = base + tt - (l.nsec2 - 1);
            if (base + tt < kend && t >= 0 && t < n && pp < total) {
                const int sp = (int)(pp / C), cp = (int)(pp - (long)sp * C);
                rowbuf[((size_t)sp * cap_rows + row0 + t) * C + cp] = ys[tt][p];
            }
        }
    }
    if (valid && l.has_sec) {
        zp[((l.f * 8 + l.q) * 2 + 0) * (size_t)C] = l.z0;
        zp[((l.f * 8 + l.q) * 2 + 1) * (size_t)C] = l.z1;
    }
}

// ---- one-launch forms: filter tile -> LDS ring -> completed windows ---------------------------------------------------
// Same block shape and the same per-step code as hga_filter_kernel (16 columns x 16 section lanes).  `ring` holds the last
// R rows of the block's 16 columns (overlap / zero rows first, then the new samples at row0 + t), row i at position i mod R;
// R >= frame_length + window shift + TT + 2 so that no row a pending window still needs is overwritten by the next tile.
// Round 3: R carries no power-of-two padding (18 KB of static LDS + 16 KB of ring instead of 37 KB).  (A 32-step-tile
// instantiation -- 22 KB, 7 blocks per CU instead of 5 -- was no faster at 1024 streams and slower on small calls,
// profiles/r3_hga_tile_ab_timing.txt, and is gone.)
#define HGF_WTAB 128

// the frames a block emits: W windows over its columns, the window rule of pyx:43-44 and the finish
struct HgaFrames {
    int W, sr;
    float wl, ws;
    int apply_log;
    const double *zs_mean, *zs_std;
};

// first and one-past-last row of the first HGF_WTAB windows (the float32 / round() arithmetic once per block instead of
// once per tile); a window past the table takes its rows from that arithmetic directly
__device__ __forceinline__ void hga_window_table(int (*wtab)[HGF_WTAB], const HgaFrames &fr)
{
    for (int w = threadIdx.x; w < fr.W && w < HGF_WTAB; w += 256) {
        const int st = hga_win_start(w, fr.ws, fr.sr);
        wtab[0][w] = st;
        wtab[1][w] = hga_win_stop(st, fr.wl, fr.sr);
    }
}
__device__ __forceinline__ void hga_window_range(const int (*wtab)[HGF_WTAB], const HgaFrames &fr, int w, int &start, int &stop)
{
    if (w < HGF_WTAB) {            // one branch for both: a caller that wants the stop alone then reads one entry, not two in turn
        start = wtab[0][w];
        stop = wtab[1][w];
    } else {
        start = hga_win_start(w, fr.ws, fr.sr);
        stop = hga_win_stop(start, fr.wl, fr.sr);
    }
}

// Input tiles: thread (tt0, p) owns column p of rows tt0, tt0 + 16, ... of every tile; lcol is its column's sample 0 (null: a
// column past the edge, zeros).  Samples base + tt0 + 16 j of a column of n, C doubles apart, into registers.
__device__ __forceinline__ void hga_tile_fetch(double (&pre)[HGA_TT / 16], const double *__restrict__ lcol, int base, int n, int C)
{
    const int ltt = threadIdx.x >> 4;
#pragma unroll
    for (int j = 0; j < HGA_TT / 16; ++j) {
        const int t = base + ltt + 16 * j;
        pre[j] = (lcol && t < n) ? lcol[(size_t)t * C] : 0.0;
    }
}

// the tile's finished samples join the ring at their row: the output of step base + tt at position tile_pos + tt (mod R)
__device__ __forceinline__ void hga_ring_join(double *ring, int R, int tile_pos, const double (*ys)[16], int base, int kend,
                                              int nsec2, int n)
{
    for (int idx = threadIdx.x; idx < HGA_TT * 16; idx += 256) {
        const int tt = idx >> 4, p = idx & 15;
        const int t = base + tt - (nsec2 - 1);
        int pos = tile_pos + tt;
        if (pos >= R) pos -= R;
        if (base + tt < kend && t >= 0 && t < n) ring[pos * 16 + p] = ys[tt][p];
    }
}

// every window from w_next on whose rows are all among the first rows_done: lane = (window, column), a sequential sum over
// its rows (pyx:9-22, 42-46); then w_next moves past them (block-uniform).  ocol is the lane's output column, frame w at
// ocol[w * C] (null: a column past the edge), oc its channel for the z-score.
__device__ __forceinline__ void hga_ring_windows(const double *ring, int R, const int (*wtab)[HGF_WTAB], const HgaFrames &fr,
                                                 int &w_next, int rows_done, double *__restrict__ ocol, int C, int oc)
{
    const int p = threadIdx.x & 15, wi = threadIdx.x >> 4;
    int start, stop;
    for (int w = w_next + wi; w < fr.W; w += 16) {
        hga_window_range(wtab, fr, w, start, stop);
        if (stop > rows_done) break;
        double sum = 0.0;
        // the window's rows sit at positions start mod R ... (wrapping once at most: stop - start <= R)
        int pos = start % R, left = stop - start;
        while (left > 0) {
            const int run = min(left, R - pos);
            const double *rp = ring + pos * 16 + p;
            int i = 0;
            for (; i + 8 <= run; i += 8) {             // eight ring reads in flight, then their terms in row order
                double v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = rp[(i + u) * 16];
#pragma unroll
                for (int u = 0; u < 8; ++u) sum += v[u] * v[u];
            }
            for (; i < run; ++i) {
                const double v = rp[i * 16];
                sum += v * v;
            }
            left -= run;
            pos = 0;
        }
        if (ocol) ocol[(size_t)w * C] = hga_finish(sum, stop - start, fr.apply_log, fr.zs_mean, fr.zs_std, oc);
    }
    for (; w_next < fr.W; ++w_next) {
        hga_window_range(wtab, fr, w_next, start, stop);
        if (stop > rows_done) break;
    }
}

// All tiles of a block whose ring already holds rows [0, row0): the n samples of each column are filtered and join the ring at
// rows row0 .. row0 + n - 1, and every window goes out once its rows are there.  The next tile's samples are fetched into
// registers before the current tile's steps run and go to LDS after them: the HBM latency hides under the filter
// arithmetic instead of standing between two barriers.  lcol: hga_tile_fetch; ocol, oc: hga_ring_windows.
__device__ __forceinline__ void hga_ring_tiles(HgaLane &l, double (*xs)[16], double (*ys)[16], const int (*wtab)[HGF_WTAB],
                                               double *ring, int R, const HgaFrames &fr, const double *__restrict__ lcol, int n,
                                               int row0, double *__restrict__ ocol, int C, int oc)
{
    const int lp = threadIdx.x & 15, ltt = threadIdx.x >> 4;
    const int steps = n + l.nsec2 - 1;
    int w_next = 0;                                        // first window not yet written (block-uniform)
    double pre[HGA_TT / 16];
    hga_tile_fetch(pre, lcol, 0, n, C);
    // ring position of row (row0 + t) for the first output of the current tile, kept modulo R (block-uniform)
    int tile_pos = (row0 + R * 16 - (l.nsec2 - 1)) % R;    // row0 + t for t = 0 - (nsec2 - 1): the row "before" the first output
    for (int base = 0; base < steps; base += HGA_TT) {
        __syncthreads();                                   // previous tile fully consumed
#pragma unroll
        for (int j = 0; j < HGA_TT / 16; ++j) xs[ltt + 16 * j][lp] = pre[j];
        if (base + HGA_TT < steps) hga_tile_fetch(pre, lcol, base + HGA_TT, n, C);
        __syncthreads();
        const int kend = min(base + HGA_TT, steps);
        hga_tile_steps(l, xs, ys, base, kend, n);
        __syncthreads();
        hga_ring_join(ring, R, tile_pos, ys, base, kend, l.nsec2, n);
        tile_pos += HGA_TT;
        if (tile_pos >= R) tile_pos -= R;
        __syncthreads();
        int t_done = kend - (l.nsec2 - 1);
        t_done = t_done < 0 ? 0 : (t_done > n ? n : t_done);
        hga_ring_windows(ring, R, wtab, fr, w_next, row0 + t_done, ocol, C, oc);
    }
}

// ---- streaming form: every stream advances by one chunk of n samples; the last `overlap` rows stay for the next call ----
__global__ void __launch_bounds__(256, 4)
hga_fused_kernel(const double *__restrict__ data, double *__restrict__ zi, double *__restrict__ rowbuf, double *__restrict__ out,
                 HgaSos sos, int S, int C, int n, int nsec, int row0, int cap_rows, int zero_rows, int rows, int W, int overlap,
                 int sr, float wl, float ws, int apply_log, int R, const double *__restrict__ zs_mean,
                 const double *__restrict__ zs_std)
{
    __shared__ double xs[HGA_TT + 1][16];
    __shared__ double ys[HGA_TT][16];
    __shared__ double coef[16][5];
    __shared__ int wtab[2][HGF_WTAB];
    extern __shared__ __attribute__((aligned(16))) double ring[];         // [R][16]
    const int tid = threadIdx.x;
    const long total = (long)S * C;
    const long pair0 = (long)blockIdx.x * 16;
    const HgaFrames fr = {W, sr, wl, ws, apply_log, zs_mean, zs_std};
    HgaLane l = hga_lane_setup(sos, nsec, coef);
    // the column this thread filters, and its state
    long pair = pair0 + l.pib;
    const bool valid = pair < total;
    if (!valid) pair = total - 1;
    const int s = (int)(pair / C), c = (int)(pair - (long)s * C);
    double *zp = zi + (size_t)s * 2 * 8 * 2 * C + c;
    l.z0 = zp[((l.f * 8 + l.q) * 2 + 0) * (size_t)C];
    l.z1 = zp[((l.f * 8 + l.q) * 2 + 1) * (size_t)C];
    // the column this thread moves: input, overlap rows and frames (a block's 16 columns may span two streams)
    const int p = tid & 15;
    const long pp = pair0 + p;
    const bool pvalid = pp < total;
    const int sp = pvalid ? (int)(pp / C) : 0, cp = pvalid ? (int)(pp - (long)sp * C) : 0;
    double *const rcol = rowbuf + (size_t)sp * cap_rows * C + cp;
    // (formed here and selected against null below: formed inside the selection, the row stride C ends up in vector registers)
    const double *const lcol = data + (size_t)sp * n * C + cp;
    double *const ocol = out + (size_t)sp * W * C + cp;
    hga_window_table(wtab, fr);
    // rows [0, row0) of the ring: zeros (CASE 2, pyx:116) or the overlap the previous call left (CASE 3, pyx:123-131)
    for (int rr = tid >> 4; rr < row0; rr += 16)
        ring[(rr % R) * 16 + p] = (rr >= zero_rows && pvalid) ? rcol[(size_t)rr * C] : 0.0;
    __syncthreads();
    hga_lane_coef(l, coef);
    hga_ring_tiles(l, xs, ys, wtab, ring, R, fr, pvalid ? lcol : nullptr, n, row0, pvalid ? ocol : nullptr, C, cp);
    __syncthreads();
    // the last `overlap` rows become rows 0..overlap-1 of the next call (WarmStartFrameBuffer.remainder_data)
    if (pvalid)
        for (int kk = tid >> 4; kk < overlap; kk += 16) rcol[(size_t)kk * C] = ring[((rows - overlap + kk) % R) * 16 + p];
    if (valid && l.has_sec) {
        zp[((l.f * 8 + l.q) * 2 + 0) * (size_t)C] = l.z0;
        zp[((l.f * 8 + l.q) * 2 + 1) * (size_t)C] = l.z1;
    }
}

// ---- trial form: one launch for a list of trials of unequal length ----------------------------------------------------
// hga_fused_kernel advances all streams by one n; a session's trials (baseline_offline.py:45-60, prepare_corpus.py:42-52) are
// windows of unequal length into ONE recording, each fed to a FRESH HighGammaExtractor as a single chunk.  Here a block takes
// (trial, 16-column group): its n, W, zero rows, first input row and first output frame come from a descriptor table, the
// filter state starts at the unit-step state of sosfilt_zi (units.py:128-132) and nothing is written back -- no per-stream
// zi / rowbuf is touched.  Everything between is hga_ring_tiles, as in hga_fused_kernel.
// `data` is the recording (or its front-end output), (rows, C) row-major; trial i reads rows in_row .. in_row + n - 1 and
// writes frames out_row .. out_row + W - 1 of the concatenated (sum W, C) output.  Every range is checked on the host.
__global__ void __launch_bounds__(256, 4)
hga_trials_kernel(const double *__restrict__ data, const DssHgaTrialDesc *__restrict__ desc, double *__restrict__ out,
                  const double *__restrict__ zi_hg, const double *__restrict__ zi_fh, HgaSos sos, int C, int cgroups, int nsec,
                  int sr, float wl, float ws, int apply_log, int R, const double *__restrict__ zs_mean,
                  const double *__restrict__ zs_std)
{
    __shared__ double xs[HGA_TT + 1][16];
    __shared__ double ys[HGA_TT][16];
    __shared__ double coef[16][5];
    __shared__ int wtab[2][HGF_WTAB];
    extern __shared__ __attribute__((aligned(16))) double ring[];         // [R][16]
    const int tid = threadIdx.x;
    const int trial = blockIdx.x / cgroups, cg = blockIdx.x - trial * cgroups;
    const DssHgaTrialDesc d = desc[trial];
    const int row0 = d.zero_rows;                         // a fresh frame buffer: CASE 1 (row0 = 0) or CASE 2 (left zero pad)
    const HgaFrames fr = {d.W, sr, wl, ws, apply_log, zs_mean, zs_std};
    HgaLane l = hga_lane_setup(sos, nsec, coef);
    // units.py:128-132: every column starts at sosfilt_zi(sos), not scaled by the first sample
    const double *z_src = l.f ? zi_fh : zi_hg;
    l.z0 = l.has_sec ? z_src[l.q * 2 + 0] : 0.0;
    l.z1 = l.has_sec ? z_src[l.q * 2 + 1] : 0.0;
    hga_window_table(wtab, fr);
    for (int idx = tid; idx < row0 * 16; idx += 256) ring[idx] = 0.0;     // CASE 2, pyx:116 (row0 <= frame length <= R)
    __syncthreads();
    hga_lane_coef(l, coef);
    const int c = cg * 16 + (tid & 15);                   // the column this thread moves: input and frames
    const bool cvalid = c < C;
    const double *const lcol = data + (size_t)d.in_row * C + (cvalid ? c : 0);
    double *const ocol = out + (size_t)d.out_row * C + (cvalid ? c : 0);
    hga_ring_tiles(l, xs, ys, wtab, ring, R, fr, cvalid ? lcol : nullptr, d.n, row0, cvalid ? ocol : nullptr, C, c);
}

int dss_launch_hga_trials(const DssHgaDev &h, const double *d_data, const DssHgaTrialDesc *d_desc, int n_trials, const double *d_zi_hg,
                          const double *d_zi_fh, double *d_out, int apply_log, int with_zscore, hipStream_t st)
{
    if (n_trials <= 0) return DSS_OK;
    HgaSos sos;
    memcpy(&sos, h.sos, sizeof(sos));
    const DssHgaRing ring = dss_hga_ring(h.frame_length, h.overlap);
    if (!ring.fused) {
        dss_set_error("HGA trials: a frame of %d rows does not fit the kernel's ring", h.frame_length);
        return DSS_EINVAL;
    }
    const int cgroups = (h.C + 15) / 16;
    const long blocks = (long)n_trials * cgroups;
    if (blocks > 0x7fffffffL) { dss_set_error("HGA trials: too many blocks"); return DSS_EINVAL; }
    hipLaunchKernelGGL(hga_trials_kernel, dim3((unsigned)blocks), dim3(256), ring.bytes, st, d_data, d_desc, d_out, d_zi_hg, d_zi_fh,
                       sos, h.C, cgroups, h.nsec, h.fs, h.wl, h.ws, apply_log, ring.rows, with_zscore ? h.zs_mean : nullptr,
                       with_zscore ? h.zs_std : nullptr);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// BadChannelCorrection.__call__ (local/common.py:286-291) on log-power frames: lane = (frame, corrected channel).  The mean
// of the neighbour columns is numpy's np.mean(data[:, neighbours], axis=1): for two or more frames the fancy-indexed copy is
// Fortran-ordered and numpy adds it one column at a time -- the SEQUENTIAL sum in list order, for 8 neighbours too; a SINGLE
// frame (a trial that emits one: the reference patches trial by trial) is a contiguous row, which numpy sums with its
// pairwise kernel: eight running sums over blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder in
// order (fewer than 8 elements: sequential).  One division follows.  Neighbours are never corrected channels themselves
// (checked on the host), so the patch runs in place.  rows: the frames to patch (NULL: all N, sequential rule).
__device__ __forceinline__ double hga_row_mean(const double *fr, const int *__restrict__ cols, int a, int b, bool single)
{
    const int n = b - a;
    double sum;
    if (!single || n < 8) {
        sum = fr[cols[a]];
        for (int j = a + 1; j < b; ++j) sum += fr[cols[j]];
    } else {
        double r[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = fr[cols[a + u]];
        int i = 8;
        for (; i < n - (n % 8); i += 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) r[u] += fr[cols[a + i + u]];
        }
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) sum += fr[cols[a + i]];
    }
    return sum / (double)n;
}

__global__ void __launch_bounds__(256)
hga_patch_kernel(double *__restrict__ frames, long N, int C, int n_patches, const int *__restrict__ dst_col,
                 const int *__restrict__ nb_cols, const int *__restrict__ nb_off, const long long *__restrict__ rows)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= N * n_patches) return;
    const long i = gid / n_patches;
    const int k = (int)(gid - i * n_patches);
    double *fr = frames + (size_t)(rows ? rows[i] : i) * C;
    fr[dst_col[k]] = hga_row_mean(fr, nb_cols, nb_off[k], nb_off[k + 1], rows != nullptr);
}

// ZScoreNormalization behind the patch (the trial kernel's own epilogue cannot run before it)
__global__ void __launch_bounds__(256)
hga_zscore_kernel(double *__restrict__ frames, long total, int C, const double *__restrict__ zs_mean, const double *__restrict__ zs_std)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid % C);
    frames[gid] = (frames[gid] - zs_mean[c]) / zs_std[c];
}

int dss_launch_hga_patch(double *d_frames, long N, int C, int n_patches, const int *dst_col, const int *nb_cols, const int *nb_off,
                         const long long *d_single_rows, long n_single, const double *zs_mean, const double *zs_std, hipStream_t st)
{
    if (N <= 0) return DSS_OK;
    if (n_patches > 0) {
        const long lanes = N * n_patches;
        hipLaunchKernelGGL(hga_patch_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, d_frames, N, C, n_patches,
                           dst_col, nb_cols, nb_off, nullptr);
        DSS_HIP_CHECK(hipGetLastError());
        if (n_single > 0) {         // the frames of single-frame trials again, by numpy's rule for one contiguous row
            const long l1 = n_single * n_patches;
            hipLaunchKernelGGL(hga_patch_kernel, dim3((unsigned)((l1 + 255) / 256)), dim3(256), 0, st, d_frames, n_single, C,
                               n_patches, dst_col, nb_cols, nb_off, d_single_rows);
            DSS_HIP_CHECK(hipGetLastError());
        }
    }
    if (zs_mean) {
        const long total = N * C;
        hipLaunchKernelGGL(hga_zscore_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d_frames, total, C, zs_mean,
                           zs_std);
        DSS_HIP_CHECK(hipGetLastError());
    }
    return DSS_OK;
}

// np.mean / np.std over axis 0 of a C-contiguous (N, C) array: numpy adds whole rows in order, so column c's sum is
// row 0, += row 1, ... (no pairwise tree on this axis); std uses that mean, d = x - m, d * d summed in the same order, / N,
// sqrt.  One lane per column walks the rows -- the order is the contract, the sum is NOT split.  Eight loads in flight.
__global__ void __launch_bounds__(64)
hga_colstats_kernel(const double *__restrict__ frames, long N, int C, double *__restrict__ out)
{
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const double *col = frames + c;
    double sum = col[0];
    long i = 1;
    for (; i + 8 <= N; i += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(size_t)(i + u) * C];
#pragma unroll
        for (int u = 0; u < 8; ++u) sum += v[u];
    }
    for (; i < N; ++i) sum += col[(size_t)i * C];
    const double m = sum / (double)N;
    double d0 = col[0] - m;
    double sq = d0 * d0;
    i = 1;
    for (; i + 8 <= N; i += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = col[(size_t)(i + u) * C];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const double dd = v[u] - m; sq += dd * dd; }
    }
    for (; i < N; ++i) { const double dd = col[(size_t)i * C] - m; sq += dd * dd; }
    out[c] = m;
    out[C + c] = sqrt(sq / (double)N);
}

// ONE column (C == 1) is one contiguous run, and numpy sums a contiguous run with its pairwise kernel, not row by row: below 8
// elements in order; up to 128 eight running sums over blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder
// in order; a longer run is halved (the left half a multiple of 8) and the halves' sums are added.  Element i is a[i], or with
// sq (a[i] - m) * (a[i] - m).  The halving is walked with an explicit stack of (offset, length, stage, left sum): a run of n
// elements nests ceil(log2(n / 128)) deep, 64 levels hold any long.
__device__ double hga_pairwise_run(const double *__restrict__ a, long n, double m, bool sq)
{
#define HGA_PW_AT(I) (sq ? (a[I] - m) * (a[I] - m) : a[I])
    if (n < 8) {
        double r = HGA_PW_AT(0);
        for (long i = 1; i < n; ++i) r += HGA_PW_AT(i);
        return r;
    }
    double r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = HGA_PW_AT(u);
    long i = 8;
    for (; i < n - (n % 8); i += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] += HGA_PW_AT(i + u);
    }
    double sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) sum += HGA_PW_AT(i);
    return sum;
#undef HGA_PW_AT
}

__device__ double hga_pairwise_sum(const double *__restrict__ a, long n, double m, bool sq)
{
    long off[64], len[64];
    double left[64];
    int stage[64];
    int sp = 0;
    off[0] = 0; len[0] = n; stage[0] = 0;
    double ret = 0.0;
    while (sp >= 0) {
        if (len[sp] <= 128) { ret = hga_pairwise_run(a + off[sp], len[sp], m, sq); --sp; continue; }
        long n2 = len[sp] / 2;
        n2 -= n2 % 8;
        if (stage[sp] == 0) {                              // the left half first
            stage[sp] = 1;
            if (sp + 1 >= 64) return ret;                  // unreachable for a long n; never past the stack
            off[sp + 1] = off[sp]; len[sp + 1] = n2; stage[sp + 1] = 0;
            ++sp;
        } else if (stage[sp] == 1) {                       // then the right half
            left[sp] = ret;
            stage[sp] = 2;
            off[sp + 1] = off[sp] + n2; len[sp + 1] = len[sp] - n2; stage[sp + 1] = 0;
            ++sp;
        } else {
            ret = left[sp] + ret;
            --sp;
        }
    }
    return ret;
}

__global__ void __launch_bounds__(64)
hga_colstats_one_kernel(const double *__restrict__ frames, long N, double *__restrict__ out)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const double m = hga_pairwise_sum(frames, N, 0.0, false) / (double)N;
    out[0] = m;
    out[1] = sqrt(hga_pairwise_sum(frames, N, m, true) / (double)N);
}

int dss_launch_hga_colstats(const double *d_frames, long N, int C, double *d_out, hipStream_t st)
{
    if (C == 1) {
        hipLaunchKernelGGL(hga_colstats_one_kernel, dim3(1), dim3(64), 0, st, d_frames, N, d_out);
        DSS_HIP_CHECK(hipGetLastError());
        return DSS_OK;
    }
    hipLaunchKernelGGL(hga_colstats_kernel, dim3((C + 63) / 64), dim3(64), 0, st, d_frames, N, C, d_out);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- stage 2: windowed mean power ---------------------------------------------------------------------------------
// A 256-thread block takes 8 consecutive windows x 32 consecutive channels of one stream: the rows those windows cover
// (50 + 7*10 for the reference's 50 ms / 10 ms at 1 kHz) are staged once through LDS in 256-byte row segments instead
// of being fetched by each of the five windows that overlap them; lane (window, channel) then runs its window's
// sequential sum over rows exactly as array_sum_and_power does (pyx:9-22).
#define HGA_WB 8
#define HGA_WC 32
#define HGA_WROWS 160            // LDS rows per block; a block whose windows span more falls back to global reads

__global__ void __launch_bounds__(256)
hga_window_kernel(const double *__restrict__ rowbuf, double *__restrict__ out, int S, int C, int W, int cap_rows, int sr,
                  float wl, float ws, int apply_log, const double *__restrict__ zs_mean, const double *__restrict__ zs_std)
{
    __shared__ double tile[HGA_WROWS][HGA_WC];
    const int tid = threadIdx.x, cl = tid & (HGA_WC - 1), wi = tid / HGA_WC;
    const int cgroups = (C + HGA_WC - 1) / HGA_WC, wchunks = (W + HGA_WB - 1) / HGA_WB;
    int bid = blockIdx.x;
    const int wc = bid % wchunks; bid /= wchunks;
    const int cg = bid % cgroups;
    const int s = bid / cgroups;
    const int w0 = wc * HGA_WB, wlast = min(w0 + HGA_WB, W) - 1;
    const int row_lo = hga_win_start(w0, ws, sr);
    const int row_hi = hga_win_stop(hga_win_start(wlast, ws, sr), wl, sr);
    const int nrows = row_hi - row_lo;
    const bool staged = nrows <= HGA_WROWS;
    const double *base = rowbuf + (size_t)s * cap_rows * C;
    const int c0 = cg * HGA_WC;
    if (staged) {
        for (int idx = tid; idx < nrows * HGA_WC; idx += 256) {
            const int rr = idx / HGA_WC, cc = idx - rr * HGA_WC;
            tile[rr][cc] = (c0 + cc < C) ? base[(size_t)(row_lo + rr) * C + c0 + cc] : 0.0;
        }
    }
    __syncthreads();
    const int win = w0 + wi, c = c0 + cl;
    if (win >= W || c >= C) return;
    const int start = hga_win_start(win, ws, sr);
    const int stop = hga_win_stop(start, wl, sr);
    double sum = 0.0;
    if (staged) {
        for (int rr = start; rr < stop; ++rr) {
            const double v = tile[rr - row_lo][cl];
            sum += v * v;
        }
    } else {
        for (int rr = start; rr < stop; ++rr) {
            const double v = base[(size_t)rr * C + c];
            sum += v * v;
        }
    }
    out[((size_t)s * W + win) * C + c] = hga_finish(sum, stop - start, apply_log, zs_mean, zs_std, c);
}

// ---- stage 3: keep the last `overlap` rows (ascending copy: a source row is always ahead of its destination) ------
__global__ void __launch_bounds__(256)
hga_overlap_kernel(double *__restrict__ rowbuf, int S, int C, int cap_rows, int rows, int overlap)
{
    const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= (long)S * C) return;
    const int s = (int)(gid / C), c = (int)(gid - (long)s * C);
    double *col = rowbuf + (size_t)s * cap_rows * C + c;
    for (int k = 0; k < overlap; ++k) col[(size_t)k * C] = col[(size_t)(rows - overlap + k) * C];
}

int dss_launch_hga(const DssHgaDev &h, const double *d_data, int n, int row0, int zero_rows, int rows, int W, double *d_out,
                   int apply_log, hipStream_t st)
{
    HgaSos sos;
    memcpy(&sos, h.sos, sizeof(sos));
    const long pairs = (long)h.S * h.C;
    if (h.force_path != 2) {   // fused form when the ring (frame + shift + one tile of rows) fits beside the tiles
        const DssHgaRing ring = dss_hga_ring(h.frame_length, h.overlap);
        if (ring.fused && rows - h.overlap + HGA_TT <= (1 << 30) && h.overlap <= ring.rows && row0 <= ring.rows) {
            hipLaunchKernelGGL(hga_fused_kernel, dim3((unsigned)((pairs + 15) / 16)), dim3(256), ring.bytes, st, d_data, h.zi,
                               h.rows, d_out, sos, h.S, h.C, n, h.nsec, row0, h.cap_rows, zero_rows, rows, W, h.overlap, h.fs, h.wl,
                               h.ws, apply_log, ring.rows, h.zs_mean, h.zs_std);
            DSS_HIP_CHECK(hipGetLastError());
            return DSS_OK;
        }
    }
    hipLaunchKernelGGL(hga_filter_kernel, dim3((unsigned)((pairs + 15) / 16)), dim3(256), 0, st, d_data, h.zi, h.rows, sos,
                       h.S, h.C, n, h.nsec, row0, h.cap_rows, zero_rows);
    DSS_HIP_CHECK(hipGetLastError());
    if (W > 0) {
        const long blocks = (long)h.S * ((h.C + HGA_WC - 1) / HGA_WC) * ((W + HGA_WB - 1) / HGA_WB);
        hipLaunchKernelGGL(hga_window_kernel, dim3((unsigned)blocks), dim3(256), 0, st, h.rows, d_out, h.S, h.C, W, h.cap_rows,
                           h.fs, h.wl, h.ws, apply_log, h.zs_mean, h.zs_std);
        DSS_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(hga_overlap_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, st, h.rows, h.S, h.C,
                       h.cap_rows, rows, h.overlap);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// state <- sosfilt_zi tiled over channels (units.py:128-132); zero the overlap rows (pyx:79-82)
__global__ void hga_reset_kernel(double *zi, double *rowbuf, const double *zi_hg, const double *zi_fh, int S, int C,
                                 int nsec, int cap_rows, int overlap)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= S * C) return;
    const int s = gid / C, c = gid - s * C;
    double *zp = zi + (size_t)s * 2 * 8 * 2 * C + c;
    for (int f = 0; f < 2; ++f)
        for (int q = 0; q < 8; ++q)
            for (int k = 0; k < 2; ++k) {
                const double *src = f ? zi_fh : zi_hg;
                zp[((f * 8 + q) * 2 + k) * (size_t)C] = (q < nsec) ? src[q * 2 + k] : 0.0;
            }
    double *col = rowbuf + (size_t)s * cap_rows * C + c;
    for (int r = 0; r < overlap; ++r) col[(size_t)r * C] = 0.0;
}

int dss_launch_hga_reset(const DssHgaDev &h, const double *d_zi_hg, const double *d_zi_fh, hipStream_t st)
{
    const int total = h.S * h.C;
    hipLaunchKernelGGL(hga_reset_kernel, dim3((total + 255) / 256), dim3(256), 0, st, h.zi, h.rows, d_zi_hg, d_zi_fh, h.S,
                       h.C, h.nsec, h.cap_rows, h.overlap);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// Stateless compute_log_power_features: one lane per (window, channel); 50-term sequential sum.
__global__ void __launch_bounds__(256)
hga_log_power_kernel(const double *__restrict__ data, double *__restrict__ out, int T, int C, int W, int sr, float wl,
                     float ws, int apply_log)
{
    const int gid = blockIdx.x * blockDim.x + threadIdx.x;
    if (gid >= W * C) return;
    const int win = gid / C, c = gid - win * C;
    const int start = hga_win_start(win, ws, sr);
    const int stop = hga_win_stop(start, wl, sr);
    double sum = 0.0;
    for (int r = start; r < stop; ++r) {
        const double q = data[(size_t)r * C + c];
        sum += q * q;
    }
    out[gid] = hga_finish(sum, stop - start, apply_log, nullptr, nullptr, c);
}

int dss_launch_log_power(const double *d_data, int T, int C, int sr, float wl, float ws, int W, double *d_out,
                         int apply_log, hipStream_t st)
{
    const int total = W * C;
    if (total <= 0) return DSS_OK;
    hipLaunchKernelGGL(hga_log_power_kernel, dim3((total + 255) / 256), dim3(256), 0, st, d_data, d_out, T, C, W, sr, wl,
                       ws, apply_log);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}


// Fused front end: column reorder + per-grid common average reference + channel selection.  A block stages FE_ROWS
// consecutive (stream, sample) rows of the raw packet through LDS with coalesced loads (lanes across the c_raw columns;
// the odd row length keeps column walks conflict-free), then one lane per (row, grid) runs the grid mean as the
// SEQUENTIAL sum the reference's numpy expression performs (np.mean over a Fortran-ordered fancy-index copy adds one
// column at a time) followed by one division, and finally lanes across the C output channels subtract and store
// coalesced.  Bit-identical to the numpy chain (local/common.py:16-58,308-345).
#define FE_ROWS 32
__global__ void __launch_bounds__(256)
hga_frontend_kernel(const double *__restrict__ raw, double *__restrict__ pre, int total, int c_raw, int C,
                    const int *__restrict__ src_col, const int *__restrict__ grid_of, int n_grids,
                    const int *__restrict__ comp_cols, const int *__restrict__ comp_off)
{
    extern __shared__ __attribute__((aligned(16))) double fe_tile[];     // [FE_ROWS][c_raw], [FE_ROWS][4] means, [<= 4 * c_raw] member columns
    double *means = fe_tile + (size_t)FE_ROWS * c_raw;
    int *cols = reinterpret_cast<int *>(means + FE_ROWS * 4);            // the grids' member columns, in summation order
    const int tid = threadIdx.x;
    const long row_base = (long)blockIdx.x * FE_ROWS;
    const int nrows = (int)min((long)FE_ROWS, (long)total - row_base);
    const double *src = raw + (size_t)row_base * c_raw;
    // rows are contiguous: fully coalesced; eight loads per thread in flight (a loop of unknown length is not unrolled,
    // and one load per trip would expose the HBM latency sixteen times per tile)
    const int n_el = nrows * c_raw;
    for (int base = 0; base < n_el; base += 8 * 256) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int idx = base + u * 256 + tid; v[u] = idx < n_el ? src[idx] : 0.0; }
#pragma unroll
        for (int u = 0; u < 8; ++u) { const int idx = base + u * 256 + tid; if (idx < n_el) fe_tile[idx] = v[u]; }
    }
    for (int k = tid; k < comp_off[n_grids]; k += 256) cols[k] = comp_cols[k];
    __syncthreads();
    if (tid < nrows * n_grids) {
        const int rr = tid / n_grids, g = tid - rr * n_grids;
        const double *row = fe_tile + (size_t)rr * c_raw;
        const int a = comp_off[g], b2 = comp_off[g + 1];
        double sum = 0.0;
        int k = a;
        for (; k + 8 <= b2; k += 8) {              // eight members' reads in flight, then their terms in list order
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = row[cols[k + u]];
#pragma unroll
            for (int u = 0; u < 8; ++u) sum += v[u];
        }
        for (; k < b2; ++k) sum += row[cols[k]];
        means[rr * 4 + g] = sum / (double)(b2 - a);
    }
    __syncthreads();
    const int n_out = nrows * C;                    // eight independent elements per thread and trip, as for the loads
    for (int base = 0; base < n_out; base += 8 * 256) {
        double o[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + u * 256 + tid;
            o[u] = 0.0;
            if (idx < n_out) {
                const int rr = idx / C, c = idx - rr * C;
                const int g = grid_of[c];
                const double v = fe_tile[(size_t)rr * c_raw + src_col[c]];
                o[u] = g >= 0 ? v - means[rr * 4 + g] : v;
            }
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int idx = base + u * 256 + tid;
            if (idx < n_out) pre[(size_t)row_base * C + idx] = o[u];
        }
    }
}

// Amplifier payloads as they arrive on the wire -- float32, channel-major: [stream][channel][sample] (the body of a BCI2000
// packet behind its 7-byte header, reference local/units.py:78-82 and development_amplifier.py:14-25) -- to the float64
// time-major rows [stream][sample][channel] every other entry point takes: what ZMQConnector.interpret_bytes does on the host
// with reshape + transpose + astype(float64), for all streams at once.  float32 -> float64 is exact, so results do not change.
// One workgroup per stream; the payload goes through LDS so that both the read and the write are linear.
__global__ void __launch_bounds__(256) hga_wire_kernel(const float *__restrict__ payload, double *__restrict__ rows, int C, int n)
{
    extern __shared__ float wtile[];                          // [channel][sample], as it arrived
    const int s = blockIdx.x, total = C * n;
    const float *src = payload + (size_t)s * total;
    for (int k = threadIdx.x; k < total; k += 256) wtile[k] = src[k];
    __syncthreads();
    double *dst = rows + (size_t)s * total;
    for (int k = threadIdx.x; k < total; k += 256) {
        const int t = k / C, c = k - t * C;
        dst[k] = (double)wtile[c * n + t];
    }
}

int dss_launch_hga_wire(const float *d_payload, double *d_rows, int S, int C, int n, hipStream_t s)
{
    const size_t lds = (size_t)C * n * sizeof(float);
    if (lds > 64 * 1024) { dss_set_error("wire packet of %d channels x %d samples exceeds the 64 KB tile", C, n); return DSS_EINVAL; }
    hipLaunchKernelGGL(hga_wire_kernel, dim3(S), dim3(256), lds, s, d_payload, d_rows, C, n);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

int dss_launch_hga_frontend(const double *d_raw, double *d_pre, int S, int n, int c_raw, int C, const int *src_col,
                            const int *grid_of, int n_grids, const int *comp_cols, const int *comp_off, hipStream_t st)
{
    const int total = S * n;
    const size_t lds = ((size_t)FE_ROWS * c_raw + FE_ROWS * 4) * sizeof(double) + (size_t)4 * c_raw * sizeof(int);   // member lists: at most 4 grids of c_raw columns
    if (lds > 64 * 1024 || n_grids > 4) { dss_set_error("front end: %d raw columns / %d grids exceed the tile", c_raw, n_grids); return DSS_EINVAL; }
    hipLaunchKernelGGL(hga_frontend_kernel, dim3((total + FE_ROWS - 1) / FE_ROWS), dim3(256), lds, st, d_raw, d_pre, total, c_raw, C,
                       src_col, grid_of, n_grids, comp_cols, comp_off);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
