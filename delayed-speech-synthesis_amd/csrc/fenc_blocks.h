// csrc/fenc_blocks.h -- the frame arithmetic of the LPC feature encoder, stated once for its two forms: the trial list of Part 16
// (feature_encoder.hip, three launches, a fresh encoder per trial) and the streams of Part 18 (feature_encoder_stream.hip, one
// launch per push, the encoder's state carried between pushes).  Device code only.
//
// Three bodies, named after the trial-list launches they are:
//  (A) fenc_tile_features: the spectrum, band energies, floor, DCT and LPC taps of one tile of FENC_TILE_FRAMES frames whose
//      pre-emphasised samples the caller has staged;
//  (B) fenc_frame_scores: the residual and the two score rows of one frame, one lag per lane;
//  (C) fenc_track_step: one sub-frame of the pitch track.
// Where the samples come from and where scores and taps go is the caller's; the sums and their order are here, so that both
// forms give equal bits for equal samples.
#pragma once

#include "feature_encoder.h"
#include "spectral_frame.h"

#define FENC_XROWS (FENC_TILE_FRAMES * FENC_FRAME + FENC_FRAME)      // samples the windows of a tile cover
#define FENC_RS (FENC_XROWS | 1)
#define FENC_PW 163                                                   // stride of a frame's power spectrum in LDS
#define FENC_PREEMPH ((double)0.85f)

static_assert(FENC_TILE_FRAMES == 16, "one MFMA tile of frames; the LPC passes take them eight at a time");

static __constant__ int c_fenc_edges[DSS_NB_BANDS] = {0, 4, 8, 12, 16, 20, 24, 28, 32, 40, 48, 56, 64, 80, 96, 112, 136, 160};

// ---- (A) ---------------------------------------------------------------------------------------------------------------
// LDS, in doubles: [tw 640 | win 320 | mean 16] [xs FENC_RS] [pw 16 x FENC_PW].  Behind the DFT the first region holds the LPC
// chain's per-frame scratch (floats), the second the band values, the float32 cepstrum and the chain's cosine table, the third
// (the power spectra, dead behind the band energies) the tile's taps where the caller asks for them.
#define FENC_R0 976
#define FENC_LDS (FENC_R0 + FENC_RS + FENC_TILE_FRAMES * FENC_PW)

struct FencTileView {
    SpecLds L;
    DssSpecDev p;
    DssSpecGeom g;
};

__device__ __forceinline__ FencTileView fenc_tile_view(double *lds)
{
    FencTileView w;
    w.L.tw = reinterpret_cast<double2 *>(lds);
    w.L.win = lds + 640;
    w.L.mean = lds + 960;
    w.L.xs = lds + FENC_R0;
    w.L.extra = w.L.xs + FENC_RS;
    w.p = {};
    w.p.nperseg = FENC_WINDOW; w.p.hop = FENC_FRAME; w.p.nfft = FENC_WINDOW; w.p.bins = FENC_BINS; w.p.nblk = (FENC_BINS + 15) / 16;
    w.p.K4 = FENC_WINDOW; w.p.sh = FENC_FRAME;
    w.g = {};
    w.g.F = FENC_TILE_FRAMES; w.g.f_shift = 4; w.g.CG = 1; w.g.cg_shift = 0; w.g.NB = 1; w.g.rows = FENC_XROWS; w.g.RS = FENC_RS;
    return w;
}

// twiddles, window and the (zero) means into the first region; the caller stages xs and holds the barrier
__device__ __forceinline__ void fenc_tile_tables(const FencTileView &w, const DssFencDev &v, int tid)
{
    for (int j = tid; j < FENC_WINDOW; j += FENC_THREADS) {
        w.L.tw[j] = reinterpret_cast<const double2 *>(v.tw)[j];
        w.L.win[j] = (double)v.window[j];
    }
    if (tid < FENC_TILE_FRAMES) w.L.mean[tid] = 0.0;
}

// The tile's frames 0 .. 15 from the staged xs (frame f's window starts at xs[160 f]), behind the caller's barrier.  Frames
// f < nvalid write outputs 0..17 and 20..35 to orow + 36 f; with taps given, every frame's 16 taps also go to taps[16 f ..]
// (floats in the third region), complete after the caller's next barrier.  Called by every thread of the workgroup.
__device__ __forceinline__ void fenc_tile_features(double *lds, const FencTileView &w, const DssFencDev &v, int nvalid,
                                                   float *__restrict__ orow, float *taps)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, row = lane & 15, kq = lane >> 4;
    double *pw = w.L.extra;

    // the DFT of the tile's 16 frames: a wave owns one block of 16 bins at a time
    for (int blk = wave; blk < w.p.nblk; blk += FENC_THREADS / 64) {
        spec_d4 re0, im0, re1, im1;
        spec_item(w.L, w.p, w.g, 0, blk, 0, re0, im0, re1, im1);
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
    __syncthreads();                                   // pw is dead from here on
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
        if (f < nvalid) orow[f * FENC_OUT + j] = c32;
    }
    __syncthreads();

    // the decoder's lpc_from_cepstrum on the float32 cepstrum: 32 lanes per frame, eight frames per pass
    float *fs = reinterpret_cast<float *>(lds);
    const int sub = tid >> 5, l = tid & 31;
    float *cs = fs + sub * 220, *exs = cs + 20, *as = cs + 40, *xr = cs + 60;
    static_assert(8 * 220 <= 2 * FENC_R0, "the first region holds the chain's scratch");
    static_assert(FENC_TILE_FRAMES * DSS_LPC_ORDER <= 2 * FENC_TILE_FRAMES * FENC_PW, "the third region holds the taps");
    for (int pass = 0; pass < FENC_TILE_FRAMES / 8; ++pass) {
        const int f = pass * 8 + sub;
        __syncthreads();
        if (l < DSS_NB_BANDS) cs[l] = l == 0 ? cep32[f * DSS_NB_BANDS] + 4 : cep32[f * DSS_NB_BANDS + l];
        __syncthreads();
        float lpc[DSS_LPC_ORDER];
        lpc_chain_frame(v.lpc, v.idct_scale, ck_lds, cs, exs, xr, as, l, lpc);
        if (l == 0) {
            if (f < nvalid) {
                float *dst = orow + f * FENC_OUT + 20;
#pragma unroll
                for (int i = 0; i < DSS_LPC_ORDER; ++i) dst[i] = lpc[i];
            }
            if (taps) {
#pragma unroll
                for (int i = 0; i < DSS_LPC_ORDER; ++i) taps[f * DSS_LPC_ORDER + i] = lpc[i];
            }
        }
    }
}

// ---- (B) ---------------------------------------------------------------------------------------------------------------
// Frame i of an encoder: e over t = 160 i - 336 .. 160 i + 80 (416 samples: 256 of history, the frame's 160), from r over one
// sample more and x over sixteen more.  Sample t takes the taps of frame (t + 80) / 160; before t = -80 everything is zero.
#define FENC_NE 416
#define FENC_NR (FENC_NE + 1)
#define FENC_NX (FENC_NR + DSS_LPC_ORDER)
#define FENC_SCORE_LDS (FENC_NX + FENC_NR + FENC_NE + FENC_LAGS)     // doubles: xs, rs, es, xcs

// The caller has staged xs[m] = x(160 i - 353 + m) and lp = the taps of frames i - 2 .. i (zeros for frames before 0); the
// barrier behind that staging is here.  Writes the damped scores and the sub-frame weight of the frame's two sub-frames to
// row0[0 .. 255] and row0[256 .. 511].  Called by every thread of the workgroup; no barrier behind the stores.
__device__ __forceinline__ void fenc_frame_scores(const double *xs, double *rs, double *es, double *xcs,
                                                  const float (*lp)[DSS_LPC_ORDER], long long i, double *row0)
{
    const int q = threadIdx.x;
    const long long tb = i * FENC_FRAME - (FENC_NE - FENC_FRAME / 2 + 1);                // t of rs[0]: 160 i - 337
    __syncthreads();
    for (int k = q; k < FENC_NR; k += FENC_THREADS) {
        const long long t = tb + k;
        double acc = 0.0;
        if (t >= -(FENC_FRAME / 2)) {
            const float *a = lp[(int)((t + FENC_FRAME / 2) / FENC_FRAME - (i - 2))];
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
    double *dst = row0 + q;
    dst[0] = q == FENC_LAGS - 1 ? 2.0 * aa[0] / tot : xc[0];
    dst[FENC_LAGS] = q == FENC_LAGS - 1 ? 2.0 * aa[1] / tot : xc[1];
}

// ---- (C) ---------------------------------------------------------------------------------------------------------------
// One sub-frame of the track: the max-plus recursion with one state per lane, the argmax as a workgroup reduction with the first
// index winning ties.  P (FENC_TRACK), red_v, red_i (one per wave) and bp (FENC_TRACK) are LDS; p_all and best are the same in
// every thread.  row is the sub-frame's score row; on a frame's second sub-frame (odd) the first one's row stands FENC_LAGS
// doubles before it and outputs 18 and 19 go to dst, the frame's output row.  Called by every thread of the workgroup, behind a
// barrier that follows the writes of P and of the row.
__device__ __forceinline__ void fenc_track_step(double *P, double *red_v, int *red_i, int *bp, const double *row, bool odd,
                                                double &p_all, int &best, float *dst)
{
    const int q = threadIdx.x, lane = q & 63, wave = q >> 6;
    const bool on = q < FENC_TRACK;
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
        if (odd) bp[q] = ptr;
    }
    p_all = bv;
    best = bi;
    __syncthreads();
    if (odd && q == 0) {
        const int q1 = best, q0 = bp[q1];
        int period2 = (256 - q0) + (256 - q1);
        period2 = period2 < 66 ? 66 : (period2 > 510 ? 510 : period2);
        const double *r0 = row - FENC_LAGS;
        dst[18] = (float)(0.01 * (double)(period2 - 200));
        dst[19] = (float)((r0[FENC_LAGS - 1] * r0[q0] + g * row[q1]) / 2.0 - 0.5);
    }
}
