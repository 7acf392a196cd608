// csrc/spectral_frame.h -- the frame arithmetic of the spectrogram kernels, shared by spectral.hip (Part 11 of include/dss_hip.h)
// and contamination.hip (Part 12): the LDS view of a workgroup, the staging of the rows of F frames, the frames' means and the
// DFT of one (channel, block of 16 bins) on v_mfma_f64_16x16x4_f64.  Device code only; spectral.hip's header comment describes
// the layouts.
#pragma once

#include "spectral.h"

typedef double spec_d4 __attribute__((ext_vector_type(4)));

struct SpecLds {
    double2 *tw;      // [nfft] (cos, sin)
    double *win;      // [K4]
    double *mean;     // [F][CG]
    double *xs;       // [CG][RS]
    double *extra;    // what the kernel keeps behind them
};

__device__ __forceinline__ SpecLds spec_lds(double *lds, const DssSpecDev &p, const DssSpecGeom &g)
{
    SpecLds L;
    L.tw = reinterpret_cast<double2 *>(lds);
    L.win = lds + 2 * p.nfft;
    L.mean = L.win + p.K4;
    L.xs = L.mean + g.F * g.CG;
    L.extra = L.xs + g.CG * g.RS;
    return L;
}

__device__ __forceinline__ void spec_load_tables(const SpecLds &L, const DssSpecDev &p)
{
    for (int j = threadIdx.x; j < p.nfft; j += SPEC_THREADS) L.tw[j] = reinterpret_cast<const double2 *>(p.tw)[j];
    for (int j = threadIdx.x; j < p.K4; j += SPEC_THREADS) L.win[j] = p.win[j];
}

// Rows of frames fr0 .. fr0 + F of trial d, channels c0 .. c0 + CG, to xs.  Nothing is read behind the trial's last row or
// beyond channel C: those places hold zeros.
__device__ __forceinline__ void spec_stage(const SpecLds &L, const DssSpecDev &p, const DssSpecGeom &g, const double *__restrict__ x,
                                           int ld, int C, const DssSpecTrial &d, long long fr0, int c0)
{
    const int total = g.rows << g.cg_shift;
    const bool apart = p.sh != p.hop;                // frames do not overlap: each is staged on its own
    for (int q = threadIdx.x; q < total; q += SPEC_THREADS) {
        const int r = q >> g.cg_shift, c = q & (g.CG - 1);
        long long t;
        bool ok = c0 + c < C;
        if (apart) {
            const int f = r / p.K4, k = r - f * p.K4;
            t = (fr0 + f) * p.hop + k;
            ok = ok && k < p.nperseg;
        } else {
            t = fr0 * p.hop + r;
        }
        ok = ok && t < d.n;
        L.xs[c * g.RS + r] = ok ? x[(d.first + t) * ld + c0 + c] : 0.0;
    }
}

// The mean of every staged frame, its samples added in order (0 without detrending).
__device__ __forceinline__ void spec_means(const SpecLds &L, const DssSpecDev &p, const DssSpecGeom &g)
{
    for (int q = threadIdx.x; q < (g.F << g.cg_shift); q += SPEC_THREADS) {
        const int f = q & (g.F - 1), c = q >> g.f_shift;
        double s = 0.0;
        if (p.detrend) {
            const double *v = L.xs + c * g.RS + f * p.sh;
            for (int k = 0; k < p.nperseg; ++k) s += v[k];
            s /= (double)p.nperseg;
        }
        L.mean[f * g.CG + c] = s;
    }
}

// Channel c (inside the group), bins bin0 + 16 blk .. bin0 + 16 blk + 15: the DFT sums of frames 0 .. 15 (re0, im0) and 16 .. 31 (re1, im1).
__device__ __forceinline__ void spec_item(const SpecLds &L, const DssSpecDev &p, const DssSpecGeom &g, int c, int blk, int bin0,
                                          spec_d4 &re0, spec_d4 &im0, spec_d4 &re1, spec_d4 &im1)
{
    const int lane = threadIdx.x & 63, row = lane & 15, kq = lane >> 4;
    const int bin = bin0 + blk * 16 + row;
    const int b = bin < p.bins ? bin : 0;
    const bool v0 = row < g.F, v1 = row + 16 < g.F;
    const double *x0 = L.xs + c * g.RS + (v0 ? row * p.sh : 0) + kq;
    const double *x1 = L.xs + c * g.RS + (v1 ? (row + 16) * p.sh : 0) + kq;
    const double m0 = v0 ? L.mean[row * g.CG + c] : 0.0;
    const double m1 = v1 ? L.mean[(row + 16) * g.CG + c] : 0.0;
    const double *wq = L.win + kq;
    int idx = (int)(((long long)b * kq) % p.nfft);
    const int step = (int)((4LL * b) % p.nfft);
    const spec_d4 zero = {0.0, 0.0, 0.0, 0.0};
    re0 = zero; im0 = zero; re1 = zero; im1 = zero;
    const bool two = g.F > 16;
    for (int k = 0; k < p.K4; k += 4) {
        const double2 t = L.tw[idx];
        const double w = wq[k];
        const bool live = k + kq < p.nperseg;
        const double a0 = (live && v0) ? (x0[k] - m0) * w : 0.0;
        re0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, t.x, re0, 0, 0, 0);
        im0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, t.y, im0, 0, 0, 0);
        if (two) {
            const double a1 = (live && v1) ? (x1[k] - m1) * w : 0.0;
            re1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, t.x, re1, 0, 0, 0);
            im1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, t.y, im1, 0, 0, 0);
        }
        idx += step;
        if (idx >= p.nfft) idx -= p.nfft;
    }
}
