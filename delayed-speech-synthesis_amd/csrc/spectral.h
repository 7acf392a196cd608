// csrc/spectral.h -- device view and launchers of the spectrogram kernels (spectral.hip), shared with the host side of Part 11
// of include/dss_hip.h (dss_spec.cpp).
#pragma once

#include "dss_common.h"

#define SPEC_THREADS 256
#define SPEC_LDS_SOFT 81920       // bytes of LDS per workgroup, half of gfx950's 160 KB: two workgroups share a CU
#define SPEC_KIND_TRIALS 0
#define SPEC_KIND_LOCKED 1
#define SPEC_KIND_MEAN 2

// One trial: rows first .. first + n of the signal array, W frames.  `out` is where the trial's result starts: its first
// output frame (spec_trials_kernel), or its place in the caller's list (spec_mean_partial_kernel).  `frame0` is the frame that
// column 0 of the locked result takes from this trial (onset - pre).
struct DssSpecTrial { long long first, n, out; int W, frame0; };
// One workgroup of spec_trials_kernel: frames frame0 .. frame0 + F of descriptor `trial`.
struct DssSpecTile { int trial, frame0; };

// How a workgroup is cut: F frames (a power of two <= 32) x CG channels (a power of two <= 16) x NB blocks of 16 bins.
struct DssSpecGeom {
    int F, f_shift, CG, cg_shift, NB;
    int rows, RS;                 // staged rows per channel ((F - 1) * sh + K4), and their stride in LDS (rows | 1)
    unsigned lds_bytes;
};

struct DssSpecDev {
    int nperseg, hop, nfft, bins, nblk;
    int K4, sh;                   // 4 * ceil(nperseg / 4); rows between frames in LDS: min(hop, K4)
    int mode, detrend, odd;       // odd: nfft is odd, so the last bin is doubled too
    double scale;                 // PSD: 1 / (fs * sum win^2); magnitude: its square root
    const double *win;            // [K4] the window, zeros behind nperseg
    const double *tw;             // [nfft][2] cos, sin of 2 pi j / nfft
};

// Fills g for a kernel kind and C channels; false when nothing fits (cannot happen inside the limits of dss_spec_check_params).
bool dss_spec_pick_geom(const DssSpecDev &v, int C, int kind, DssSpecGeom *g);

int dss_launch_spec_trials(const DssSpecDev &v, const DssSpecGeom &g, const double *d_x, int ld, int C, const DssSpecTrial *d_desc,
                           const DssSpecTile *d_tiles, int n_tiles, double *d_out, hipStream_t s);
int dss_launch_spec_locked(const DssSpecDev &v, const DssSpecGeom &g, const double *d_x, int ld, int C, const DssSpecTrial *d_desc,
                           int n_trials, int J, double *d_out, hipStream_t s);
int dss_launch_spec_mean(const DssSpecDev &v, const DssSpecGeom &g, const double *d_x, int ld, int C, const DssSpecTrial *d_desc,
                         int n_trials, long long total_frames, double *d_partial, double *d_out, hipStream_t s);
