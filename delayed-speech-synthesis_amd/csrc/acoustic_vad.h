// csrc/acoustic_vad.h -- device view and launchers of the acoustic (energy based) VAD labels (acoustic_vad.hip), shared with
// the host side of Part 7 of include/dss_hip.h (dss_avad.cpp).
#pragma once

#include "dss_common.h"

#define AVAD_TILE_FRAMES 32       // frames one workgroup of avad_energy_kernel transforms (two 16-row MFMA tiles)
#define AVAD_MAX_BANDS 64
#define AVAD_LDS_LIMIT 163840     // bytes of LDS one workgroup may take on gfx950

// One trial: `lead` zeros, then audio[first .. first + n - lead); W frames written from out_frame on; `index` is the trial's
// place in the caller's list (the table is sorted longest first).
struct DssAvadTrialDesc { long long first, out_frame; int n, lead, W, silence, index, pad; };
// One workgroup of the energy kernel: frames frame0 .. frame0 + AVAD_TILE_FRAMES of descriptor `trial`.
struct DssAvadTile { int trial, frame0; };

struct DssAvadDev {
    int N, shift, bins, bands;    // window samples, frame shift, N / 2 + 1 spectrum bins, mel bands
    int context;                  // frames of context of the vote
    double threshold, mean_scale, proportion;
    const double *win;            // [N] window[k] * 2^-15 (the int16 -> [-1, 1) scaling is exact and folded in)
    const double *tw;             // [N][2] cos, sin of 2 pi j / N
    const double *mel_w;          // the nonzero run of every band's column of the mel matrix, band after band
    const int *band_lo;           // [bands] first bin of that run
    const int *band_off;          // [bands + 1] its place in mel_w
};

size_t dss_avad_energy_lds_bytes(int N, int shift, int bins, int bands);
int dss_launch_avad_energy(const DssAvadDev &v, const short *d_audio, const DssAvadTrialDesc *d_desc, const DssAvadTile *d_tiles,
                           int n_tiles, double *d_log_energy, hipStream_t s);
int dss_launch_avad_vote(const DssAvadDev &v, const DssAvadTrialDesc *d_desc, int n_trials, const double *d_log_energy,
                         unsigned char *d_labels, double *d_threshold, hipStream_t s);
