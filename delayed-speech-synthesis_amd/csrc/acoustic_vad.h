// csrc/acoustic_vad.h -- device view and launchers of the acoustic (energy based) VAD labels (acoustic_vad.hip), shared with
// the host side of Part 7 of include/dss_hip.h (dss_avad.cpp).
#pragma once

#include "dss_common.h"

#define AVAD_TILE_FRAMES 32       // frames one workgroup of avad_energy_kernel transforms (two 16-row MFMA tiles)
#define AVAD_MAX_BANDS 64
#define AVAD_LDS_LIMIT 163840     // bytes of LDS one workgroup may take on gfx950
#define AVAD_PEAK_TILE 4096       // samples one workgroup of avad_peak_kernel / avad_prepare_kernel takes

// One trial: `lead` zeros, then audio[first .. first + n - lead); W frames written from out_frame on; `index` is the trial's
// place in the caller's list (the table is sorted longest first).  `normalize`: the trial's samples are scaled by the factor of
// its peak and by the post gain (avad_gain.h); its prepared samples are written from out_sample on.
struct DssAvadTrialDesc { long long first, out_frame, out_sample; int n, lead, W, silence, index, normalize; };
// One workgroup of the energy kernel: frames frame0 .. frame0 + AVAD_TILE_FRAMES of descriptor `trial`; of the prepare kernel:
// samples frame0 .. frame0 + AVAD_PEAK_TILE of it.
struct DssAvadTile { int trial, frame0; };
// One workgroup of the peak kernel: audio[first .. first + n), n <= AVAD_PEAK_TILE, of the trial at place `index` in the list.
struct DssAvadPeakTile { long long first; int n, index; };

struct DssAvadDev {
    int N, shift, bins, bands;    // window samples, frame shift, N / 2 + 1 spectrum bins, mel bands
    int context;                  // frames of context of the vote
    double threshold, mean_scale, proportion;
    const double *win;            // [N] window[k] * 2^-15 (the int16 -> [-1, 1) scaling is exact and folded in)
    const double *tw;             // [N][2] cos, sin of 2 pi j / N
    const double *mel_w;          // the nonzero run of every band's column of the mel matrix, band after band
    const int *band_lo;           // [bands] first bin of that run
    const int *band_off;          // [bands + 1] its place in mel_w
    const double *gain;           // [AVAD_GAIN_ENTRIES] factor by peak (dss_avad_set_gain), NULL before it
    double post_gain;             // the second factor
};

size_t dss_avad_energy_lds_bytes(int N, int shift, int bins, int bands);
int dss_launch_avad_energy(const DssAvadDev &v, const short *d_audio, const DssAvadTrialDesc *d_desc, const DssAvadTile *d_tiles,
                           int n_tiles, double *d_log_energy, const int *d_peaks, hipStream_t s);
int dss_launch_avad_peak(const short *d_audio, const DssAvadPeakTile *d_tiles, int n_tiles, int *d_peaks, hipStream_t s);
int dss_launch_avad_prepare(const DssAvadDev &v, const short *d_audio, const DssAvadTrialDesc *d_desc, const DssAvadTile *d_tiles,
                            int n_tiles, const int *d_peaks, short *d_prepared, hipStream_t s);
int dss_launch_avad_vote(const DssAvadDev &v, const DssAvadTrialDesc *d_desc, int n_trials, const double *d_log_energy,
                         unsigned char *d_labels, double *d_threshold, hipStream_t s);
