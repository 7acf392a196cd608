// csrc/feature_encoder.h -- device view and launchers of the LPC feature encoder's kernels (feature_encoder.hip), shared with the
// host side of Part 16 of include/dss_hip.h (dss_fenc.cpp).
#pragma once

#include "dss_common.h"
#include "lpc_chain.h"

#define FENC_THREADS 256
#define FENC_TILE_FRAMES 16       // frames of one trial per workgroup of the spectrum launch (one MFMA tile of frames)
#define FENC_FRAME 160
#define FENC_WINDOW 320
#define FENC_BINS 161
#define FENC_OUT 36
#define FENC_LAGS 256             // score indices per sub-frame; column FENC_LAGS - 1 of a score row holds the sub-frame weight
#define FENC_TRACK 224            // indices the pitch track follows

// One trial: samples first .. first + n of the audio, `frames` = n / 160 frames, written from output frame `out` on.
struct DssFencTrial { long long first, n, out; int frames, pad; };
// One workgroup of the spectrum launch: frames frame0 .. frame0 + FENC_TILE_FRAMES of descriptor `trial`.
struct DssFencTile { int trial, frame0; };

struct DssFencDev {
    const float *window;          // [320] float32
    const double *tw;             // [320][2] cos, sin of 2 pi j / 320
    DssLpcTables lpc;
    double idct_scale;            // sqrt(2 / 18)
};

// The tables of `d` uploaded into `blocks` (dss_fenc.cpp): what dss_fenc_create and dss_fenc_streams_create set up.  For the
// host files, which include dss_host.h first.
#ifdef DSS_LOCAL
DSS_LOCAL int dss_fenc_setup(DssDevBlocks &blocks, DssFencDev *d);
#endif

// Part 18: what one stream's encoder carries from push to push.  A fresh encoder is the all-zero state: zero history gives
// x = +0.0 before the stream, zero taps stand for the frames before 0, the track starts at P = 0, p_all = 0, best = 0.
#define FENC_HIST (3 * FENC_FRAME)      // raw samples kept (the scores read 354 back); three frames, so the update is a shift
struct DssFencStreamState {
    double P[FENC_TRACK];
    double p_all;
    long long frames;             // frames encoded since the reset
    float taps[2][16];            // of the two newest frames
    int best, pad;
    short hist[FENC_HIST];        // the newest samples, oldest first
};

// One launch, a workgroup per stream: stream s encodes counts[s] (NULL: frames_max) frames of d_audio (S, 160 frames_max) into
// d_out36 (S, frames_max, 36), zeros in the rows past its count; a count of 0 leaves the stream's state alone.
int dss_launch_fenc_streams(const DssFencDev &v, const short *d_audio, int n_streams, int frames_max, const int *d_counts,
                            DssFencStreamState *d_states, float *d_out36, hipStream_t s);

// stamps: NULL, or four events recorded before, between and behind the three launches (development timing).
int dss_launch_fenc(const DssFencDev &v, const short *d_audio, const DssFencTrial *d_desc, int n_trials, const DssFencTile *d_tiles,
                    int n_tiles, float *d_out36, double *d_scores, hipStream_t s, const hipEvent_t *stamps);
