// csrc/contamination.h -- device view and launcher of the audio-ECoG spectrogram correlation kernels (contamination.hip), shared
// with the host side of Part 12 of include/dss_hip.h (dss_contam.cpp).
#pragma once

#include "spectral.h"

#define CONTAM_F 32               // frames per tile: both 16-frame halves of spec_item
#define CONTAM_PAD 32             // the kept bins padded to two blocks of 16; place n_bins of an audio frame holds the frame's mask
#define CONTAM_MAX_BINS 31
#define CONTAM_MAX_CHANNELS 65535     // the channels are the grid's y dimension
#define CONTAM_LG 8               // lags whose accumulators one wave keeps in registers (36 VGPRs per lag)
#define CONTAM_AS 48              // doubles between the frames of the audio window in LDS (lanes 16 apart hit other banks)
#define CONTAM_WAVES (SPEC_THREADS / 64)
#define CONTAM_AUD_THREADS 1024

struct DssContamDev {
    DssSpecDev spec;              // nfft = nperseg, magnitude, no detrending; the scale is not applied (correlations do not see it)
    DssSpecGeom geom;             // F = CONTAM_F, CG = 1
    int bin_lo, B;                // kept bins bin_lo .. bin_lo + B
    int L, nlag;                  // lags -L .. L
    int Z, lgn;                   // lag groups of the grid, lags per wave: Z * CONTAM_WAVES * lgn >= nlag, lgn <= CONTAM_LG
    unsigned lds_bytes;           // of the correlation kernel
};

// Doubles of one (chunk, lag, channel) record of partial sums: sum ab (B x B), sum b (B), sum b^2 (4 x B, one per K position).
__host__ __device__ static inline size_t contam_record(int B) { return (size_t)B * B + 5 * (size_t)B; }

// Fills everything but the table pointers from the checked parameters; false if the frame shape does not fit the LDS limit.
bool dss_contam_shape(int nperseg, int hop, int bin_lo, int n_bins, int max_lag, DssContamDev *v);

// Offsets, in doubles, of the seven arrays inside the result of a call with C channels: n (nlag), shift (B), sum a and sum a^2
// (nlag, B), sum b and sum b^2 (nlag, C, B), sum ab (nlag, C, B, B); [7] is the total.
void dss_contam_layout(const DssContamDev &v, int C, long long off[8]);

// All launches of one call, queued on s.  d_keep: W bytes; d_aud: W x CONTAM_PAD doubles of workspace; d_shift: CONTAM_PAD doubles;
// d_partial: chunks x nlag x C records.
int dss_launch_contam(const DssContamDev &v, const double *d_x, int ld, int C, const double *d_audio, long long T, int W,
                      const unsigned char *d_keep, double *d_aud, double *d_shift, double *d_partial, int chunks, int tiles_per_chunk,
                      double *d_out, hipStream_t s);
