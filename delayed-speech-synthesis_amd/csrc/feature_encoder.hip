// csrc/feature_encoder.hip -- the LPC feature encoder over a trial list (gfx950): Part 16 of include/dss_hip.h.
//
// The method is this project's statement of the published encoder (tests/feature_encoder_reference.py is the
// binding definition): per 160-sample frame 18 Bark cepstral coefficients, the pitch feature and correlation, 16 LPC taps.  One
// fresh encoder per trial.  Three launches on one stream:
//
//  (A) fenc_spectrum_kernel, one workgroup per FENC_TILE_FRAMES frames of one trial.  The pre-emphasised samples the tile's
//      windows cover are staged in LDS once (overlapping windows re-read LDS); the 320 x 161 DFT of 16 frames is spec_item
//      (spectral_frame.h) on v_mfma_f64_16x16x4_f64; band energies, log and floor, DCT in fp64, rounded to float32 once at the
//      store; then the decoder's own lpc_from_cepstrum (lpc_chain.h, fp32) on that float32 cepstrum.  Writes outputs 0..17 and
//      20..35; the taps in the output rows are what (B) reads.
//  (B) fenc_scores_kernel, one workgroup per frame, one lag per lane.  The frame's residual stretch and 256 samples of history
//      are recomputed from the audio with the OWNING frames' taps (frames i - 2 .. i), nothing is carried between workgroups.
//      Writes the damped scores and the sub-frame weight to the (sub-frames, 256) fp64 scratch.
//  (C) fenc_track_kernel, one workgroup per trial, serial over its sub-frames: the max-plus recursion with one state per lane,
//      the argmax as a workgroup reduction with the first index winning ties.  Writes outputs 18 and 19.
//
// Sums whose order decides equal bits with the reference for equal inputs (DCT, residual, track) add their terms in its order;
// the build forbids contraction.  The bodies of the three launches are stated in fenc_blocks.h, which the stream form of Part 18
// (feature_encoder_stream.hip) shares; here is where a trial's samples come from and where the scores go.
#include "fenc_blocks.h"

__device__ __forceinline__ double fenc_preemph(const short *__restrict__ s, long long t, long long n)
{
    if (t < 0 || t >= n) return 0.0;
    const double prev = t > 0 ? (double)s[t - 1] : 0.0;
    return (double)s[t] + (-FENC_PREEMPH) * prev;
}

// ---- (A) ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FENC_THREADS)
fenc_spectrum_kernel(DssFencDev v, const short *__restrict__ audio, const DssFencTrial *__restrict__ desc,
                     const DssFencTile *__restrict__ tiles, float *__restrict__ out36)
{
    __shared__ __attribute__((aligned(16))) double lds[FENC_LDS];
    const DssFencTile tile = tiles[blockIdx.x];
    const DssFencTrial d = desc[tile.trial];
    const short *s = audio + d.first;
    const int tid = threadIdx.x;

    const FencTileView w = fenc_tile_view(lds);
    fenc_tile_tables(w, v, tid);
    const long long t0 = (long long)tile.frame0 * FENC_FRAME - FENC_FRAME;
    for (int r = tid; r < FENC_RS; r += FENC_THREADS) w.L.xs[r] = r < FENC_XROWS ? fenc_preemph(s, t0 + r, d.n) : 0.0;
    __syncthreads();
    fenc_tile_features(lds, w, v, d.frames - tile.frame0, out36 + (d.out + tile.frame0) * FENC_OUT, nullptr);
}

// ---- (B) ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FENC_THREADS)
fenc_scores_kernel(const short *__restrict__ audio, const DssFencTrial *__restrict__ desc, const DssFencTile *__restrict__ tiles,
                   const float *__restrict__ out36, double *__restrict__ scores)
{
    __shared__ double xs[FENC_NX], rs[FENC_NR], es[FENC_NE], xcs[FENC_LAGS];
    __shared__ float lp[3][DSS_LPC_ORDER];
    const DssFencTile tile = tiles[blockIdx.x / FENC_TILE_FRAMES];
    const DssFencTrial d = desc[tile.trial];
    const int i = tile.frame0 + (int)(blockIdx.x % FENC_TILE_FRAMES);
    if (i >= d.frames) return;
    const short *s = audio + d.first;
    const int q = threadIdx.x;
    const long long tb = (long long)i * FENC_FRAME - (FENC_NE - FENC_FRAME / 2 + 1);      // t of rs[0]: 160 i - 337

    if (q < 3 * DSS_LPC_ORDER) {
        const int fr = i - 2 + q / DSS_LPC_ORDER;
        lp[q / DSS_LPC_ORDER][q % DSS_LPC_ORDER] = fr >= 0 ? out36[(d.out + fr) * FENC_OUT + 20 + q % DSS_LPC_ORDER] : 0.f;
    }
    for (int m = q; m < FENC_NX; m += FENC_THREADS) xs[m] = fenc_preemph(s, tb - DSS_LPC_ORDER + m, d.n);
    fenc_frame_scores(xs, rs, es, xcs, lp, i, scores + (2 * (d.out + i)) * FENC_LAGS);
}

// ---- (C) ---------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(FENC_THREADS)
fenc_track_kernel(const DssFencTrial *__restrict__ desc, const double *__restrict__ scores, float *__restrict__ out36)
{
    __shared__ double P[FENC_TRACK], red_v[FENC_THREADS / 64];
    __shared__ int red_i[FENC_THREADS / 64], bp[FENC_TRACK];
    const DssFencTrial d = desc[blockIdx.x];
    const int q = threadIdx.x;
    if (q < FENC_TRACK) P[q] = 0.0;
    double p_all = 0.0;
    int best = 0;
    __syncthreads();
    for (int sf = 0; sf < 2 * d.frames; ++sf)
        fenc_track_step(P, red_v, red_i, bp, scores + (2 * d.out + sf) * FENC_LAGS, sf & 1, p_all, best,
                        out36 + (d.out + (sf >> 1)) * FENC_OUT);
}

int dss_launch_fenc(const DssFencDev &v, const short *d_audio, const DssFencTrial *d_desc, int n_trials, const DssFencTile *d_tiles,
                    int n_tiles, float *d_out36, double *d_scores, hipStream_t s, const hipEvent_t *stamps)
{
    if (n_tiles < 1) return DSS_OK;
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[0], s));
    hipLaunchKernelGGL(fenc_spectrum_kernel, dim3(n_tiles), dim3(FENC_THREADS), 0, s, v, d_audio, d_desc, d_tiles, d_out36);
    DSS_HIP_CHECK(hipGetLastError());
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[1], s));
    hipLaunchKernelGGL(fenc_scores_kernel, dim3((unsigned)n_tiles * FENC_TILE_FRAMES), dim3(FENC_THREADS), 0, s, d_audio, d_desc, d_tiles,
                       d_out36, d_scores);
    DSS_HIP_CHECK(hipGetLastError());
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[2], s));
    hipLaunchKernelGGL(fenc_track_kernel, dim3(n_trials), dim3(FENC_THREADS), 0, s, d_desc, d_scores, d_out36);
    DSS_HIP_CHECK(hipGetLastError());
    if (stamps) DSS_HIP_CHECK(hipEventRecord(stamps[3], s));
    return DSS_OK;
}
