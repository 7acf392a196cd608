// csrc/feature_encoder_stream.hip -- the LPC feature encoder on streams (gfx950): Part 18 of include/dss_hip.h.
//
// The encoder of Part 16 is causal: frame i reads samples up to 160 i + 159 and nothing later, so any chunking of a stream gives
// the bits of the whole trial once everything frame i needs from before the chunk is carried (DssFencStreamState, feature_encoder.h):
// 480 raw samples, the float32 taps of frames i - 2 and i - 1, the track's P, p_all and best, and the frame counter.
//
// One kernel, one 256-thread workgroup per stream, one launch per push whatever the numbers of streams and frames.  Per tile of up
// to FENC_TILE_FRAMES frames the workgroup stages history plus new samples and runs body (A) of fenc_blocks.h; then, frame by
// frame, body (B) with the two score rows kept in LDS, and the two track steps (C) on them.  Scores never reach global memory.
// Behind the last tile it stores the history, the two newest tap rows and the track state.  A workgroup touches its own stream's
// state only; nothing crosses workgroups, and every loop bound comes from counts the host has checked.
//
// LDS: the tile regions of (A) (FENC_LDS doubles); behind (A) their first FENC_SCORE_LDS + 2 FENC_LAGS doubles hold (B)'s arrays
// and the two score rows, and the tile's taps wait in the third region until they are copied out.  Beside them only what lives
// across tiles: the track state and FENC_TILE_FRAMES + 2 tap rows.
#include "fenc_blocks.h"

static_assert(FENC_SCORE_LDS + 2 * FENC_LAGS <= FENC_R0 + FENC_RS, "(B)'s arrays and the score rows lie before the tile's taps");
static_assert(FENC_HIST >= FENC_NE - FENC_FRAME / 2 + 1 + DSS_LPC_ORDER + 1, "the scores read this far back");
static_assert(sizeof(DssFencStreamState) % 8 == 0, "states are an array");

__global__ void __launch_bounds__(FENC_THREADS)
fenc_stream_kernel(DssFencDev v, const short *__restrict__ audio, int frames_max, const int *__restrict__ counts,
                   DssFencStreamState *__restrict__ states, float *__restrict__ out36)
{
    __shared__ __attribute__((aligned(16))) double lds[FENC_LDS];
    __shared__ double P[FENC_TRACK], red_v[FENC_THREADS / 64];
    __shared__ int red_i[FENC_THREADS / 64], bp[FENC_TRACK];
    __shared__ float lpt[FENC_TILE_FRAMES + 2][DSS_LPC_ORDER];       // the taps of frames f0 - 2 .. f0 + 15 of the tile at f0
    const int tid = threadIdx.x;
    const int K = counts ? counts[blockIdx.x] : frames_max;
    float *orow = out36 + (size_t)blockIdx.x * frames_max * FENC_OUT;
    for (int j = K * FENC_OUT + tid; j < frames_max * FENC_OUT; j += FENC_THREADS) orow[j] = 0.f;
    if (K < 1) return;

    DssFencStreamState *st = states + blockIdx.x;
    const short *a = audio + (size_t)blockIdx.x * frames_max * FENC_FRAME;
    const short *hist = st->hist;
    const long long seen = st->frames;
    const int n = K * FENC_FRAME;
    // sample t of the push, t >= -FENC_HIST: the history before 0.  x(t) needs t - 1 as well.
    auto sample = [&](int t) { return (double)(t < 0 ? hist[FENC_HIST + t] : a[t]); };
    auto preemph = [&](int t) { return sample(t) + (-FENC_PREEMPH) * sample(t - 1); };

    if (tid < FENC_TRACK) P[tid] = st->P[tid];
    if (tid < 2 * DSS_LPC_ORDER) lpt[tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER] = st->taps[tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER];
    double p_all = st->p_all;
    int best = st->best;

    const FencTileView w = fenc_tile_view(lds);
    double *xs = lds, *rs = xs + FENC_NX, *es = rs + FENC_NR, *xcs = es + FENC_NE, *rows = xcs + FENC_LAGS;
    float *tile_taps = reinterpret_cast<float *>(w.L.extra);
    for (int f0 = 0; f0 < K; f0 += FENC_TILE_FRAMES) {
        const int nv = K - f0 < FENC_TILE_FRAMES ? K - f0 : FENC_TILE_FRAMES;
        __syncthreads();                               // the tile before is done with lds
        fenc_tile_tables(w, v, tid);
        const int t0 = f0 * FENC_FRAME - FENC_FRAME;
        for (int r = tid; r < FENC_RS; r += FENC_THREADS) w.L.xs[r] = (r < FENC_XROWS && t0 + r < n) ? preemph(t0 + r) : 0.0;
        __syncthreads();
        fenc_tile_features(lds, w, v, nv, orow + f0 * FENC_OUT, tile_taps);
        __syncthreads();
        lpt[2 + tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER] = tile_taps[tid];
        static_assert(FENC_THREADS == FENC_TILE_FRAMES * DSS_LPC_ORDER, "one tap per thread");
        __syncthreads();

        for (int f = 0; f < nv; ++f) {
            const int tx = (f0 + f) * FENC_FRAME - (FENC_NE - FENC_FRAME / 2 + 1) - DSS_LPC_ORDER;      // t of xs[0]: 160 i - 353
            for (int m = tid; m < FENC_NX; m += FENC_THREADS) xs[m] = preemph(tx + m);
            fenc_frame_scores(xs, rs, es, xcs, lpt + f, seen + f0 + f, rows);
            __syncthreads();
            float *dst = orow + (f0 + f) * FENC_OUT;
            fenc_track_step(P, red_v, red_i, bp, rows, false, p_all, best, dst);
            fenc_track_step(P, red_v, red_i, bp, rows + FENC_LAGS, true, p_all, best, dst);
        }
        __syncthreads();
        float keep = 0.f;                              // the two newest rows move to the front
        if (tid < 2 * DSS_LPC_ORDER) keep = lpt[nv + tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER];
        __syncthreads();
        if (tid < 2 * DSS_LPC_ORDER) lpt[tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER] = keep;
    }
    __syncthreads();

    // the state behind the push; the new history may still read the old one
    short h[(FENC_HIST + FENC_THREADS - 1) / FENC_THREADS];
#pragma unroll
    for (int k = 0; k < (FENC_HIST + FENC_THREADS - 1) / FENC_THREADS; ++k) {
        const int j = tid + k * FENC_THREADS;
        h[k] = 0;
        if (j < FENC_HIST) { const int t = n - FENC_HIST + j; h[k] = t < 0 ? hist[FENC_HIST + t] : a[t]; }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < (FENC_HIST + FENC_THREADS - 1) / FENC_THREADS; ++k) {
        const int j = tid + k * FENC_THREADS;
        if (j < FENC_HIST) st->hist[j] = h[k];
    }
    if (tid < FENC_TRACK) st->P[tid] = P[tid];
    if (tid < 2 * DSS_LPC_ORDER) st->taps[tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER] = lpt[tid / DSS_LPC_ORDER][tid % DSS_LPC_ORDER];
    if (tid == 0) { st->p_all = p_all; st->best = best; st->frames = seen + K; }
}

int dss_launch_fenc_streams(const DssFencDev &v, const short *d_audio, int n_streams, int frames_max, const int *d_counts,
                            DssFencStreamState *d_states, float *d_out36, hipStream_t s)
{
    if (n_streams < 1 || frames_max < 1) return DSS_OK;
    hipLaunchKernelGGL(fenc_stream_kernel, dim3(n_streams), dim3(FENC_THREADS), 0, s, v, d_audio, frames_max, d_counts, d_states, d_out36);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
