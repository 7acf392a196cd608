// csrc/lpc_chain.h -- lpc_from_cepstrum (freq.c) for one frame on 32 lanes, shared by the decoder's frame_lpc_kernel
// (lpcnet_frame.hip) and the feature encoder's spectrum launch (feature_encoder.hip), which writes with it the taps the decoder
// will later derive from the same cepstrum.  Device code only.
//
// The chain of a frame -- inverse DCT of the cepstrum, band energies, band interpolation, the 17 autocorrelation lags as a
// direct inverse DFT (160 terms each, in ascending bin order), lag window, Levinson-Durbin -- with the reference's operation
// order inside every element; what is independent runs on different lanes: one band per lane, one bin per lane, one LAG per
// lane (its 160-term sum stays one sequential chain), and the recursion on one lane.  One lane per frame (rounds 1-3) took
// 60 us whatever the batch: 160 x 17 dependent pairs of instructions per lane behind scalar loads of the cosine table.
#pragma once

#include "dss_common.h"

#define LPC_CK_STRIDE 20          // floats per bin of the LDS copy of cos_kl (17 lags, padded)

// The derived tables the chain reads (csrc/lpc_tables.h builds them on the host).
struct DssLpcTables {
    const float *dct_table;       // [18*18]
    const float *cos_kl;          // [160][17]
    const float *interp_a, *interp_b;   // [160]
    const double *lag_window;     // [17]
};

static __constant__ float c_compensation[DSS_NB_BANDS] = {0.8f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 1.f, 0.666667f, 0.5f, 0.5f, 0.5f,
                                                          0.333333f, 0.25f, 0.25f, 0.2f, 0.166667f, 0.173913f};

// cos_kl into its LDS copy, by all `threads` threads of the block; the caller's barrier follows.
__device__ __forceinline__ void lpc_chain_load_ck(const DssLpcTables &T, float (*ck_lds)[LPC_CK_STRIDE], int tid, int threads)
{
    for (int k = tid; k < 160 * (DSS_LPC_ORDER + 1); k += threads) ck_lds[k / (DSS_LPC_ORDER + 1)][k % (DSS_LPC_ORDER + 1)] = T.cos_kl[k];
}

// One frame on lanes l = 0 .. 31.  Called by EVERY thread of the block at the same place (it holds three barriers), after a
// barrier behind the writes of ck_lds and of cs (the cepstrum, 4 already added to cs[0]).  exs (18), xr (160) and as (17) are
// the frame's own LDS scratch.  Lane 0 returns the taps in lpc; the other lanes' lpc is not touched.
__device__ __forceinline__ void lpc_chain_frame(const DssLpcTables &T, double idct_scale, const float (*ck_lds)[LPC_CK_STRIDE],
                                                const float *cs, float *exs, float *xr, float *as, int l, float lpc[DSS_LPC_ORDER])
{
    constexpr int eband5ms[DSS_NB_BANDS] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40};
    if (l < DSS_NB_BANDS) {                                                 // band l: inverse DCT term by term, then the energy
        float sum = 0;
#pragma unroll
        for (int j = 0; j < DSS_NB_BANDS; ++j) sum += cs[j] * T.dct_table[l * DSS_NB_BANDS + j];
        const float e = (float)((double)sum * idct_scale);                 // sum*sqrt(2./NB_BANDS)
        exs[l] = (float)(pow(10.0, (double)e) * (double)c_compensation[l]);
    }
    __syncthreads();
    for (int k = l; k < 160; k += 32) {                                     // interp_band_gain: bin k lies in band i
        int i = 0;
#pragma unroll
        for (int q = 1; q < DSS_NB_BANDS - 1; ++q) i += (k >= eband5ms[q] * 4);
        xr[k] = T.interp_a[k] * exs[i] + T.interp_b[k] * exs[i + 1];
    }
    __syncthreads();
    if (l <= DSS_LPC_ORDER) {                                               // lag l: direct inverse DFT, bins ascending
        float ac = xr[0];
        for (int k = 1; k < 160; ++k) {
            const float x2 = 2.f * xr[k];
            ac += x2 * ck_lds[k][l];
        }
        float a;
        if (l == 0) a = (float)((double)ac + ((double)ac * 1e-4 + 320 / 12 / 38.));
        else a = (float)((double)ac * T.lag_window[l]);
        as[l] = a;
    }
    __syncthreads();
    if (l == 0) {                                                           // Levinson-Durbin (the recursion is serial)
        float a[DSS_LPC_ORDER + 1];
#pragma unroll
        for (int i = 0; i <= DSS_LPC_ORDER; ++i) a[i] = as[i];
#pragma unroll
        for (int i = 0; i < DSS_LPC_ORDER; ++i) lpc[i] = 0.f;
        float error = a[0];
        bool live = a[0] != 0;
#pragma unroll
        for (int i = 0; i < DSS_LPC_ORDER; i++) {
            if (live) {
                float rr = 0;
#pragma unroll
                for (int j = 0; j < i; j++) rr += lpc[j] * a[i - j];
                rr += a[i + 1];
                const float r = -rr / error;
                lpc[i] = r;
#pragma unroll
                for (int j = 0; j < (i + 1) >> 1; j++) {
                    const float tmp1 = lpc[j], tmp2 = lpc[i - 1 - j];
                    lpc[j] = tmp1 + r * tmp2;
                    lpc[i - 1 - j] = tmp2 + r * tmp1;
                }
                error = error - (r * r) * error;
                if (error < .001f * a[0]) live = false;                      // the C loop's break
            }
        }
    }
}
