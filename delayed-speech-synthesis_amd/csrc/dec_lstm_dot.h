// csrc/dec_lstm_dot.h -- the gate-row dot product of the bidirectional decoder's kernels (bilstm_decoder.hip: inference;
// dec_train.hip: the forward half of a training trial): one thread per gate row over the packed weight copies of DssDecDev.
#pragma once

#include "dss_common.h"


#define DEC_THREADS 512           // >= 4 * H and >= W * H
#define DEC_MAXH DSS_DEC_MAXH              // (a multiple of 4)
#define DEC_MAXC DSS_DEC_MAXC              // inputs of a layer: n_inputs for layer 0, 2H above it
#define DEC_TP 4                  // steps whose input halves (W_ih x) are formed in one pass over W_ih

typedef float df4 __attribute__((ext_vector_type(4)));
template <int W> struct DecVec { typedef float type __attribute__((ext_vector_type(W))); };
template <> struct DecVec<1> { struct type { float v; __device__ float &operator[](int) { return v; } __device__ const float &operator[](int) const { return v; } }; };

__device__ __forceinline__ float dec_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// Gate rows times inputs: wq is [n / 4][4H][4] (four consecutive inputs of a row side by side); n a multiple of 4 (the host pads with
// zero weights, the kernel keeps the padded inputs at zero); x is [input][W streams] in LDS.
// the input halves of DEC_TP steps' gate rows at once: one pass over W_ih (n / 4 sixteen-byte loads per thread) serves DEC_TP
// steps.  acc[tt] accumulates exactly the terms, in exactly the order, dec_dot would give step tt.
template <int W, typename V>
__device__ __forceinline__ void dec_dot_steps(V (&acc)[DEC_TP], const float *__restrict__ wq, int H4, int row, const V (*x)[DEC_MAXC], int n)
{
    const df4 *wr = reinterpret_cast<const df4 *>(wq) + row;
    int q = 0;
    for (; q + 4 <= n / 4; q += 4) {
        df4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wr[(size_t)(q + u) * H4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int tt = 0; tt < DEC_TP; ++tt) {
                const V x0 = x[tt][4 * (q + u)], x1 = x[tt][4 * (q + u) + 1], x2 = x[tt][4 * (q + u) + 2], x3 = x[tt][4 * (q + u) + 3];
#pragma unroll
                for (int s = 0; s < W; ++s) {
                    acc[tt][s] = __builtin_fmaf(w[u].x, x0[s], acc[tt][s]);
                    acc[tt][s] = __builtin_fmaf(w[u].y, x1[s], acc[tt][s]);
                    acc[tt][s] = __builtin_fmaf(w[u].z, x2[s], acc[tt][s]);
                    acc[tt][s] = __builtin_fmaf(w[u].w, x3[s], acc[tt][s]);
                }
            }
        }
    }
    for (; q < n / 4; ++q) {
        const df4 w = wr[(size_t)q * H4];
#pragma unroll
        for (int tt = 0; tt < DEC_TP; ++tt) {
            const V x0 = x[tt][4 * q], x1 = x[tt][4 * q + 1], x2 = x[tt][4 * q + 2], x3 = x[tt][4 * q + 3];
#pragma unroll
            for (int s = 0; s < W; ++s) {
                acc[tt][s] = __builtin_fmaf(w.x, x0[s], acc[tt][s]);
                acc[tt][s] = __builtin_fmaf(w.y, x1[s], acc[tt][s]);
                acc[tt][s] = __builtin_fmaf(w.z, x2[s], acc[tt][s]);
                acc[tt][s] = __builtin_fmaf(w.w, x3[s], acc[tt][s]);
            }
        }
    }
}
