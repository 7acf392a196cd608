// csrc/vad_lstm_dot.h -- the gate-row dot products of the neural detector's kernels (vad_lstm.hip: inference; vad_train.hip: the
// forward half of a training window): one thread per gate row over the packed weight copies of DssVadDev.
#pragma once

#include "dss_common.h"

#define VAD_THREADS 640           // >= 4 * H
#define VAD_MAXH DSS_VAD_MAXH              // (a multiple of 4)
#define VAD_MAXC DSS_VAD_MAXC
#define VAD_TP 4                  // frames whose input halves (W_ih x) are formed in one pass over W_ih

typedef float vf4 __attribute__((ext_vector_type(4)));
// W streams of a workgroup side by side (W = 1 or 2, chosen per call: one stream per workgroup while that still leaves enough
// workgroups -- a thread's arithmetic per frame is proportional to W)
template <int W> struct VadVec { typedef float type __attribute__((ext_vector_type(W))); };
template <> struct VadVec<1> { struct type { float v; __device__ float &operator[](int) { return v; } __device__ const float &operator[](int) const { return v; } }; };

__device__ __forceinline__ float vad_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// one row of a gate matrix times [n inputs][SW streams] from LDS.  wq: [n / 4][4H][4] -- four consecutive inputs of a
// row side by side, so a lane's load is 16 bytes and a wave's 1 KB of consecutive bytes; n a multiple of 4 (the host pads
// with zero weights, the kernel keeps the padded inputs at zero).  Fused multiply-adds: this operator's reference is torch.
template <int W, typename V>
__device__ __forceinline__ void vad_dot(V &acc, const float *__restrict__ wq, int H4, int row, const V *x, int n)
{
    const vf4 *wr = reinterpret_cast<const vf4 *>(wq) + row;
    int q = 0;
    for (; q + 4 <= n / 4; q += 4) {                       // four 16-byte loads in flight
        vf4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wr[(size_t)(q + u) * H4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const V x0 = x[4 * (q + u)], x1 = x[4 * (q + u) + 1], x2 = x[4 * (q + u) + 2], x3 = x[4 * (q + u) + 3];
#pragma unroll
            for (int s = 0; s < W; ++s) {
                acc[s] = __builtin_fmaf(w[u].x, x0[s], acc[s]);
                acc[s] = __builtin_fmaf(w[u].y, x1[s], acc[s]);
                acc[s] = __builtin_fmaf(w[u].z, x2[s], acc[s]);
                acc[s] = __builtin_fmaf(w[u].w, x3[s], acc[s]);
            }
        }
    }
    for (; q < n / 4; ++q) {
        const vf4 w = wr[(size_t)q * H4];
        const V x0 = x[4 * q], x1 = x[4 * q + 1], x2 = x[4 * q + 2], x3 = x[4 * q + 3];
#pragma unroll
        for (int s = 0; s < W; ++s) {
            acc[s] = __builtin_fmaf(w.x, x0[s], acc[s]);
            acc[s] = __builtin_fmaf(w.y, x1[s], acc[s]);
            acc[s] = __builtin_fmaf(w.z, x2[s], acc[s]);
            acc[s] = __builtin_fmaf(w.w, x3[s], acc[s]);
        }
    }
}

// the input halves of VAD_TP frames' gate rows at once: one pass over W_ih serves VAD_TP frames; acc[tt] accumulates exactly
// the terms, in exactly the order, vad_dot would give frame tt
template <int W, typename V, int XS>
__device__ __forceinline__ void vad_dot_steps(V (&acc)[VAD_TP], const float *__restrict__ wq, int H4, int row, const V (*x)[XS], int n)
{
    const vf4 *wr = reinterpret_cast<const vf4 *>(wq) + row;
    int q = 0;
    for (; q + 4 <= n / 4; q += 4) {
        vf4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wr[(size_t)(q + u) * H4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int tt = 0; tt < VAD_TP; ++tt) {
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
    for (; q < n / 4; ++q) {
        const vf4 w = wr[(size_t)q * H4];
#pragma unroll
        for (int tt = 0; tt < VAD_TP; ++tt) {
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
