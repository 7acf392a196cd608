// csrc/lstm_blocks.h -- the building blocks of the two LSTM operators' kernels, each stated once: the neural detector (vad_lstm.hip:
// inference; vad_train.hip: training) and the bidirectional decoder (bilstm_decoder.hip; dec_train.hip).  One thread per gate row
// over packed weight copies, the inputs of W streams side by side in LDS, the cell update of torch.nn.LSTM (gate order i, f, g, o).
// Functions only: what differs between the operators (threads, capacities, frames per pass) comes in as a template or function
// argument.  Fused multiply-adds are written out (__builtin_fmaf): these operators' reference is torch, and the library is built
// with -ffp-contract=off, so every other product and sum is rounded where it is written.
#pragma once

#include "dss_common.h"
#include "dss_global_ptr.h"

// ---- per operator: threads of a workgroup, capacities, frames whose input halves (W_ih x) are formed in one pass over W_ih -------
#define VAD_THREADS 640           // >= 4 * H
#define VAD_MAXH DSS_VAD_MAXH              // (a multiple of 4)
#define VAD_MAXC DSS_VAD_MAXC
#define VAD_TP 4

#define DEC_THREADS 512           // >= 4 * H and >= W * H
#define DEC_MAXH DSS_DEC_MAXH              // (a multiple of 4)
#define DEC_MAXC DSS_DEC_MAXC              // inputs of a layer: n_inputs for layer 0, 2H above it
#define DEC_TP 4

typedef float f4 __attribute__((ext_vector_type(4)));
// W streams of a workgroup side by side (chosen per call: one stream per workgroup while that still leaves enough workgroups -- a
// thread's arithmetic per frame is proportional to W)
template <int W> struct LstmVec { typedef float type __attribute__((ext_vector_type(W))); };
template <> struct LstmVec<1> { struct type { float v; __device__ float &operator[](int) { return v; } __device__ const float &operator[](int) const { return v; } }; };

__device__ __forceinline__ float lstm_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// The packed copy of a gate matrix: [inputs / 4][4H rows][4 consecutive inputs] -- four consecutive inputs of a row side by side,
// so a lane's load is 16 bytes and a wave's 1 KB of consecutive bytes.  Element (input k, row r); W_hh's inputs stand behind
// W_ih's, whose count is padded to a multiple of 4 (zero weights; the kernels keep the padded inputs at zero).  The host loaders
// (dss_pack_rows) and the training kernels' update of the copy both index through here.
__host__ __device__ inline size_t lstm_packed_index(int k, int r, int H4) { return ((size_t)(k >> 2) * H4 + r) * 4 + (k & 3); }

// acc[s] += w.x x0[s] + .. + w.w x3[s], in that order
template <int W, typename V>
__device__ __forceinline__ void lstm_fma4(V &acc, const f4 w, const V x0, const V x1, const V x2, const V x3)
{
#pragma unroll
    for (int s = 0; s < W; ++s) {
        acc[s] = __builtin_fmaf(w.x, x0[s], acc[s]);
        acc[s] = __builtin_fmaf(w.y, x1[s], acc[s]);
        acc[s] = __builtin_fmaf(w.z, x2[s], acc[s]);
        acc[s] = __builtin_fmaf(w.w, x3[s], acc[s]);
    }
}

// one row of a packed gate matrix times [n inputs][W streams] from LDS; n a multiple of 4
template <int W, typename V>
__device__ __forceinline__ void lstm_dot(V &acc, const float *__restrict__ wq, int H4, int row, const V *x, int n)
{
    const f4 *wr = reinterpret_cast<const f4 *>(wq) + row;
    int q = 0;
    for (; q + 4 <= n / 4; q += 4) {                       // four 16-byte loads in flight
        f4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wr[(size_t)(q + u) * H4];
#pragma unroll
        for (int u = 0; u < 4; ++u) lstm_fma4<W>(acc, w[u], x[4 * (q + u)], x[4 * (q + u) + 1], x[4 * (q + u) + 2], x[4 * (q + u) + 3]);
    }
    for (; q < n / 4; ++q) lstm_fma4<W>(acc, wr[(size_t)q * H4], x[4 * q], x[4 * q + 1], x[4 * q + 2], x[4 * q + 3]);
}

// the input halves of TP frames' gate rows at once: one pass over W_ih (n / 4 sixteen-byte loads per thread) serves TP frames;
// acc[tt] accumulates exactly the terms, in exactly the order, lstm_dot would give frame tt
template <int W, typename V, int XS, int TP>
__device__ __forceinline__ void lstm_dot_steps(V (&acc)[TP], const float *__restrict__ wq, int H4, int row, const V (*x)[XS], int n)
{
    const f4 *wr = reinterpret_cast<const f4 *>(wq) + row;
    int q = 0;
    for (; q + 4 <= n / 4; q += 4) {
        f4 w[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) w[u] = wr[(size_t)(q + u) * H4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
#pragma unroll
            for (int tt = 0; tt < TP; ++tt)
                lstm_fma4<W>(acc[tt], w[u], x[tt][4 * (q + u)], x[tt][4 * (q + u) + 1], x[tt][4 * (q + u) + 2], x[tt][4 * (q + u) + 3]);
    }
    for (; q < n / 4; ++q) {
        const f4 w = wr[(size_t)q * H4];
#pragma unroll
        for (int tt = 0; tt < TP; ++tt) lstm_fma4<W>(acc[tt], w, x[tt][4 * q], x[tt][4 * q + 1], x[tt][4 * q + 2], x[tt][4 * q + 3]);
    }
}

// A thread's row of W_hh (whh: the packed copy from its first recurrent input on) into registers for all steps: MAXH values, zero
// beyond Hp and in threads that own no row.  A step's recurrent half then costs LDS reads of h and arithmetic only -- with the row
// streamed from L2 every step, L2 latency set the step time.
template <int MAXH>
__device__ __forceinline__ void lstm_load_row(f4 (&w)[MAXH / 4], const float *__restrict__ whh, int H4, int row, bool rowt, int Hp)
{
    const f4 *wr = reinterpret_cast<const f4 *>(whh) + (rowt ? row : 0);
#pragma unroll
    for (int q = 0; q < MAXH / 4; ++q) w[q] = (rowt && 4 * q < Hp) ? wr[(size_t)q * H4] : (f4){0.f, 0.f, 0.f, 0.f};
}

// the recurrent half from those registers: the terms and the order of lstm_dot over the same row
template <int W, typename V, int MAXH>
__device__ __forceinline__ void lstm_dot_row(V &acc, const f4 (&w)[MAXH / 4], const V *h, int Hp)
{
#pragma unroll
    for (int q = 0; q < MAXH / 4; ++q) {
        if (4 * q >= Hp) break;
        lstm_fma4<W>(acc, w[q], h[4 * q], h[4 * q + 1], h[4 * q + 2], h[4 * q + 3]);
    }
}

// The cell update from a unit's four gate pre-activations: c' = f c + i g, returns h' = o tanh(c'); i, f, g, o come back activated
// (training stashes them; inference lets them go).
__device__ __forceinline__ float lstm_cell(float &gi, float &gf, float &gg, float &go, float &c)
{
    gi = lstm_sigmoid(gi); gf = lstm_sigmoid(gf); gg = tanhf(gg); go = lstm_sigmoid(go);
    c = gf * c + gi * gg;
    return go * tanhf(c);
}

// ---- training: the step kernels (a workgroup per gate row, or per row of the head) ----------------------------------------------

// torch.optim.RMSprop on element k: sq <- alpha sq + (1 - alpha) g^2;  p <- p - lr g / (sqrt(sq) + eps), each evaluated in float64
// from the stored float32 values and rounded once.  Stores the gradient; returns the parameter's new value (apply == 0: its value).
__device__ __forceinline__ float lstm_rmsprop(float *p, float *sq, float *g, int k, float grad, int apply, double lr, double alpha, double eps)
{
    g[k] = grad;
    if (!apply) return p[k];
    const float s = (float)(alpha * (double)sq[k] + (1.0 - alpha) * ((double)grad * (double)grad));
    sq[k] = s;
    const float v = (float)((double)p[k] - lr * (double)grad / (sqrt((double)s) + eps));
    p[k] = v;
    return v;
}

// What a step kernel's workgroup works on: one row of [A columns | B columns | bias] against the row's gradient per frame.
// Gate row r of a layer: A = its W_ih row (the layer's inputs), B = its W_hh row (the layer's own h of the step before), two biases
// (bias_ih and bias_hh get the same gradient and each its own square average; the packed bias is their float32 sum), and the packed
// copy.  A row of the head: A only, one bias, no packed copy (wpk == NULL).
struct LstmStepRow {
    const float *dg; int dgs;                  // the row's gradient at frame t: dg[t * dgs]
    const float *inA; int nA;                  // column k < nA reads inA[t * nA + k]
    const float *inB; int nB; long strideB;    // column nA + k reads inB[t * strideB + k] (the decoder's backward direction: < 0)
    int o_A, o_B, o_bias, o_bias2;             // flat offsets of the row's first A element, first B element and bias(es)
    float *wpk, *bpk; int r, H4, kB;           // packed copy, this row's packed bias, row, rows, packed input index of B's column 0
};

// Column k's gradient is the sum over the frames t = 0 .. T-1, IN THAT ORDER, of dg[t] in[t][k] (one fused multiply-add per frame; the
// bias adds dg[t] itself): tiles of THREADS frames of dg go through LDS, a thread owns columns tid and tid + THREADS.  Then, fused,
// the update of the master parameters (p, sq, g: flat, torch layout) and of the packed copies the forward pass reads.
template <int THREADS>
__device__ __forceinline__ void lstm_train_step_row(const LstmStepRow &w, float *p, float *sq, float *g, const int T, const int apply,
                                                    const double lr, const double alpha, const double eps)
{
    __shared__ float dgt[THREADS];
    const int tid = threadIdx.x, ncol = w.nA + w.nB + 1;
    const float *src[2];
    long stride[2];
    int col[2];
    bool live[2], bias[2];
    float acc[2] = {0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        col[u] = tid + u * THREADS;
        live[u] = col[u] < ncol;
        bias[u] = col[u] == ncol - 1;
        if (!live[u] || bias[u]) { src[u] = w.inA; stride[u] = 0; }
        else if (col[u] < w.nA) { src[u] = w.inA + col[u]; stride[u] = w.nA; }
        else { src[u] = w.inB + (col[u] - w.nA); stride[u] = w.strideB; }
    }
    for (int t0 = 0; t0 < T; t0 += THREADS) {
        const int n = min(THREADS, T - t0);
        if (tid < n) dgt[tid] = w.dg[(size_t)(t0 + tid) * w.dgs];
        __syncthreads();
        for (int tt = 0; tt < n; ++tt) {
            const float gt = dgt[tt];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float x = bias[u] ? 1.f : dss_gp(src[u])[(long)(t0 + tt) * stride[u]];
                acc[u] = __builtin_fmaf(gt, x, acc[u]);
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
        if (!live[u]) continue;
        const int k = col[u];
        if (bias[u]) {
            const float bi = lstm_rmsprop(p, sq, g, w.o_bias, acc[u], apply, lr, alpha, eps);
            if (!w.wpk) continue;
            const float bh = lstm_rmsprop(p, sq, g, w.o_bias2, acc[u], apply, lr, alpha, eps);
            if (apply) *w.bpk = bi + bh;
        } else {
            const bool a = k < w.nA;
            const float v = lstm_rmsprop(p, sq, g, a ? w.o_A + k : w.o_B + (k - w.nA), acc[u], apply, lr, alpha, eps);
            if (w.wpk && apply) w.wpk[lstm_packed_index(a ? k : w.kB + (k - w.nA), w.r, w.H4)] = v;
        }
    }
}
