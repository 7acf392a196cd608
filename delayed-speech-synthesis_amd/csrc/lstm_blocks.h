// csrc/lstm_blocks.h -- the building blocks of the two LSTM operators' kernels, each stated once: the neural detector (vad_lstm.hip:
// inference; vad_train.hip: training) and the bidirectional decoder (bilstm_decoder.hip; dec_train.hip).  One thread per gate row
// over packed weight copies, the inputs of W streams side by side in LDS, the cell update of torch.nn.LSTM (gate order i, f, g, o).
// On top of the blocks, the loops that every kernel of an operator runs: the decoder's layer loop (bilstm_layer_body) and regressor
// (dec_regress_rows), the detector's forward loop (vad_forward_body).  Inference and training differ in what they keep of a
// step, which the caller hands in as a function object.
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

// what an operator's kernels can hold: every launcher asks here
static inline bool vad_fits(int C, int H) { return H >= 1 && H <= VAD_MAXH && 4 * H <= VAD_THREADS && C >= 1 && C <= VAD_MAXC; }
static inline bool dec_fits(int C, int H) { return H >= 1 && H <= DEC_MAXH && 4 * H <= DEC_THREADS && C >= 1 && C <= DEC_MAXC && 2 * H <= DEC_MAXC; }

// ---- the decoder's layer loop ----------------------------------------------------------------------------------------------------
// One layer, one workgroup: W streams of one direction `dir` through the layer whose packed weights are wT and whose summed biases
// are bias_v.  Every kernel that steps a decoder layer runs this body (bilstm_decoder.hip: the plain and the group inference form;
// dec_train.hip: the trainers' forward half, W = 1), so a stream's bits do not depend on which of them stepped it.  Where a
// stream's frames lie is the caller's: stream(sl, Ts, irow, orow) gives stream sl of the workgroup (0 <= sl < W) its Ts frames (0:
// the slot is empty), the row of `in` that holds its frame 0 and the row of the output that takes it; frame t is row + t in both.
// A stream's backward direction starts at its OWN last frame, and nothing is computed or written beyond it.  What is kept is the
// caller's too: loaded(row, k, x) sees input k of input row `row` as it goes to LDS, and the owner of a cell calls
// cell(step, row, unit, i, f, g, o, c, h) after lstm_cell with the step, the frame's output row and the activated gates.
template <typename InT, int W, typename StreamFn, typename LoadFn, typename CellFn>
__device__ __forceinline__ void bilstm_layer_body(const InT *__restrict__ in, const int Cin, const int H, const float *__restrict__ wT,
                                                  const float *__restrict__ bias_v, const int dir, StreamFn stream, LoadFn loaded, CellFn cell)
{
    typedef typename LstmVec<W>::type V;
    __shared__ __attribute__((aligned(16))) V xin[DEC_TP][DEC_MAXC];      // [step of the chunk][input][stream of this workgroup]
    __shared__ __attribute__((aligned(16))) V hs[DEC_MAXH];               // [unit][stream]; units H .. Hp-1 stay zero
    __shared__ __attribute__((aligned(16))) V gates[4 * DEC_MAXH];        // [gate row][stream]
    const int tid = threadIdx.x, H4 = 4 * H;
    const int Cp = (Cin + 3) & ~3, Hp = (H + 3) & ~3;      // the padded input counts the weight copies were built for
    const int cs = W == 1 ? 0 : tid / H, cu = tid - cs * H;       // the (stream, unit) this thread owns in the cell updates
    int Tc = 0;                                            // frames of the stream this thread's cell belongs to
    size_t oc = 0;                                         //   and its first output row
    if (tid < W * H) { size_t ic; stream(cs, Tc, ic, oc); }
    __shared__ int Tsh[W];                                 // per stream of this workgroup: frames, first input row
    __shared__ size_t Rsh[W];
    if (tid < W) {
        int Ts; size_t ir, orow;
        stream(tid, Ts, ir, orow);
        Tsh[tid] = Ts; Rsh[tid] = ir;
    }
    float c = 0.f;                                         // create_new_initial_state: zeros (models.py:22-24)
    for (int k = tid; k < DEC_MAXH * W; k += DEC_THREADS) reinterpret_cast<float *>(hs)[k] = 0.f;
    for (int k = tid; k < DEC_TP * DEC_MAXC * W; k += DEC_THREADS) reinterpret_cast<float *>(xin)[k] = 0.f;
    const bool rowt = tid < H4;
    const float bias = rowt ? bias_v[tid] : 0.f;
    // this thread's row of W_hh stays in its registers for all steps (DEC_MAXH values, zero beyond H): a step's recurrent half
    // then costs LDS reads of h and arithmetic only -- with the row streamed from L2 every step, L2 latency set the step time
    f4 whh[DEC_MAXH / 4];
    lstm_load_row<DEC_MAXH>(whh, wT + (size_t)Cp * H4, H4, tid, rowt, Hp);
    __syncthreads();
    int Tw = 0;                                            // the longest of this workgroup's streams
#pragma unroll
    for (int sl = 0; sl < W; ++sl) Tw = max(Tw, Tsh[sl]);
    // The recurrence is serial in time, the input halves of the gates are not: per chunk of DEC_TP steps one pass over W_ih forms
    // them for all its steps (each gets the same terms in the same order as a step on its own), and a step then adds only W_hh h.
    for (int step0 = 0; step0 < Tw; step0 += DEC_TP) {
        const int nst = min(DEC_TP, Tw - step0);
        for (int idx = tid; idx < nst * Cin * W; idx += DEC_THREADS) {
            const int tt = idx / (Cin * W), rem = idx - tt * (Cin * W);
            const int sl = W == 1 ? 0 : rem / Cin, k = rem - sl * Cin;
            const int Ts = Tsh[sl], step = step0 + tt;
            const size_t row = Rsh[sl] + (dir ? Ts - 1 - step : step);
            const float x = step < Ts ? (float)in[row * Cin + k] : 0.f;
            reinterpret_cast<float *>(&xin[tt][k])[sl] = x;
            if (step < Ts) loaded(row, k, x);
        }
        __syncthreads();
        V pre[DEC_TP];
#pragma unroll
        for (int tt = 0; tt < DEC_TP; ++tt)
#pragma unroll
            for (int s = 0; s < W; ++s) pre[tt][s] = 0.f;
        if (rowt) lstm_dot_steps<W, V, DEC_MAXC, DEC_TP>(pre, wT, H4, tid, xin, Cp);        // (steps beyond nst: stale inputs, never used)
#pragma unroll
        for (int tt = 0; tt < DEC_TP; ++tt) {
            if (tt >= nst) break;
            const int step = step0 + tt;
            if (rowt) {                                    // gate pre-activations: W_ih x + W_hh h + (b_ih + b_hh)
                V acc = pre[tt];
                lstm_dot_row<W, V, DEC_MAXH>(acc, whh, hs, Hp);
#pragma unroll
                for (int s = 0; s < W; ++s) acc[s] += bias;
                gates[tid] = acc;
            }
            __syncthreads();
            if (tid < W * H && step < Tc) {                // cell update of (stream cs, unit cu)
                float gi = reinterpret_cast<const float *>(&gates[cu])[cs];
                float gf = reinterpret_cast<const float *>(&gates[H + cu])[cs];
                float gg = reinterpret_cast<const float *>(&gates[2 * H + cu])[cs];
                float go = reinterpret_cast<const float *>(&gates[3 * H + cu])[cs];
                const float h = lstm_cell(gi, gf, gg, go, c);
                reinterpret_cast<float *>(&hs[cu])[cs] = h;        // (what the direction carries to its own next step)
                cell(step, oc + (dir ? Tc - 1 - step : step), cu, gi, gf, gg, go, c, h);
            }
            __syncthreads();
        }
    }
}

// ---- the decoder's regressor (models.py:45,57) ---------------------------------------------------------------------------------
// value[row][o] = b[o] + sum_k w[o][k] top[row][k] for the DEC_RROWS rows of a 256-thread block: the whole weight matrix and the
// rows' inputs go through LDS once (one thread per (row, output) reading both from global memory took 29 us for 512 rows: 200
// strided loads in series per thread).  rs: dec_regress_lds_floats(K, O) floats of LDS, [O][K + 1] weights, then [DEC_RROWS][K]
// inputs.  Which rows there are is the caller's: row(rr) is row rr's K inputs, or NULL for a row that does not exist; and so is
// where a value goes: put(rr, o, value) is called once per live (row, output).  Four kernels run this body (bilstm_decoder.hip's
// three regressors; dec_train.hip's head), so a row's features are the same bits in all of them.
#define DEC_RROWS 8
static_assert(DEC_RROWS == DSS_DEC_RROWS, "the host deals the group form's blocks (dss_dec_group.cpp)");
__host__ __device__ inline size_t dec_regress_lds_floats(int K, int O) { return (size_t)O * (K + 1) + (size_t)DEC_RROWS * K; }

template <typename RowFn, typename PutFn>
__device__ __forceinline__ void dec_regress_rows(float *rs, const int K, const int O, const float *__restrict__ w, const float *__restrict__ b,
                                                 RowFn row, PutFn put)
{
    float *ws = rs, *xs = rs + (size_t)O * (K + 1);
    const int tid = threadIdx.x;
    for (int k = tid; k < O * K; k += 256) { const int o = k / K, j = k - o * K; ws[o * (K + 1) + j] = w[k]; }
    for (int k = tid; k < DEC_RROWS * K; k += 256) {
        const int rr = k / K;
        const float *x = row(rr);
        xs[k] = x ? x[k - rr * K] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < DEC_RROWS * O; idx += 256) {
        const int rr = idx / O, o = idx - rr * O;
        if (!row(rr)) continue;
        const float *x = xs + rr * K, *wr = ws + o * (K + 1);
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = __builtin_fmaf(wr[k], x[k], a);
        put(rr, o, a + b[o]);
    }
}

// ---- the detector's forward loop -------------------------------------------------------------------------------------------------
// The forward pass of one workgroup: SW streams, W frames each, through both layers and the classifier.  Stream s of the call
// (s0 <= s < min(s0 + SW, S)) reads frames[(s * W + w) * C ..] and writes, unless logits is NULL, logits[(s * W + w) * 2 ..] and,
// where LABELS is set, labels[s * W + w] (otherwise the labels, their LDS and their barrier are not compiled).  CARRY: (h, c) of
// both layers come from the handle and go back to it; otherwise the streams start from zeros (create_new_initial_state,
// models.py:22-24) and the handle's state is not touched.  Every kernel that steps a detector runs this body (vad_lstm.hip: the
// streaming, the trial-list and the group form; vad_train.hip: the trainers' forward half, SW = 1), so a frame's bits do not
// depend on which of them stepped it.  What is kept is the caller's: loaded(stream, w, k, x) sees input k of frame w as it goes to
// LDS, and the owner of a cell calls cell(layer, stream, w, unit, i, f, g, o, c, h) after lstm_cell with the activated gates; what
// it returns for layer 0 is what layer 1 reads as that unit's input (inference: h; training: h times the dropout mask).
// A caller that loads the descriptor from a device table hands in vad_global_dev's copy of it.
__device__ __forceinline__ DssVadDev vad_global_dev(const DssVadDev &t)       // the pointers as global pointers (dss_gp)
{
    DssVadDev v;
    v.S = 1; v.C = t.C; v.H = t.H;
    v.wT0 = dss_gp(t.wT0); v.b0 = dss_gp(t.b0); v.wT1 = dss_gp(t.wT1); v.b1 = dss_gp(t.b1); v.wc = dss_gp(t.wc); v.bc = dss_gp(t.bc);
    v.h = dss_gp(t.h); v.c = dss_gp(t.c);
    return v;
}

template <typename FrameT, int SW, bool CARRY, bool LABELS, typename LoadFn, typename CellFn>
__device__ __forceinline__ void vad_forward_body(const DssVadDev &v, const FrameT *__restrict__ frames, const int W, int *__restrict__ labels,
                                                 float *__restrict__ logits, const int s0, const int S, LoadFn loaded, CellFn cell)
{
    typedef typename LstmVec<SW>::type V;
    __shared__ __attribute__((aligned(16))) V xin[VAD_TP][VAD_MAXC];      // [frame of the chunk][input][stream of this workgroup]
    __shared__ __attribute__((aligned(16))) V h0s[VAD_TP][VAD_MAXH];      // layer 1's inputs: what cell() returned for layer 0
    __shared__ __attribute__((aligned(16))) V hs[2][VAD_MAXH];            // [layer][unit][stream]: the h a layer carries to its own next
                                                                          //   step; units H .. Hp-1 stay zero
    __shared__ __attribute__((aligned(16))) V gates[4 * VAD_MAXH];        // [gate row][stream]
    __shared__ float lg[SW][2];                                           // (LABELS only)
    const int tid = threadIdx.x, C = v.C, H = v.H, H4 = 4 * H;
    const int Cp = (C + 3) & ~3, Hp = (H + 3) & ~3;        // the padded input counts the weight copies were built for
    // the (stream, unit) this thread owns in the cell updates
    const int cs = SW == 1 ? 0 : tid / H, cu = tid - cs * H;
    const bool own = tid < SW * H && s0 + cs < S;
    float c0 = 0.f, c1 = 0.f;
    for (int k = tid; k < 2 * VAD_MAXH * SW; k += VAD_THREADS) reinterpret_cast<float *>(hs)[k] = 0.f;
    for (int k = tid; k < VAD_TP * VAD_MAXH * SW; k += VAD_THREADS) reinterpret_cast<float *>(h0s)[k] = 0.f;
    for (int k = tid; k < VAD_TP * VAD_MAXC * SW; k += VAD_THREADS) reinterpret_cast<float *>(xin)[k] = 0.f;
    __syncthreads();
    if (CARRY && own) {
        const size_t o = (size_t)(s0 + cs) * H + cu;
        reinterpret_cast<float *>(&hs[0][cu])[cs] = v.h[o];
        reinterpret_cast<float *>(&hs[1][cu])[cs] = v.h[(size_t)S * H + o];
        c0 = v.c[o]; c1 = v.c[(size_t)S * H + o];
    }
    const bool rowt = tid < H4;
    const float bias0 = rowt ? v.b0[tid] : 0.f, bias1 = rowt ? v.b1[tid] : 0.f;

    // Layer by layer over chunks of VAD_TP frames: a layer's recurrence is serial in time, the input halves of its gates are not --
    // one pass over W_ih forms them for all frames of the chunk (each gets the same terms in the same order as a frame on its
    // own), and a step then adds only W_hh h.  Layer 1's inputs are layer 0's outputs of the chunk's frames (h0s).
    for (int w0 = 0; w0 < W; w0 += VAD_TP) {
        const int nst = min(VAD_TP, W - w0);
        for (int idx = tid; idx < nst * C * SW; idx += VAD_THREADS) {       // the chunk's inputs (units.py:433: frames as float32)
            const int tt = idx / (C * SW), rem = idx - tt * (C * SW);
            const int sl = rem / C, k = rem - sl * C;
            const float x = (s0 + sl < S) ? (float)frames[((size_t)(s0 + sl) * W + w0 + tt) * C + k] : 0.f;
            reinterpret_cast<float *>(&xin[tt][k])[sl] = x;
            if (s0 + sl < S) loaded(sl, w0 + tt, k, x);
        }
        __syncthreads();
#pragma unroll
        for (int layer = 0; layer < 2; ++layer) {
            V pre[VAD_TP];
#pragma unroll
            for (int tt = 0; tt < VAD_TP; ++tt)
#pragma unroll
                for (int s = 0; s < SW; ++s) pre[tt][s] = 0.f;
            if (rowt) {                                    // (frames beyond nst: stale inputs, never used)
                if (layer == 0) lstm_dot_steps<SW, V, VAD_MAXC, VAD_TP>(pre, v.wT0, H4, tid, xin, Cp);
                else lstm_dot_steps<SW, V, VAD_MAXH, VAD_TP>(pre, v.wT1, H4, tid, h0s, Hp);
            }
#pragma unroll
            for (int tt = 0; tt < VAD_TP; ++tt) {
                if (tt >= nst) break;
                const int w = w0 + tt;
                // ---- gate pre-activations of this layer and frame: W_ih x + W_hh h + (b_ih + b_hh)
                if (rowt) {
                    V acc = pre[tt];
                    if (layer == 0) lstm_dot<SW, V>(acc, v.wT0 + (size_t)Cp * H4, H4, tid, hs[0], Hp);
                    else lstm_dot<SW, V>(acc, v.wT1 + (size_t)Hp * H4, H4, tid, hs[1], Hp);
#pragma unroll
                    for (int s = 0; s < SW; ++s) acc[s] += layer == 0 ? bias0 : bias1;
                    gates[tid] = acc;
                }
                __syncthreads();
                // ---- cell update of (stream cs, unit cu)
                if (tid < SW * H) {
                    float gi = reinterpret_cast<const float *>(&gates[cu])[cs];
                    float gf = reinterpret_cast<const float *>(&gates[H + cu])[cs];
                    float gg = reinterpret_cast<const float *>(&gates[2 * H + cu])[cs];
                    float go = reinterpret_cast<const float *>(&gates[3 * H + cu])[cs];
                    float &c = layer == 0 ? c0 : c1;
                    const float h = lstm_cell(gi, gf, gg, go, c);
                    reinterpret_cast<float *>(&hs[layer][cu])[cs] = h;
                    const float down = cell(layer, cs, w, cu, gi, gf, gg, go, c, h);
                    if (layer == 0) reinterpret_cast<float *>(&h0s[tt][cu])[cs] = down;
                }
                __syncthreads();
                if (layer == 1) {
                    // ---- classifier (models.py:20,32) and the raw label (units.py:434: argmax, the first maximum wins: equal
                    // logits are non-speech).  Without labels nothing waits here: the next step writes hs[1] only behind its own
                    // first barrier.
                    if (tid < SW * 2) {
                        const int sl = tid >> 1, cls = tid & 1;
                        float a = 0.f;
                        for (int k = 0; k < H; ++k) a = __builtin_fmaf(v.wc[cls * H + k], reinterpret_cast<const float *>(&hs[1][k])[sl], a);
                        a += v.bc[cls];
                        if constexpr (LABELS) lg[sl][cls] = a;
                        if ((!LABELS || logits) && s0 + sl < S) logits[((size_t)(s0 + sl) * W + w) * 2 + cls] = a;
                    }
                    if constexpr (LABELS) {
                        __syncthreads();
                        if (tid < SW && s0 + tid < S) labels[(size_t)(s0 + tid) * W + w] = lg[tid][1] > lg[tid][0] ? 1 : 0;
                    }
                }
            }
        }
    }
    if (CARRY && own) {
        const size_t o = (size_t)(s0 + cs) * H + cu;
        v.h[o] = reinterpret_cast<const float *>(&hs[0][cu])[cs];
        v.h[(size_t)S * H + o] = reinterpret_cast<const float *>(&hs[1][cu])[cs];
        v.c[o] = c0;
        v.c[(size_t)S * H + o] = c1;
    }
}

// ---- scoring ----------------------------------------------------------------------------------------------------------------------
// nn.CrossEntropyLoss of one frame of two classes, in float64 from the float32 logits: logsumexp(z) - z[target]; lse comes back
// too (softmax(z)[k] = exp(z[k] - lse)).
__device__ __forceinline__ double lstm_cross_entropy(const double z0, const double z1, const int target, double &lse)
{
    const double m = fmax(z0, z1);
    lse = m + log(exp(z0 - m) + exp(z1 - m));
    return lse - (target ? z1 : z0);
}

// the first row of trial k of a launch's trial list in the concatenated arrays
__device__ __forceinline__ long long dss_trial_row(const DssTrialLens &tl, const int k)
{
    long long off = tl.base;
    for (int j = 0; j < k; ++j) off += tl.len[j];
    return off;
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
