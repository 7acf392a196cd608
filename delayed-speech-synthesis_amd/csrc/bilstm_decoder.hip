// csrc/bilstm_decoder.hip -- the bidirectional recurrent decoder of the online path for many streams per launch (gfx950).
//
// Restates, for S independent streams and the T high-gamma frames of a call (one amplifier packet = 4 frames in the streaming
// mode, a whole segment otherwise),
//   BidirectionalSpeechSynthesisModel.forward       local/models.py:36-58   LSTM(C -> H, 2 layers, bidirectional) -> Linear(2H -> 20)
//   DecodingModel.process, the model call           local/units.py:499-508  frames as float32, a fresh zero state per call
// The reference runs torch.nn.LSTM; its arithmetic is torch's, not a fixed C sequence, so parity here is tolerance-level like
// the detector's (vad_lstm.hip): the test states it (|feature - torch| <= 2e-5 on the reference-generated golden vector) and
// fused multiply-adds are allowed.  Gate order i, f, g, o (torch.nn.LSTM); a layer's input at frame t is
// [h_forward(t), h_backward(t)] of the layer below.
//
// Three launches per call instead of MIOpen's ~20: one per layer -- its two directions are independent and run as separate
// workgroups (blockIdx.y) -- and the regressor.  A 512-thread workgroup owns W streams (1, 2 or 4: as few as keeps every CU busy) and one direction for all T steps;
// thread t owns gate row t (4H <= 512 rows) and runs the row's dot product for the W streams at once: the weights
// (copies with four consecutive inputs of a row side by side: one 16-byte load per lane, 1 KB of consecutive bytes per wave)
// of the input half come from L2 once per workgroup and chunk of DEC_TP steps, the row of W_hh stays in the thread's registers
// for the whole call, the inputs come from LDS as broadcast reads; h lives in LDS, c in the registers of the thread that owns
// (stream, unit).  Time steps are sequential; streams x gate rows x directions are the parallel axes.
#include "lstm_blocks.h"

// One layer, one workgroup: W streams of one direction `dir` through the layer whose packed weights are wT and whose summed biases
// are bias_v; forward h goes to columns [0, H) of a row of out, backward h to [H, 2H).  Two kernels run this body (below, and the
// group form at the end of this file), so a stream's bits do not depend on which of them stepped it.  Where a stream's frames lie
// is the caller's: stream(sl, Ts, irow, orow) gives stream sl of the workgroup (0 <= sl < W) its Ts frames (0: the slot is empty),
// the row of `in` that holds its frame 0 and the row of `out` that takes it; frame t is row + t in both.  A stream's backward
// direction starts at its OWN last frame, and nothing is computed or written beyond it.
template <typename InT, int W, typename StreamFn>
__device__ __forceinline__ void bilstm_layer_body(const InT *__restrict__ in, const int Cin, const int H, const float *__restrict__ wT,
                                                  const float *__restrict__ bias_v, const int dir, float *__restrict__ out, StreamFn stream)
{
    typedef typename LstmVec<W>::type V;
    __shared__ __attribute__((aligned(16))) V xin[DEC_TP][DEC_MAXC];      // [step of the chunk][input][stream of this workgroup]
    __shared__ __attribute__((aligned(16))) V hs[DEC_MAXH];               // [unit][stream]; units H .. Hp-1 stay zero
    __shared__ __attribute__((aligned(16))) V gates[4 * DEC_MAXH];        // [gate row][stream]
    const int tid = threadIdx.x, H4 = 4 * H;
    const int Cp = (Cin + 3) & ~3, Hp = (H + 3) & ~3;      // the padded input counts the weight copies were built for
    const int cs = tid / H, cu = tid - cs * H;             // the (stream, unit) this thread owns in the cell updates
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
            const int sl = rem / Cin, k = rem - sl * Cin;
            const int Ts = Tsh[sl], step = step0 + tt;
            const int t = dir ? Ts - 1 - step : step;
            reinterpret_cast<float *>(&xin[tt][k])[sl] = step < Ts ? (float)in[(Rsh[sl] + t) * Cin + k] : 0.f;
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
                reinterpret_cast<float *>(&hs[cu])[cs] = h;
                out[(oc + (dir ? Tc - 1 - step : step)) * (2 * H) + dir * H + cu] = h;
            }
            __syncthreads();
        }
    }
}

// One layer, both directions (blockIdx.y): in (S, T, Cin) -> out (S, T, 2H).
// Ragged form (segments of different lengths in one call, dss_dec_forward_rows_dev): stream s has counts[s] <= T frames (NULL:
// T) and its input frames are row in_row[s] (NULL: s) of a buffer with Tin frames per row (a pool of segment buffers).
template <typename InT, int W>
__global__ void __launch_bounds__(DEC_THREADS)
bilstm_layer_kernel(const InT *__restrict__ in, int S, int T, int Cin, int H, const float *__restrict__ wT_f,
                    const float *__restrict__ wT_b, const float *__restrict__ b_f, const float *__restrict__ b_b,
                    float *__restrict__ out, const int *__restrict__ counts, const int *__restrict__ in_row, int Tin)
{
    const int dir = blockIdx.y, s0 = blockIdx.x * W;
    bilstm_layer_body<InT, W>(in, Cin, H, dir ? wT_b : wT_f, dir ? b_b : b_f, dir, out, [&](int sl, int &Ts, size_t &irow, size_t &orow) {
        const int s = s0 + sl;
        const bool live = s < S;
        Ts = live ? (counts ? min(counts[s], T) : T) : 0;
        irow = live ? (size_t)(in_row ? in_row[s] : s) * Tin : 0;
        orow = (size_t)s * T;
    });
}

// regressor (models.py:45,57): feats[row][o] = b[o] + sum_k w[o][k] top[row][k], row = (stream, frame).  A block takes
// DEC_RROWS rows: their inputs and the whole weight matrix go through LDS once (one thread per (row, output) reading both
// from global memory took 29 us for 512 rows: 200 strided loads in series per thread).
#define DEC_RROWS 8
static_assert(DEC_RROWS == DSS_DEC_RROWS, "the host deals the group form's blocks (dss_dec_group.cpp)");
__global__ void __launch_bounds__(256)
dec_regress_kernel(const float *__restrict__ top, long rows, int K, int O, const float *__restrict__ w, const float *__restrict__ b,
                   float *__restrict__ feats, const int *__restrict__ counts, int T)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];             // [O][K + 1] weights, then [DEC_RROWS][K] inputs
    float *ws = rs, *xs = rs + (size_t)O * (K + 1);
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * DEC_RROWS;
    for (int k = tid; k < O * K; k += 256) { const int o = k / K, j = k - o * K; ws[o * (K + 1) + j] = w[k]; }
    // ragged calls: row r = (stream r / T, frame r % T) exists only below its stream's frame count
    auto live = [&](long r) { return r < rows && (!counts || (int)(r % T) < counts[r / T]); };
    for (int k = tid; k < DEC_RROWS * K; k += 256) {
        const long r = r0 + k / K;
        xs[k] = live(r) ? top[r * K + (k % K)] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < DEC_RROWS * O; idx += 256) {
        const int rr = idx / O, o = idx - rr * O;
        if (!live(r0 + rr)) continue;
        const float *x = xs + rr * K, *wr = ws + o * (K + 1);
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = __builtin_fmaf(wr[k], x[k], a);
        feats[(r0 + rr) * O + o] = a + b[o];
    }
}

int dss_launch_decoder(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, float *d_feats,
                       const int *d_counts, const int *d_in_row, int Tin, hipStream_t st)
{
    if (Tin <= 0) Tin = T;                                 // plain calls: the input is (S, T, C)
    if (d.H < 1 || d.H > DEC_MAXH || 4 * d.H > DEC_THREADS || d.C < 1 || d.C > DEC_MAXC || 2 * d.H > DEC_MAXC) {
        dss_set_error("decoder kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", d.H, d.C, DEC_MAXH, DEC_MAXC);
        return DSS_EINVAL;
    }
    if (d.O < 1 || d.O > 32) { dss_set_error("decoder kernel: %d outputs out of range (<= 32)", d.O); return DSS_EINVAL; }
    if (S < 1 || S > d.S_max || T < 1 || T > d.T_max) {
        dss_set_error("decoder kernel: %d streams x %d frames exceed the handle's %d x %d", S, T, d.S_max, d.T_max);
        return DSS_EINVAL;
    }
    // streams per workgroup: a thread's work per step grows with W, the number of workgroups shrinks with it; 2 x S / W of
    // them should still cover the CUs (64 streams: 128 workgroups of one stream; 1024 streams: 512 of four)
    const int Wsel = 2 * S <= 256 ? 1 : (S <= 256 ? 2 : 4);
    const dim3 block(DEC_THREADS);
#define DEC_LAUNCH(INT, WV, IN, CIN, L, OUT)                                                                                   \
    hipLaunchKernelGGL((bilstm_layer_kernel<INT, WV>), dim3((S + WV - 1) / WV, 2), block, 0, st, (const INT *)(IN), S, T, CIN, d.H,  \
                       d.wT[L][0], d.wT[L][1], d.b[L][0], d.b[L][1], OUT, d_counts, (L) == 0 ? d_in_row : (const int *)nullptr,   \
                       (L) == 0 ? Tin : T)
#define DEC_LAUNCH_W(INT, IN, CIN, L, OUT)                                                                                      \
    do {                                                                                                                        \
        if (Wsel == 1) DEC_LAUNCH(INT, 1, IN, CIN, L, OUT);                                                                     \
        else if (Wsel == 2) DEC_LAUNCH(INT, 2, IN, CIN, L, OUT);                                                                \
        else DEC_LAUNCH(INT, 4, IN, CIN, L, OUT);                                                                               \
    } while (0)
    if (frames_f64) DEC_LAUNCH_W(double, d_frames, d.C, 0, d.mid);
    else DEC_LAUNCH_W(float, d_frames, d.C, 0, d.mid);
    DEC_LAUNCH_W(float, d.mid, 2 * d.H, 1, d.top);
#undef DEC_LAUNCH_W
#undef DEC_LAUNCH
    const long rows = (long)S * T;
    const size_t rlds = ((size_t)d.O * (2 * d.H + 1) + (size_t)DEC_RROWS * 2 * d.H) * sizeof(float);
    hipLaunchKernelGGL(dec_regress_kernel, dim3((unsigned)((rows + DEC_RROWS - 1) / DEC_RROWS)), dim3(256), rlds, st, d.top, rows, 2 * d.H,
                       d.O, d.wr, d.br, d_feats, d_counts, T);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- a trial list (dss_dec_forward_trials_dev; the reference's validation pass, train_bidirectional_model.py:165-178) ----------
// The layers are bilstm_layer_kernel's ragged form as it is: trial s of the chunk is "row" first[s] of a buffer with ONE frame per
// row, i.e. frames first[s] + t of the concatenated (N, C) array, with counts[s] frames of its own -- so a trial's arithmetic is
// what dss_dec_forward_rows_dev gives it.  Only the regressor differs: its rows leave the padded (S, T) grid of the layer outputs
// for the trial's rows out_row[s] .. of the concatenated features (same dot product, term for term, as dec_regress_kernel).
__global__ void __launch_bounds__(256)
dec_regress_trials_kernel(const float *__restrict__ top, long rows, int K, int O, const float *__restrict__ w, const float *__restrict__ b,
                          float *__restrict__ feats, const int *__restrict__ counts, const long long *__restrict__ out_row, int T)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];             // [O][K + 1] weights, then [DEC_RROWS][K] inputs
    float *ws = rs, *xs = rs + (size_t)O * (K + 1);
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * DEC_RROWS;
    auto live = [&](long r) { return r < rows && (int)(r % T) < counts[r / T]; };
    bool any = false;                                      // (uniform over the block: a block of padding rows has nothing to do)
    for (int rr = 0; rr < DEC_RROWS; ++rr) any = any || live(r0 + rr);
    if (!any) return;
    for (int k = tid; k < O * K; k += 256) { const int o = k / K, j = k - o * K; ws[o * (K + 1) + j] = w[k]; }
    for (int k = tid; k < DEC_RROWS * K; k += 256) {
        const long r = r0 + k / K;
        xs[k] = live(r) ? top[r * K + (k % K)] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < DEC_RROWS * O; idx += 256) {
        const int rr = idx / O, o = idx - rr * O;
        const long r = r0 + rr;
        if (!live(r)) continue;
        const float *x = xs + rr * K, *wr = ws + o * (K + 1);
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = __builtin_fmaf(wr[k], x[k], a);
        feats[(size_t)(out_row[r / T] + r % T) * O + o] = a + b[o];
    }
}

int dss_launch_decoder_trials(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, float *d_feats,
                              const int *d_counts, const int *d_first, const long long *d_out_row, hipStream_t st)
{
    if (d.H < 1 || d.H > DEC_MAXH || 4 * d.H > DEC_THREADS || d.C < 1 || d.C > DEC_MAXC || 2 * d.H > DEC_MAXC) {
        dss_set_error("decoder kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", d.H, d.C, DEC_MAXH, DEC_MAXC);
        return DSS_EINVAL;
    }
    if (d.O < 1 || d.O > 32) { dss_set_error("decoder kernel: %d outputs out of range (<= 32)", d.O); return DSS_EINVAL; }
    if (S < 1 || S > d.S_max || T < 1 || T > d.T_max || !d_counts || !d_first || !d_out_row) {
        dss_set_error("decoder kernel: %d trials x %d frames exceed the handle's %d x %d", S, T, d.S_max, d.T_max);
        return DSS_EINVAL;
    }
    const int Wsel = 2 * S <= 256 ? 1 : (S <= 256 ? 2 : 4);                // as dss_launch_decoder
    const dim3 block(DEC_THREADS);
#define DEC_TLAUNCH(INT, WV, IN, CIN, L, OUT)                                                                                  \
    hipLaunchKernelGGL((bilstm_layer_kernel<INT, WV>), dim3((S + WV - 1) / WV, 2), block, 0, st, (const INT *)(IN), S, T, CIN, d.H,  \
                       d.wT[L][0], d.wT[L][1], d.b[L][0], d.b[L][1], OUT, d_counts, (L) == 0 ? d_first : (const int *)nullptr,    \
                       (L) == 0 ? 1 : T)
#define DEC_TLAUNCH_W(INT, IN, CIN, L, OUT)                                                                                     \
    do {                                                                                                                        \
        if (Wsel == 1) DEC_TLAUNCH(INT, 1, IN, CIN, L, OUT);                                                                    \
        else if (Wsel == 2) DEC_TLAUNCH(INT, 2, IN, CIN, L, OUT);                                                               \
        else DEC_TLAUNCH(INT, 4, IN, CIN, L, OUT);                                                                              \
    } while (0)
    if (frames_f64) DEC_TLAUNCH_W(double, d_frames, d.C, 0, d.mid);
    else DEC_TLAUNCH_W(float, d_frames, d.C, 0, d.mid);
    DEC_TLAUNCH_W(float, d.mid, 2 * d.H, 1, d.top);
#undef DEC_TLAUNCH_W
#undef DEC_TLAUNCH
    const long rows = (long)S * T;
    const size_t rlds = ((size_t)d.O * (2 * d.H + 1) + (size_t)DEC_RROWS * 2 * d.H) * sizeof(float);
    hipLaunchKernelGGL(dec_regress_trials_kernel, dim3((unsigned)((rows + DEC_RROWS - 1) / DEC_RROWS)), dim3(256), rlds, st, d.top, rows,
                       2 * d.H, d.O, d.wr, d.br, d_feats, d_counts, d_out_row, T);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- a trial list over the members of a group (dss_dec_group_forward_trials_dev; Part 17) --------------------------------------
// Every trial names the member that runs it, and the weights are the members' current ones: the packed copies and master
// parameters of the group's device table of trainer descriptors (DssDecTrainDev), read in stream order behind the members' steps.
// A thread keeps its row of W_hh in registers for the whole call, so the W streams of a layer workgroup belong to ONE model: the
// workgroup table names the model and the first of its n <= W stream slots, and the body is bilstm_layer_body as it is.  There is
// no padded (streams x longest) grid: a stream's layer outputs are rows buf_row .. buf_row + len of concatenated (rows, 2H)
// buffers, which layer 1 reads as layer 0 reads the frames, one frame per row.  The tables are constant while the launches run
// (dss_cp) and the pointers read from them are global pointers (dss_gp).
template <typename InT, int W>
__global__ void __launch_bounds__(DEC_THREADS)
bilstm_layer_group_kernel(const DssDecTrainDev *__restrict__ models, const InT *__restrict__ in, const int layer,
                          const DssDecGroupStream *__restrict__ streams, const DssDecGroupWg *__restrict__ wgs, float *__restrict__ out)
{
    const DssDecGroupWg &g = *dss_cp(wgs + blockIdx.x);
    const DssDecTrainDev &d = *dss_cp(models + g.model);
    const DssDecGroupStream *st = dss_cp(streams + g.slot0);
    const int dir = blockIdx.y, n = g.n;
    bilstm_layer_body<InT, W>(in, layer ? 2 * d.H : d.C, d.H, dss_gp(d.wT[layer][dir]), dss_gp(d.b[layer][dir]), dir, out,
                              [&](int sl, int &Ts, size_t &irow, size_t &orow) {
        const bool live = sl < n;
        const DssDecGroupStream &e = st[live ? sl : 0];
        Ts = live ? e.len : 0;
        irow = (size_t)(layer ? e.buf_row : e.in_row);
        orow = (size_t)e.buf_row;
    });
}

// The regressor of such a list: dec_regress_kernel's dot product term for term.  A block's n <= DEC_RROWS rows of `top` belong to
// one model, whose regressor is the last two of the eighteen tensors of its master parameters (torch layout, as the inference
// handle keeps them): o_wr, o_br are their offsets.  Row r of the buffer lies in the stream slot s >= block.slot with
// buf_row <= r < buf_row + len and goes to row out_row + (r - buf_row) of the concatenated features.
__global__ void __launch_bounds__(256)
dec_regress_trials_group_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupStream *__restrict__ streams,
                                const DssDecGroupBlock *__restrict__ blocks, const float *__restrict__ top, const int o_wr, const int o_br,
                                float *__restrict__ feats)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];             // [O][K + 1] weights, then [DEC_RROWS][K] inputs
    const DssDecGroupBlock &blk = *dss_cp(blocks + blockIdx.x);
    const DssDecTrainDev &d = *dss_cp(models + blk.model);
    const DssDecGroupStream *st = dss_cp(streams);
    const int K = 2 * d.H, O = d.O, nr = blk.n;
    const float *w = dss_gp(d.p) + o_wr, *b = dss_gp(d.p) + o_br;
    float *ws = rs, *xs = rs + (size_t)O * (K + 1);
    const int tid = threadIdx.x;
    const long long r0 = blk.row0;
    for (int k = tid; k < O * K; k += 256) { const int o = k / K, j = k - o * K; ws[o * (K + 1) + j] = w[k]; }
    for (int k = tid; k < DEC_RROWS * K; k += 256) {
        const int rr = k / K;
        xs[k] = rr < nr ? top[(size_t)(r0 + rr) * K + (k % K)] : 0.f;
    }
    __syncthreads();
    for (int idx = tid; idx < DEC_RROWS * O; idx += 256) {
        const int rr = idx / O, o = idx - rr * O;
        if (rr >= nr) continue;
        const long long r = r0 + rr;
        int s = blk.slot;                                  // at most DEC_RROWS - 1 streams end inside a block
        for (int j = 1; j < DEC_RROWS && r >= st[s].buf_row + st[s].len; ++j) ++s;
        const float *x = xs + rr * K, *wr = ws + o * (K + 1);
        float a = 0.f;
        for (int k = 0; k < K; ++k) a = __builtin_fmaf(wr[k], x[k], a);
        feats[(size_t)(st[s].out_row + (r - st[s].buf_row)) * O + o] = a + b[o];
    }
}

int dss_launch_decoder_trials_group(const DssDecTrainDev *d_models, int C, int H, int O, const void *d_frames, int frames_f64, int W,
                                    const DssDecGroupStream *d_streams, const DssDecGroupWg *d_wgs, int n_wgs,
                                    const DssDecGroupBlock *d_blocks, int n_blocks, float *d_mid, float *d_top, float *d_feats,
                                    hipStream_t st)
{
    if (H < 1 || H > DEC_MAXH || 4 * H > DEC_THREADS || C < 1 || C > DEC_MAXC || 2 * H > DEC_MAXC) {
        dss_set_error("decoder kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", H, C, DEC_MAXH, DEC_MAXC);
        return DSS_EINVAL;
    }
    if (O < 1 || O > 32) { dss_set_error("decoder kernel: %d outputs out of range (<= 32)", O); return DSS_EINVAL; }
    if ((W != 1 && W != 2 && W != 4) || n_wgs < 1 || n_blocks < 1 || !d_streams || !d_wgs || !d_blocks || !d_mid || !d_top) {
        dss_set_error("decoder group kernels: %d streams per workgroup, %d workgroups, %d blocks or a null table", W, n_wgs, n_blocks);
        return DSS_EINVAL;
    }
    const dim3 grid(n_wgs, 2), block(DEC_THREADS);
#define DEC_GLAUNCH(INT, WV, IN, L, OUT)                                                                                        \
    hipLaunchKernelGGL((bilstm_layer_group_kernel<INT, WV>), grid, block, 0, st, d_models, (const INT *)(IN), L, d_streams, d_wgs, OUT)
#define DEC_GLAUNCH_W(INT, IN, L, OUT)                                                                                          \
    do {                                                                                                                        \
        if (W == 1) DEC_GLAUNCH(INT, 1, IN, L, OUT);                                                                            \
        else if (W == 2) DEC_GLAUNCH(INT, 2, IN, L, OUT);                                                                       \
        else DEC_GLAUNCH(INT, 4, IN, L, OUT);                                                                                   \
    } while (0)
    if (frames_f64) DEC_GLAUNCH_W(double, d_frames, 0, d_mid);
    else DEC_GLAUNCH_W(float, d_frames, 0, d_mid);
    DEC_GLAUNCH_W(float, d_mid, 1, d_top);
#undef DEC_GLAUNCH_W
#undef DEC_GLAUNCH
    DSS_HIP_CHECK(hipGetLastError());
    const int total = (int)dss_dec_train_param_count(C, H, O);             // the regressor's weight and bias stand last
    const size_t rlds = ((size_t)O * (2 * H + 1) + (size_t)DEC_RROWS * 2 * H) * sizeof(float);
    hipLaunchKernelGGL(dec_regress_trials_group_kernel, dim3((unsigned)n_blocks), dim3(256), rlds, st, d_models, d_streams, d_blocks, d_top,
                       total - O - O * 2 * H, total - O, d_feats);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// per-trial mean squared error of concatenated (sum len, O) features against targets of the same shape (nn.MSELoss() on one trial,
// train_bidirectional_model.py:176-177), in float64 in a fixed order: thread t of the trial's workgroup adds the squared
// differences of elements t, t + 256, ... in that order, then a halving tree over the 256 partial sums.  The launch's trials
// travel as kernel arguments (DssTrialLens).
__global__ void __launch_bounds__(256)
dec_mse_trials_kernel(DssTrialLens tl, const float *__restrict__ feats, const float *__restrict__ targets, int O, double *__restrict__ mse)
{
    __shared__ double part[256];
    const int tid = threadIdx.x, k = blockIdx.x;
    long long off = tl.base;
    for (int j = 0; j < k; ++j) off += tl.len[j];
    const long long n = (long long)tl.len[k] * O;
    const float *f = feats + off * O, *g = targets + off * O;
    double acc = 0.0;
    for (long long i = tid; i < n; i += 256) { const double e = (double)f[i] - (double)g[i]; acc += e * e; }
    part[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid == 0) mse[tl.first_trial + k] = part[0] / (double)n;
}

int dss_launch_dec_mse_trials(const DssTrialLens &tl, const float *d_feats, const float *d_targets, int n_outputs, double *d_mse,
                              hipStream_t st)
{
    hipLaunchKernelGGL(dec_mse_trials_kernel, dim3(tl.n), dim3(256), 0, st, tl, d_feats, d_targets, n_outputs, d_mse);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
