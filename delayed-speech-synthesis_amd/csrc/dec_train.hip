// csrc/dec_train.hip -- one training step of the bidirectional decoder (gfx950): backpropagation through a whole trial, and the
// RMSprop update.
//
// Restates, for batch size 1 (the only one the reference's script uses),
//   train_bidirectional_model.py:134-152  per trial of T frames: forward from the zero state, nn.MSELoss (the mean over the T x O
//                                         elements), backward to all eighteen parameter tensors, optim.step()
//   torch.optim.RMSprop(lr, alpha, eps)   sq <- alpha sq + (1 - alpha) g^2;  p <- p - lr g / (sqrt(sq) + eps)
//   nn.LSTM(dropout = p), train mode      layer 0's output [h_forward(t) | h_backward(t)], as layer 1 reads it, times a mask of 0 or
//                                         1 / (1 - p); the mask is an INPUT here, (T, 2H) multipliers or NULL
// The steps of one direction of one layer are serial; the two directions of a layer are independent, and so are the frames
// everywhere else.  Seven launches per trial on one stream ("Training the decoder"):
//   dec_train_layer_kernel<0>, <1>   a workgroup per direction: bilstm_layer_body (lstm_blocks.h), the loop the inference kernels run,
//                                    for one stream, keeping the stash the backward pass needs
//   dec_train_head_kernel            a workgroup per 8 frames: features (dec_regress_rows, the inference kernels' regressor), dfeat,
//                                    the per-frame loss terms, dtop = W_r^T dfeat
//   dec_train_bptt_kernel<1>         a workgroup per direction: backward through time, the gate gradients dG1[dir][T][4H]; a
//                                    third workgroup adds the per-frame loss terms in frame order
//   dec_train_dmid_kernel            a workgroup per 8 frames: what layer 1 sends down through both W_ih_l1 and the mask
//   dec_train_bptt_kernel<0>         dG0[dir][T][4H]
//   dec_train_step_kernel            a workgroup per gate row of each (layer, direction) and per row of the regressor: the weight
//                                    gradients as sums over t in frame order, the bias gradients and, fused, the RMSprop update
//                                    of the master parameters (torch layout) and of the packed copies the forward pass reads
// Every sum has a fixed order and there are no atomics: the same call from the same state gives the same bits.  Fused
// multiply-adds are written out (__builtin_fmaf); the library is built with -ffp-contract=off.
// Each kernel's body is a __device__ __forceinline__ function that takes the descriptor by reference and the block's index as an
// argument, because two kernels run it: the single trainer's (above), and the group form at the end of this file, which steps
// several trainers in one launch (blockIdx.y is the model; DESIGN.md, "Training several decoders at once").  The arithmetic is
// stated once, so a model's bits do not depend on which of the two ran it.
#include "lstm_blocks.h"

// offsets of the eighteen tensors in the flat parameter array (state_dict order; also of the gradients and the square averages)
__host__ __device__ static inline DssDecTrainOff dec_train_off(int C, int H, int O)
{
    DssDecTrainOff o;
    const int H4 = 4 * H;
    int k = 0;
    for (int L = 0; L < 2; ++L)
        for (int dir = 0; dir < 2; ++dir) {
            o.wih[L][dir] = k; k += H4 * (L ? 2 * H : C);
            o.whh[L][dir] = k; k += H4 * H;
            o.bih[L][dir] = k; k += H4;
            o.bhh[L][dir] = k; k += H4;
        }
    o.wr = k; k += O * 2 * H;
    o.br = k; k += O;
    o.total = k;
    return o;
}

long dss_dec_train_param_count(int C, int H, int O) { return dec_train_off(C, H, O).total; }

// Every pointer read from the descriptor or from a trial table goes through dss_gp (dss_global_ptr.h): the group kernels at the end
// of this file load them from a table, and must still address global memory, not the flat aperture.

// ---- forward, one layer: bilstm_layer_body (lstm_blocks.h) for one stream, keeping the stash -------------------------------------
// The loop is the inference kernels', so the features of a trial without a mask are their bits.  dir is the direction; step s is
// frame s (forward) or T - 1 - s (backward).  Kept of a step: the activated gates (row s of act), c and h behind it (row s + 1 of
// the stashes; row 0 is the zero state), h at the step's frame -- times the mask in layer 0 (midm), as it is in layer 1 (top);
// the unmasked h is what the direction carries to its own next step -- and, from layer 0's forward direction, the frames as
// float32 (xs).
template <typename InT, int LAYER>
__device__ __forceinline__ void dec_train_layer_body(const DssDecTrainDev &d, const int dir, const InT *__restrict__ in, const int T,
                                                     const float *__restrict__ mask)
{
    const int tid = threadIdx.x, H = d.H, H4 = 4 * H, Cin = LAYER ? 2 * H : d.C;
    float *act = dss_gp(d.act[LAYER][dir]), *cst = dss_gp(d.c[LAYER][dir]), *hst = dss_gp(d.h[LAYER][dir]);
    float *xs = dss_gp(d.xs), *out = dss_gp(LAYER ? d.top : d.midm);
    if (tid < H) { cst[tid] = 0.f; hst[tid] = 0.f; }
    bilstm_layer_body<InT, 1>(in, Cin, H, dss_gp(d.wT[LAYER][dir]), dss_gp(d.b[LAYER][dir]), dir,
                              [&](int, int &Ts, size_t &irow, size_t &orow) { Ts = T; irow = 0; orow = 0; },
                              [&](size_t t, int k, float x) { if (LAYER == 0 && dir == 0) xs[t * Cin + k] = x; },
                              [&](int step, size_t t, int u, float gi, float gf, float gg, float go, float c, float h) {
        float *a = act + (size_t)step * H4;
        a[u] = gi; a[H + u] = gf; a[2 * H + u] = gg; a[3 * H + u] = go;
        cst[(size_t)(step + 1) * H + u] = c;
        hst[(size_t)(step + 1) * H + u] = h;
        const size_t oi = t * (2 * H) + dir * H + u;
        out[oi] = LAYER == 0 && mask ? h * mask[oi] : h;
    });
}

template <typename InT, int LAYER>
__global__ void __launch_bounds__(DEC_THREADS)
dec_train_layer_kernel(DssDecTrainDev d, const InT *__restrict__ in, int T, const float *__restrict__ mask)
{
    dec_train_layer_body<InT, LAYER>(d, blockIdx.x, in, T, mask);
}

// ---- head, loss terms, gradient of the features ---------------------------------------------------------------------------------
// A workgroup takes DEC_RROWS frames.  feat[t][o] = b[o] + sum_k w[o][k] top[t][k] is dec_regress_rows (lstm_blocks.h), the inference
// kernels' regressor; dfeat = 2 (feat - target) / (T O), evaluated in float64 and rounded once; lossf[t] = sum over o, in that
// order, of the squared differences in float64; dtop[t][k] = sum over o, in that order, of w[o][k] dfeat[t][o].
__device__ __forceinline__ void dec_train_head_body(const DssDecTrainDev &d, const int blk, const int T, const float *__restrict__ targets)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];             // dec_regress_rows' weights and inputs, then [DEC_RROWS][O] dfeat
    __shared__ double es[DEC_RROWS][DSS_DEC_MAXO];
    const int tid = threadIdx.x, K = 2 * d.H, O = d.O;
    const DssDecTrainOff o = dec_train_off(d.C, d.H, O);
    const float *ws = rs, *top = dss_gp(d.top);
    float *dfs = rs + dec_regress_lds_floats(K, O);
    const int t0 = blk * DEC_RROWS, nst = min(DEC_RROWS, T - t0);
    dec_regress_rows(rs, K, O, dss_gp(d.p) + o.wr, dss_gp(d.p) + o.br, [&](int rr) { return rr < nst ? top + (size_t)(t0 + rr) * K : nullptr; },
                     [&](int rr, int oo, float f) {
        const size_t fi = (size_t)(t0 + rr) * O + oo;
        const double e = (double)f - (double)targets[fi];
        const float df = (float)(2.0 * e / ((double)T * (double)O));
        dss_gp(d.feat)[fi] = f;
        dss_gp(d.dfeat)[fi] = df;
        dfs[rr * O + oo] = df;
        es[rr][oo] = e;
    });
    __syncthreads();
    if (tid < nst) {
        double acc = 0.0;
        for (int oo = 0; oo < O; ++oo) acc += es[tid][oo] * es[tid][oo];
        dss_gp(d.lossf)[t0 + tid] = acc;
    }
    for (int idx = tid; idx < nst * K; idx += 256) {
        const int rr = idx / K, k = idx - rr * K;
        float a = 0.f;
        for (int oo = 0; oo < O; ++oo) a = __builtin_fmaf(ws[oo * (K + 1) + k], dfs[rr * O + oo], a);
        dss_gp(d.dtop)[(size_t)(t0 + rr) * K + k] = a;
    }
}

__global__ void __launch_bounds__(256)
dec_train_head_kernel(DssDecTrainDev d, int T, const float *__restrict__ targets)
{
    dec_train_head_body(d, blockIdx.x, T, targets);
}

// ---- backward through time of one (layer, direction) --------------------------------------------------------------------------
// blockIdx.x is the direction.  Thread u < H owns unit u: dh = (what the step after this one sends through W_hh) + (what arrives
// from above at the step's frame: dtop for layer 1, dmid for layer 0); dc likewise carries f dc of the step after, in a register.
// "The step after" is in the direction's own time: frame t + 1 forward, frame t - 1 backward, so the backward direction walks the
// frames upward.  The four gate gradients of the step go to LDS and to dG at the step's FRAME; then thread (gate q, column j)
// forms its part of W_hh^T dG for the step before from column j of gate q's rows of the row-major master copy, which it holds in
// registers for the whole trial (the H rows in row order), and the owner adds the four parts as (i + f) + (g + o).
// The owner's seven stash values of a step are loaded one step ahead, so their latency is off the chain.
// Layer 1's launch has a third workgroup: the trial's loss, the per-frame terms added in frame order in float64.
__device__ __forceinline__ void dec_train_loss_body(const DssDecTrainDev &d, const int T, double *__restrict__ loss)
{
    __shared__ double ls[DSS_DEC_TRAIN_MAXT];
    const int tid = threadIdx.x;
    for (int t = tid; t < T; t += DEC_THREADS) ls[t] = dss_gp(d.lossf)[t];
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc += ls[t];
        *loss = acc / ((double)T * (double)d.O);
    }
}

template <int LAYER>
__device__ __forceinline__ void dec_train_bptt_body(const DssDecTrainDev &d, const int dir, const int T)
{
    __shared__ __attribute__((aligned(16))) float dgs[4][DEC_MAXH];       // the gate gradients of the step in hand; units >= H stay zero
    __shared__ float part[4][DEC_MAXH];                                   // W_hh^T dG per gate, before the owner adds them
    const int tid = threadIdx.x, H = d.H, H4 = 4 * H;
    const DssDecTrainOff o = dec_train_off(d.C, H, d.O);
    const float *Whh = dss_gp(d.p) + (dir ? o.whh[LAYER][1] : o.whh[LAYER][0]);
    const int q = tid / DEC_MAXH, j = tid - q * DEC_MAXH;
    const bool own = tid < H, colt = j < H;
    float wt[DEC_MAXH];
#pragma unroll
    for (int r = 0; r < DEC_MAXH; ++r) wt[r] = (colt && r < H) ? Whh[((size_t)q * H + r) * H + j] : 0.f;
    reinterpret_cast<float *>(dgs)[tid] = 0.f;             // (DEC_THREADS == 4 * DEC_MAXH)
    const float *act = dss_gp(dir ? d.act[LAYER][1] : d.act[LAYER][0]), *cst = dss_gp(dir ? d.c[LAYER][1] : d.c[LAYER][0]);
    const float *up = dss_gp(LAYER ? d.dtop : d.dmid) + dir * H + tid;
    float *dG = dss_gp(dir ? d.dg[LAYER][1] : d.dg[LAYER][0]);
    // the owner's stash values of step s, into seven registers
#define DEC_LOAD_STEP(s)                                                                                                           \
    do {                                                                                                                           \
        const float *a_ = act + (size_t)(s) * H4;                                                                                  \
        n_gi = a_[tid]; n_gf = a_[H + tid]; n_gg = a_[2 * H + tid]; n_go = a_[3 * H + tid];                                        \
        n_c = cst[(size_t)((s) + 1) * H + tid]; n_cp = cst[(size_t)(s) * H + tid];                                                 \
        n_up = up[(size_t)(dir ? T - 1 - (s) : (s)) * (2 * H)];                                                                    \
    } while (0)
    float n_gi = 0.f, n_gf = 0.f, n_gg = 0.f, n_go = 0.f, n_c = 0.f, n_cp = 0.f, n_up = 0.f;
    if (own) DEC_LOAD_STEP(T - 1);
    float dcn = 0.f;
    __syncthreads();
    for (int s = T - 1; s >= 0; --s) {
        if (own) {
            const float v_gi = n_gi, v_gf = n_gf, v_gg = n_gg, v_go = n_go, v_c = n_c, v_cp = n_cp, v_up = n_up;
            if (s > 0) DEC_LOAD_STEP(s - 1);
            const int t = dir ? T - 1 - s : s;
            float dh = s == T - 1 ? 0.f : (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
            dh += v_up;
            const float tc = tanhf(v_c);
            const float dc = __builtin_fmaf(dh * v_go, 1.f - tc * tc, dcn);
            const float di = dc * v_gg * (v_gi * (1.f - v_gi));
            const float df = dc * v_cp * (v_gf * (1.f - v_gf));
            const float dg = dc * v_gi * (1.f - v_gg * v_gg);
            const float dO = dh * tc * (v_go * (1.f - v_go));
            dcn = dc * v_gf;
            dgs[0][tid] = di; dgs[1][tid] = df; dgs[2][tid] = dg; dgs[3][tid] = dO;
            float *g = dG + (size_t)t * H4;
            g[tid] = di; g[H + tid] = df; g[2 * H + tid] = dg; g[3 * H + tid] = dO;
        }
        __syncthreads();
        if (s > 0 && colt) {
            float acc = 0.f;
#pragma unroll
            for (int k = 0; k < DEC_MAXH / 4; ++k) {
                if (4 * k >= H) break;
                const f4 g4 = *reinterpret_cast<const f4 *>(&dgs[q][4 * k]);
                acc = __builtin_fmaf(wt[4 * k], g4.x, acc);
                acc = __builtin_fmaf(wt[4 * k + 1], g4.y, acc);
                acc = __builtin_fmaf(wt[4 * k + 2], g4.z, acc);
                acc = __builtin_fmaf(wt[4 * k + 3], g4.w, acc);
            }
            part[q][j] = acc;
        }
        __syncthreads();
    }
#undef DEC_LOAD_STEP
}

template <int LAYER>
__global__ void __launch_bounds__(DEC_THREADS)
dec_train_bptt_kernel(DssDecTrainDev d, int T, double *__restrict__ loss)
{
    if (LAYER == 1 && blockIdx.x == 2) {
        dec_train_loss_body(d, T, loss);
        return;
    }
    dec_train_bptt_body<LAYER>(d, blockIdx.x, T);
}

// ---- what layer 1 sends down ------------------------------------------------------------------------------------------------------
// dmid[t][k] = mask[t][k] (sum_r W_ih_l1[r][k] dG1[fwd][t][r] + sum_r W_ih_l1_reverse[r][k] dG1[bwd][t][r]), k < 2H: each sum over
// the 4H gate rows in row order, the forward direction's first.  A workgroup takes DTM_FR frames; thread k owns column k, so a wave's
// load of a weight row is consecutive bytes; the gate gradients of the frames sit side by side in LDS (broadcast reads).
#define DTM_FR 8
__device__ __forceinline__ void dec_train_dmid_body(const DssDecTrainDev &d, const int blk, const int T, const float *__restrict__ mask)
{
    __shared__ __attribute__((aligned(16))) float dgl[2][4 * DEC_MAXH][DTM_FR];
    const int tid = threadIdx.x, H = d.H, H4 = 4 * H, K = 2 * H;
    const DssDecTrainOff o = dec_train_off(d.C, H, d.O);
    const int t0 = blk * DTM_FR, nst = min(DTM_FR, T - t0);
    for (int idx = tid; idx < 2 * DTM_FR * H4; idx += 256) {
        const int dd = idx / (DTM_FR * H4), rem = idx - dd * (DTM_FR * H4);
        const int tt = rem / H4, r = rem - tt * H4;
        dgl[dd][r][tt] = tt < nst ? dss_gp(d.dg[1][dd])[(size_t)(t0 + tt) * H4 + r] : 0.f;
    }
    __syncthreads();
    if (tid >= K) return;
    float acc[2][DTM_FR];
#pragma unroll
    for (int dd = 0; dd < 2; ++dd) {
#pragma unroll
        for (int tt = 0; tt < DTM_FR; ++tt) acc[dd][tt] = 0.f;
        const float *W = dss_gp(d.p) + o.wih[1][dd] + tid;
        int r = 0;
        for (; r + 4 <= H4; r += 4) {
            float w[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) w[u] = W[(size_t)(r + u) * K];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f4 g0 = *reinterpret_cast<const f4 *>(&dgl[dd][r + u][0]), g1 = *reinterpret_cast<const f4 *>(&dgl[dd][r + u][4]);
                acc[dd][0] = __builtin_fmaf(w[u], g0.x, acc[dd][0]); acc[dd][1] = __builtin_fmaf(w[u], g0.y, acc[dd][1]);
                acc[dd][2] = __builtin_fmaf(w[u], g0.z, acc[dd][2]); acc[dd][3] = __builtin_fmaf(w[u], g0.w, acc[dd][3]);
                acc[dd][4] = __builtin_fmaf(w[u], g1.x, acc[dd][4]); acc[dd][5] = __builtin_fmaf(w[u], g1.y, acc[dd][5]);
                acc[dd][6] = __builtin_fmaf(w[u], g1.z, acc[dd][6]); acc[dd][7] = __builtin_fmaf(w[u], g1.w, acc[dd][7]);
            }
        }                                                  // (4H is a multiple of 4: no remainder)
    }
#pragma unroll
    for (int tt = 0; tt < DTM_FR; ++tt) {
        if (tt >= nst) break;
        const size_t oi = (size_t)(t0 + tt) * K + tid;
        float s = acc[0][tt] + acc[1][tt];
        if (mask) s *= mask[oi];
        dss_gp(d.dmid)[oi] = s;
    }
}

__global__ void __launch_bounds__(256)
dec_train_dmid_kernel(DssDecTrainDev d, int T, const float *__restrict__ mask)
{
    dec_train_dmid_body(d, blockIdx.x, T, mask);
}

// ---- the parallel part: weight gradients and the RMSprop update --------------------------------------------------------------
// Workgroup b < 16H is gate row r of (layer L, direction dir), b = (2 L + dir) 4H + r: its columns are [W_ih row | W_hh row | bias],
// column k's gradient is the sum over the frames t = 0 .. T-1, in that order, of dG[t][r] in[t][k] (one fused multiply-add per
// frame; the bias adds dG[t][r] itself).  Workgroups 16H .. 16H + O - 1 are the rows of the regressor: [weight row | bias]
// against dfeat.  The inputs: layer 0 reads the frames (xs), layer 1 the masked output of layer 0 (midm), the head layer 1's output
// (top); the W_hh columns read the direction's own h of the step before -- frame t is step t forward, step T - 1 - t backward, and
// row s of the stash is h before step s (row 0: zeros).
// The sums, the update and the write-back are lstm_train_step_row (lstm_blocks.h), the detector's too.
// Two columns per thread: a row has at most max(C, 2H) + H + 1 <= 256 + 128 + 1 = 385 <= 2 x 256 columns.
#define DTS_THREADS 256

__device__ __forceinline__ void dec_train_step_body(const DssDecTrainDev &d, const int b, const int T, const int apply, const double lr,
                                                    const double alpha, const double eps)
{
    const int C = d.C, H = d.H, H4 = 4 * H, O = d.O;
    const bool head = b >= 4 * H4;
    const int LD = head ? 0 : b / H4, L = LD >> 1, dir = LD & 1, r = head ? b - 4 * H4 : b - LD * H4;
    // the flat offsets of this (layer, direction)'s four tensors, and of the head (dec_train_off, without an indexed table)
    const int sz0 = H4 * (C + H + 2), sz1 = H4 * (3 * H + 2);
    const int nA = head || L ? 2 * H : C;
    const int o_wih = LD < 2 ? LD * sz0 : 2 * sz0 + (LD - 2) * sz1, o_whh = o_wih + H4 * nA, o_bih = o_whh + H4 * H, o_bhh = o_bih + H4;
    const int o_wr = 2 * sz0 + 2 * sz1, o_br = o_wr + O * 2 * H;
    LstmStepRow w;
    w.dg = dss_gp(head ? d.dfeat : d.dg[L][dir]) + r;
    w.dgs = head ? O : H4;
    w.inA = dss_gp(head ? d.top : (L ? d.midm : d.xs));
    w.nA = nA;
    // frame t is step T - 1 - t of the backward direction: its stash of h is read from the last row upward
    w.inB = dss_gp(d.h[L][dir]) + (dir ? (size_t)(T - 1) * H : 0);
    w.nB = head ? 0 : H;
    w.strideB = dir ? -(long)H : (long)H;
    w.o_A = (head ? o_wr : o_wih) + r * nA;
    w.o_B = o_whh + r * H;
    w.o_bias = head ? o_br + r : o_bih + r;
    w.o_bias2 = o_bhh + r;
    w.wpk = head ? nullptr : dss_gp(d.wT[L][dir]);
    w.bpk = dss_gp(d.b[L][dir]) + r;
    w.r = r; w.H4 = H4; w.kB = (nA + 3) & ~3;
    lstm_train_step_row<DTS_THREADS>(w, dss_gp(d.p), dss_gp(d.sq), dss_gp(d.g), T, apply, lr, alpha, eps);
}


__global__ void __launch_bounds__(DTS_THREADS)
dec_train_step_kernel(DssDecTrainDev d, int T, int apply, double lr, double alpha, double eps)
{
    dec_train_step_body(d, blockIdx.x, T, apply, lr, alpha, eps);
}

int dss_launch_dec_train_trial(const DssDecTrainDev &d, const void *d_frames, int frames_f64, int T, const float *d_targets,
                               const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss, hipStream_t st)
{
    const int H = d.H, C = d.C, O = d.O;
    if (!dec_fits(C, H) || O < 1 || O > DSS_DEC_MAXO || d.Tmax > DSS_DEC_TRAIN_MAXT || T < 1 || T > d.Tmax) {
        dss_set_error("decoder training kernels: %d hidden units / %d inputs / %d outputs / %d frames out of range (<= %d / <= %d / <= %d / <= %d)",
                      H, C, O, T, DEC_MAXH, DEC_MAXC, DSS_DEC_MAXO, d.Tmax);
        return DSS_EINVAL;
    }
    const dim3 two(2), block(DEC_THREADS);
    if (frames_f64) hipLaunchKernelGGL((dec_train_layer_kernel<double, 0>), two, block, 0, st, d, (const double *)d_frames, T, d_mask);
    else hipLaunchKernelGGL((dec_train_layer_kernel<float, 0>), two, block, 0, st, d, (const float *)d_frames, T, d_mask);
    hipLaunchKernelGGL((dec_train_layer_kernel<float, 1>), two, block, 0, st, d, (const float *)d.midm, T, (const float *)nullptr);
    DSS_HIP_CHECK(hipGetLastError());
    const size_t hlds = (dec_regress_lds_floats(2 * H, O) + (size_t)DEC_RROWS * O) * sizeof(float);
    hipLaunchKernelGGL(dec_train_head_kernel, dim3((T + DEC_RROWS - 1) / DEC_RROWS), dim3(256), hlds, st, d, T, d_targets);
    hipLaunchKernelGGL((dec_train_bptt_kernel<1>), dim3(3), block, 0, st, d, T, d_loss);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dec_train_dmid_kernel, dim3((T + DTM_FR - 1) / DTM_FR), dim3(256), 0, st, d, T, d_mask);
    hipLaunchKernelGGL((dec_train_bptt_kernel<0>), two, block, 0, st, d, T, (double *)nullptr);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dec_train_step_kernel, dim3(16 * H + O), dim3(DTS_THREADS), 0, st, d, T, apply_step, lr, alpha, eps);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- several trainers in one launch (Part 13) ---------------------------------------------------------------------------------
// The same seven launches with a model axis: blockIdx.y is the model, blockIdx.x keeps its meaning.  A workgroup reads its model's
// descriptor from a device table of M and its model's entry of the step's trial table (uniform addresses: scalar loads), then runs
// the body the single-trainer kernel runs, so a model's numbers do not depend on M, on its place in the group or on what the others
// do.  The grids of the head and of dmid cover the longest trial of the step; workgroups past their own model's T return at once,
// and T == 0 is a model that sits the step out: none of its workgroups writes anything.
// Layer 1's BPTT launch is (2, M + ceil(M / 2)): rows y < M are the chains of model y, the rows behind them are the loss-adding
// workgroups of models 2 (y - M) + x, so that every chain is dispatched before the first of them.
template <typename InT, int LAYER>
__global__ void __launch_bounds__(DEC_THREADS)
dec_group_layer_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupTrial *__restrict__ trials)
{
    const DssDecGroupTrial tr = trials[blockIdx.y];
    if (tr.T <= 0) return;
    const DssDecTrainDev &d = models[blockIdx.y];
    if (LAYER) dec_train_layer_body<InT, LAYER>(d, blockIdx.x, dss_gp((const InT *)d.midm), tr.T, (const float *)nullptr);
    else dec_train_layer_body<InT, LAYER>(d, blockIdx.x, dss_gp((const InT *)tr.frames), tr.T, dss_gp(tr.mask));
}

__global__ void __launch_bounds__(256)
dec_group_head_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupTrial *__restrict__ trials)
{
    const DssDecGroupTrial tr = trials[blockIdx.y];
    if ((int)blockIdx.x * DEC_RROWS >= tr.T) return;
    const DssDecTrainDev &d = models[blockIdx.y];
    dec_train_head_body(d, blockIdx.x, tr.T, dss_gp(tr.targets));
}

template <int LAYER>
__global__ void __launch_bounds__(DEC_THREADS)
dec_group_bptt_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupTrial *__restrict__ trials, int M)
{
    if (LAYER == 1 && (int)blockIdx.y >= M) {
        const int m = 2 * ((int)blockIdx.y - M) + (int)blockIdx.x;
        if (m >= M) return;
        const DssDecGroupTrial tr = trials[m];
        if (tr.T <= 0) return;
        const DssDecTrainDev &d = models[m];
        dec_train_loss_body(d, tr.T, dss_gp(tr.loss));
        return;
    }
    const DssDecGroupTrial tr = trials[blockIdx.y];
    if (tr.T <= 0) return;
    const DssDecTrainDev &d = models[blockIdx.y];
    dec_train_bptt_body<LAYER>(d, blockIdx.x, tr.T);
}

__global__ void __launch_bounds__(256)
dec_group_dmid_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupTrial *__restrict__ trials)
{
    const DssDecGroupTrial tr = trials[blockIdx.y];
    if ((int)blockIdx.x * DTM_FR >= tr.T) return;
    const DssDecTrainDev &d = models[blockIdx.y];
    dec_train_dmid_body(d, blockIdx.x, tr.T, dss_gp(tr.mask));
}

__global__ void __launch_bounds__(DTS_THREADS)
dec_group_step_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupTrial *__restrict__ trials)
{
    const DssDecGroupTrial tr = trials[blockIdx.y];
    if (tr.T <= 0) return;
    const DssDecTrainDev &d = models[blockIdx.y];
    dec_train_step_body(d, blockIdx.x, tr.T, tr.apply, tr.lr, tr.alpha, tr.eps);
}

int dss_launch_dec_train_group(const DssDecTrainDev *d_models, const DssDecGroupTrial *d_trials, int M, int C, int H, int O, int max_T,
                               int frames_f64, hipStream_t st)
{
    if (M < 1 || M > DSS_DEC_GROUP_MAXM || !dec_fits(C, H) || O < 1 || O > DSS_DEC_MAXO || max_T < 1 || max_T > DSS_DEC_TRAIN_MAXT) {
        dss_set_error("decoder group kernels: %d models / %d hidden units / %d inputs / %d outputs / %d frames out of range (<= %d / <= %d / <= %d / <= %d / <= %d)",
                      M, H, C, O, max_T, DSS_DEC_GROUP_MAXM, DEC_MAXH, DEC_MAXC, DSS_DEC_MAXO, DSS_DEC_TRAIN_MAXT);
        return DSS_EINVAL;
    }
    const dim3 two(2, M), block(DEC_THREADS);
    if (frames_f64) hipLaunchKernelGGL((dec_group_layer_kernel<double, 0>), two, block, 0, st, d_models, d_trials);
    else hipLaunchKernelGGL((dec_group_layer_kernel<float, 0>), two, block, 0, st, d_models, d_trials);
    hipLaunchKernelGGL((dec_group_layer_kernel<float, 1>), two, block, 0, st, d_models, d_trials);
    DSS_HIP_CHECK(hipGetLastError());
    const size_t hlds = (dec_regress_lds_floats(2 * H, O) + (size_t)DEC_RROWS * O) * sizeof(float);
    hipLaunchKernelGGL(dec_group_head_kernel, dim3((max_T + DEC_RROWS - 1) / DEC_RROWS, M), dim3(256), hlds, st, d_models, d_trials);
    hipLaunchKernelGGL((dec_group_bptt_kernel<1>), dim3(2, M + (M + 1) / 2), block, 0, st, d_models, d_trials, M);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dec_group_dmid_kernel, dim3((max_T + DTM_FR - 1) / DTM_FR, M), dim3(256), 0, st, d_models, d_trials);
    hipLaunchKernelGGL((dec_group_bptt_kernel<0>), two, block, 0, st, d_models, d_trials, M);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(dec_group_step_kernel, dim3(16 * H + O, M), dim3(DTS_THREADS), 0, st, d_models, d_trials);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
