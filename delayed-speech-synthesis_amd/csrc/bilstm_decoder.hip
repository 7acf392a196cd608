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

// One layer, one workgroup, as inference runs it: bilstm_layer_body (lstm_blocks.h, where the trainers' forward half finds it too)
// keeping h alone -- forward h goes to columns [0, H) of the frame's row of out, backward h to [H, 2H).  Both layer kernels of
// this file (below, and the group form further down) go through here.
template <typename InT, int W, typename StreamFn>
__device__ __forceinline__ void bilstm_layer_infer(const InT *__restrict__ in, const int Cin, const int H, const float *__restrict__ wT,
                                                   const float *__restrict__ bias_v, const int dir, float *__restrict__ out, StreamFn stream)
{
    bilstm_layer_body<InT, W>(in, Cin, H, wT, bias_v, dir, stream, [](size_t, int, float) {},
                              [&](int, size_t row, int u, float, float, float, float, float, float h) { out[row * (2 * H) + dir * H + u] = h; });
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
    bilstm_layer_infer<InT, W>(in, Cin, H, dir ? wT_b : wT_f, dir ? b_b : b_f, dir, out, [&](int sl, int &Ts, size_t &irow, size_t &orow) {
        const int s = s0 + sl;
        const bool live = s < S;
        Ts = live ? (counts ? min(counts[s], T) : T) : 0;
        irow = live ? (size_t)(in_row ? in_row[s] : s) * Tin : 0;
        orow = (size_t)s * T;
    });
}

// regressor: feats[row][o] for the rows (stream, frame) of the padded (S, T) grid, DEC_RROWS per block (dec_regress_rows).
__global__ void __launch_bounds__(256)
dec_regress_kernel(const float *__restrict__ top, long rows, int K, int O, const float *__restrict__ w, const float *__restrict__ b,
                   float *__restrict__ feats, const int *__restrict__ counts, int T)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];
    const long r0 = (long)blockIdx.x * DEC_RROWS;
    // ragged calls: row r = (stream r / T, frame r % T) exists only below its stream's frame count
    dec_regress_rows(rs, K, O, w, b, [&](int rr) {
        const long r = r0 + rr;
        return r < rows && (!counts || (int)(r % T) < counts[r / T]) ? top + r * K : nullptr;
    }, [&](int rr, int o, float f) { feats[(r0 + rr) * O + o] = f; });
}

// the two layers of a call: S streams of at most T frames, counts[s] of them (NULL: T); layer 0 reads stream s from row in_row[s]
// (NULL: s) of a buffer with Tin frames per row, layer 1 the padded grid layer 0 wrote.
// Streams per workgroup: a thread's work per step grows with W, the number of workgroups shrinks with it; 2 x S / W of them
// should still cover the CUs (64 streams: 128 workgroups of one stream; 1024 streams: 512 of four).
template <typename InT, int W>
static void dec_launch_layers_as(const DssDecDev &d, const void *d_frames, int S, int T, const int *d_counts, const int *d_in_row, int Tin,
                                 hipStream_t st)
{
    const dim3 grid((S + W - 1) / W, 2), block(DEC_THREADS);
    hipLaunchKernelGGL((bilstm_layer_kernel<InT, W>), grid, block, 0, st, (const InT *)d_frames, S, T, d.C, d.H, d.wT[0][0], d.wT[0][1],
                       d.b[0][0], d.b[0][1], d.mid, d_counts, d_in_row, Tin);
    hipLaunchKernelGGL((bilstm_layer_kernel<float, W>), grid, block, 0, st, (const float *)d.mid, S, T, 2 * d.H, d.H, d.wT[1][0], d.wT[1][1],
                       d.b[1][0], d.b[1][1], d.top, d_counts, (const int *)nullptr, T);
}

static void dec_launch_layers(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, const int *d_counts,
                              const int *d_in_row, int Tin, hipStream_t st)
{
    const int W = dss_dec_streams_per_wg(S);
    auto *launch = frames_f64 ? (W == 1 ? dec_launch_layers_as<double, 1> : W == 2 ? dec_launch_layers_as<double, 2> : dec_launch_layers_as<double, 4>)
                              : (W == 1 ? dec_launch_layers_as<float, 1> : W == 2 ? dec_launch_layers_as<float, 2> : dec_launch_layers_as<float, 4>);
    launch(d, d_frames, S, T, d_counts, d_in_row, Tin, st);
}

int dss_launch_decoder(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, float *d_feats,
                       const int *d_counts, const int *d_in_row, int Tin, hipStream_t st)
{
    if (Tin <= 0) Tin = T;                                 // plain calls: the input is (S, T, C)
    if (!dec_fits(d.C, d.H)) {
        dss_set_error("decoder kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", d.H, d.C, DEC_MAXH, DEC_MAXC);
        return DSS_EINVAL;
    }
    if (d.O < 1 || d.O > 32) { dss_set_error("decoder kernel: %d outputs out of range (<= 32)", d.O); return DSS_EINVAL; }
    if (S < 1 || S > d.S_max || T < 1 || T > d.T_max) {
        dss_set_error("decoder kernel: %d streams x %d frames exceed the handle's %d x %d", S, T, d.S_max, d.T_max);
        return DSS_EINVAL;
    }
    dec_launch_layers(d, d_frames, frames_f64, S, T, d_counts, d_in_row, Tin, st);
    const long rows = (long)S * T;
    const size_t rlds = dec_regress_lds_floats(2 * d.H, d.O) * sizeof(float);
    hipLaunchKernelGGL(dec_regress_kernel, dim3((unsigned)((rows + DEC_RROWS - 1) / DEC_RROWS)), dim3(256), rlds, st, d.top, rows, 2 * d.H,
                       d.O, d.wr, d.br, d_feats, d_counts, T);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- a trial list (dss_dec_forward_trials_dev; the reference's validation pass, train_bidirectional_model.py:165-178) ----------
// The layers are bilstm_layer_kernel's ragged form as it is: trial s of the chunk is "row" first[s] of a buffer with ONE frame per
// row, i.e. frames first[s] + t of the concatenated (N, C) array, with counts[s] frames of its own -- so a trial's arithmetic is
// what dss_dec_forward_rows_dev gives it.  Only the regressor differs: its rows leave the padded (S, T) grid of the layer outputs
// for the trial's rows out_row[s] .. of the concatenated features (dec_regress_rows with another destination).
__global__ void __launch_bounds__(256)
dec_regress_trials_kernel(const float *__restrict__ top, long rows, int K, int O, const float *__restrict__ w, const float *__restrict__ b,
                          float *__restrict__ feats, const int *__restrict__ counts, const long long *__restrict__ out_row, int T)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];
    const long r0 = (long)blockIdx.x * DEC_RROWS;
    auto row = [&](int rr) { const long r = r0 + rr; return r < rows && (int)(r % T) < counts[r / T] ? top + r * K : nullptr; };
    bool any = false;                                      // (uniform over the block: a block of padding rows has nothing to do)
    for (int rr = 0; rr < DEC_RROWS; ++rr) any = any || row(rr);
    if (!any) return;
    dec_regress_rows(rs, K, O, w, b, row, [&](int rr, int o, float f) {
        const long r = r0 + rr;
        feats[(size_t)(out_row[r / T] + r % T) * O + o] = f;
    });
}

int dss_launch_decoder_trials(const DssDecDev &d, const void *d_frames, int frames_f64, int S, int T, float *d_feats,
                              const int *d_counts, const int *d_first, const long long *d_out_row, hipStream_t st)
{
    if (!dec_fits(d.C, d.H)) {
        dss_set_error("decoder kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", d.H, d.C, DEC_MAXH, DEC_MAXC);
        return DSS_EINVAL;
    }
    if (d.O < 1 || d.O > 32) { dss_set_error("decoder kernel: %d outputs out of range (<= 32)", d.O); return DSS_EINVAL; }
    if (S < 1 || S > d.S_max || T < 1 || T > d.T_max || !d_counts || !d_first || !d_out_row) {
        dss_set_error("decoder kernel: %d trials x %d frames exceed the handle's %d x %d", S, T, d.S_max, d.T_max);
        return DSS_EINVAL;
    }
    dec_launch_layers(d, d_frames, frames_f64, S, T, d_counts, d_first, 1, st);       // trial s: "row" first[s] of one-frame rows
    const long rows = (long)S * T;
    const size_t rlds = dec_regress_lds_floats(2 * d.H, d.O) * sizeof(float);
    hipLaunchKernelGGL(dec_regress_trials_kernel, dim3((unsigned)((rows + DEC_RROWS - 1) / DEC_RROWS)), dim3(256), rlds, st, d.top, rows,
                       2 * d.H, d.O, d.wr, d.br, d_feats, d_counts, d_out_row, T);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- a trial list over the members of a group (dss_dec_group_forward_trials_dev; Part 17) --------------------------------------
// Every trial names the member that runs it, and the weights are the members' current ones: the packed copies and master
// parameters of the group's device table of trainer descriptors (DssDecTrainDev), read in stream order behind the members' steps.
// A thread keeps its row of W_hh in registers for the whole call, so the W streams of a layer workgroup belong to ONE model: the
// workgroup table names the model and the first of its n <= W stream slots, and the body is bilstm_layer_infer as it is.  There is
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
    bilstm_layer_infer<InT, W>(in, layer ? 2 * d.H : d.C, d.H, dss_gp(d.wT[layer][dir]), dss_gp(d.b[layer][dir]), dir, out,
                              [&](int sl, int &Ts, size_t &irow, size_t &orow) {
        const bool live = sl < n;
        const DssDecGroupStream &e = st[live ? sl : 0];
        Ts = live ? e.len : 0;
        irow = (size_t)(layer ? e.buf_row : e.in_row);
        orow = (size_t)e.buf_row;
    });
}

// The regressor of such a list: dec_regress_rows once more.  A block's n <= DEC_RROWS rows of `top` belong to
// one model, whose regressor is the last two of the eighteen tensors of its master parameters (torch layout, as the inference
// handle keeps them): o_wr, o_br are their offsets.  Row r of the buffer lies in the stream slot s >= block.slot with
// buf_row <= r < buf_row + len and goes to row out_row + (r - buf_row) of the concatenated features.
__global__ void __launch_bounds__(256)
dec_regress_trials_group_kernel(const DssDecTrainDev *__restrict__ models, const DssDecGroupStream *__restrict__ streams,
                                const DssDecGroupBlock *__restrict__ blocks, const float *__restrict__ top, const int o_wr, const int o_br,
                                float *__restrict__ feats)
{
    extern __shared__ __attribute__((aligned(16))) float rs[];
    const DssDecGroupBlock &blk = *dss_cp(blocks + blockIdx.x);
    const DssDecTrainDev &d = *dss_cp(models + blk.model);
    const DssDecGroupStream *st = dss_cp(streams);
    const int K = 2 * d.H, O = d.O, nr = blk.n;
    const long long r0 = blk.row0;
    dec_regress_rows(rs, K, O, dss_gp(d.p) + o_wr, dss_gp(d.p) + o_br, [&](int rr) { return rr < nr ? top + (size_t)(r0 + rr) * K : nullptr; },
                     [&](int rr, int o, float f) {
        const long long r = r0 + rr;
        int s = blk.slot;                                  // at most DEC_RROWS - 1 streams end inside a block
        for (int j = 1; j < DEC_RROWS && r >= st[s].buf_row + st[s].len; ++j) ++s;
        feats[(size_t)(st[s].out_row + (r - st[s].buf_row)) * O + o] = f;
    });
}

int dss_launch_decoder_trials_group(const DssDecTrainDev *d_models, int C, int H, int O, const void *d_frames, int frames_f64, int W,
                                    const DssDecGroupStream *d_streams, const DssDecGroupWg *d_wgs, int n_wgs,
                                    const DssDecGroupBlock *d_blocks, int n_blocks, float *d_mid, float *d_top, float *d_feats,
                                    hipStream_t st)
{
    if (!dec_fits(C, H)) {
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
    const size_t rlds = dec_regress_lds_floats(2 * H, O) * sizeof(float);
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
    const long long off = dss_trial_row(tl, k), n = (long long)tl.len[k] * O;
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
