// csrc/vad_train.hip -- one training step of the neural voice-activity detector (gfx950): truncated backpropagation through
// time over one window, and the RMSprop update.
//
// Restates, for batch size 1 (the only one the reference's script uses),
//   train_unidirectional_vad.py:155-175   per window of T frames: forward from the carried state, nn.CrossEntropyLoss (mean
//                                         over the T frames), backward to all ten parameter tensors, optim.step(),
//                                         state.detach() -- the gradient stops at the window's initial state
//   torch.optim.RMSprop(lr, alpha, eps)   sq <- alpha sq + (1 - alpha) g^2;  p <- p - lr g / (sqrt(sq) + eps)
//   nn.LSTM(dropout = p), train mode      layer 0's output, as layer 1 reads it, times a mask of 0 or 1 / (1 - p); the mask is an
//                                         INPUT here, (T, H) multipliers or NULL -- the kernels hold no generator
// Two launches per window ("Training the detector"):
//   vad_train_window_kernel  one workgroup of 640 threads, everything that is serial in time: the forward pass (vad_forward_body
//                            of lstm_blocks.h, the loop the inference kernels run) keeping the stash the backward pass needs, the loss, dlogits,
//                            and backward through time for layer 1, then layer 0 -- the gate gradients dG1[T][4H], dG0[T][4H]
//   vad_train_step_kernel    one workgroup per gate row (and per class of the head): the weight gradients dG^T . inputs as sums
//                            over t in frame order, the bias gradients, and, fused, the RMSprop update of the master parameters
//                            (torch layout) and of the packed copies the forward pass reads
// Every sum has a fixed order and there are no atomics: the same call from the same state gives the same bits.  Fused
// multiply-adds are written out (__builtin_fmaf), as in vad_lstm.hip; the library is built with -ffp-contract=off.
// Each kernel's body is a __device__ __forceinline__ function that takes the descriptor by reference and what was a kernel
// argument or blockIdx.x as an argument, because two kernels run it: the single trainer's, and the group form at the end of this
// file, which steps several trainers in one launch (blockIdx.y is the model; DESIGN.md, "Training several detectors at once").
// The arithmetic is stated once, so a model's bits do not depend on which of the two ran it.  Every pointer read from the
// descriptor goes through dss_gp (dss_global_ptr.h): the group kernels load them from a table, and must still address global
// memory, not the flat aperture.
#include "lstm_blocks.h"

// offsets of the ten tensors in the flat parameter array (state_dict order; also of the gradients and the square averages)
struct VadTrainOff { int wih0, whh0, bih0, bhh0, wih1, whh1, bih1, bhh1, wc, bc, total; };
__host__ __device__ static inline VadTrainOff vad_train_off(int C, int H)
{
    VadTrainOff o;
    const int H4 = 4 * H;
    o.wih0 = 0;
    o.whh0 = o.wih0 + H4 * C;
    o.bih0 = o.whh0 + H4 * H;
    o.bhh0 = o.bih0 + H4;
    o.wih1 = o.bhh0 + H4;
    o.whh1 = o.wih1 + H4 * H;
    o.bih1 = o.whh1 + H4 * H;
    o.bhh1 = o.bih1 + H4;
    o.wc = o.bhh1 + H4;
    o.bc = o.wc + 2 * H;
    o.total = o.bc + 2;
    return o;
}

long dss_vad_train_param_count(int C, int H) { return vad_train_off(C, H).total; }

// W^T dg for one gate's H rows of a row-major [4H][H] matrix: output column j = sum over the gate's rows r, IN ROW ORDER, of
// W[r][j] dg[r].  Lanes run along the columns, so a wave's load is 256 consecutive bytes of one row; eight loads in flight.
__device__ __forceinline__ float vad_tdot(const float *W, int H, int j, const float *dg)
{
    float acc = 0.f;
    int r = 0;
    for (; r + 8 <= H; r += 8) {
        float w[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u] = W[(size_t)(r + u) * H + j];
#pragma unroll
        for (int u = 0; u < 8; ++u) acc = __builtin_fmaf(w[u], dg[r + u], acc);
    }
    for (; r < H; ++r) acc = __builtin_fmaf(W[(size_t)r * H + j], dg[r], acc);
    return acc;
}

// Backward through time of one layer.  Thread u < H owns unit u: dh = (what the step after this one sends through W_hh) +
// (what arrives from above: the head for layer 1, layer 1's W_ih through the mask for layer 0); dc likewise carries f dc of
// the step after.  The four gate gradients of the step go to dgs (LDS) and to dG (the workspace); then all 640 threads form
// W_hh^T dG for the step before: thread (gate q, column j) sums the H rows of gate q, and the owner adds the four parts as
// (i + f) + (g + o).  Nothing is sent below step 0: the gradient stops at the window's initial state.
template <int LAYER>
__device__ __forceinline__ void vad_bptt_layer(const DssVadTrainDev &d, const VadTrainOff &o, int T, int tid, float *dgs,
                                               float (*part)[VAD_MAXH])
{
    const int H = d.v.H, H4 = 4 * H;
    const float *act = dss_gp(LAYER ? d.act1 : d.act0), *call = dss_gp(LAYER ? d.c1 : d.c0);
    float *dG = dss_gp(LAYER ? d.dg1 : d.dg0);
    const float *p = dss_gp(d.p), *Whh = p + (LAYER ? o.whh1 : o.whh0);
    const float *dl = dss_gp(d.dl), *dh0m = dss_gp(d.dh0m);
    const int q = tid / VAD_MAXH, j = tid - q * VAD_MAXH;
    const bool own = tid < H;
    float dcn = 0.f, wc0 = 0.f, wc1 = 0.f;
    if (LAYER == 1 && own) { wc0 = p[o.wc + tid]; wc1 = p[o.wc + H + tid]; }
    for (int t = T - 1; t >= 0; --t) {
        if (own) {
            float dh = t == T - 1 ? 0.f : (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
            if (LAYER == 1) dh += __builtin_fmaf(wc1, dl[2 * t + 1], wc0 * dl[2 * t]);
            else dh += dh0m[(size_t)t * H + tid];
            const float *a = act + (size_t)t * H4;
            const float gi = a[tid], gf = a[H + tid], gg = a[2 * H + tid], go = a[3 * H + tid];
            const float c = call[(size_t)(t + 1) * H + tid], cp = call[(size_t)t * H + tid];
            const float tc = tanhf(c);
            const float dc = __builtin_fmaf(dh * go, 1.f - tc * tc, dcn);
            const float di = dc * gg * (gi * (1.f - gi));
            const float df = dc * cp * (gf * (1.f - gf));
            const float dg = dc * gi * (1.f - gg * gg);
            const float dO = dh * tc * (go * (1.f - go));
            dcn = dc * gf;
            dgs[tid] = di; dgs[H + tid] = df; dgs[2 * H + tid] = dg; dgs[3 * H + tid] = dO;
            float *g = dG + (size_t)t * H4;
            g[tid] = di; g[H + tid] = df; g[2 * H + tid] = dg; g[3 * H + tid] = dO;
        }
        __syncthreads();
        if (t > 0 && j < H) part[q][j] = vad_tdot(Whh + (size_t)q * H * H, H, j, dgs + q * H);
        __syncthreads();
    }
}

template <typename FrameT>
__device__ __forceinline__ void vad_train_window_body(const DssVadTrainDev &d, const FrameT *__restrict__ frames, const int T,
                                                      const unsigned char *__restrict__ targets, const float *__restrict__ mask,
                                                      double *__restrict__ loss)
{
    __shared__ float dgs[4 * VAD_MAXH];                                   // the gate gradients of the step in hand
    __shared__ float part[4][VAD_MAXH];                                   // W^T dG per gate, before the owner adds them
    __shared__ __attribute__((aligned(16))) float dg4[4 * VAD_MAXH][VAD_TP];     // dG1 of a chunk of frames, frames side by side
    __shared__ __attribute__((aligned(16))) float part4[4][VAD_MAXH][VAD_TP];
    const DssVadDev v = vad_global_dev(d.v);
    const int tid = threadIdx.x, C = v.C, H = v.H, H4 = 4 * H;
    const VadTrainOff o = vad_train_off(C, H);
    const bool own = tid < H, rowt = tid < H4;
    float *sh0 = dss_gp(d.h0), *sh1 = dss_gp(d.h1), *sc0 = dss_gp(d.c0), *sc1 = dss_gp(d.c1), *act0 = dss_gp(d.act0), *act1 = dss_gp(d.act1);
    float *xs = dss_gp(d.xs), *h0m = dss_gp(d.h0m), *logit = dss_gp(d.logit);

    // ---- forward: vad_forward_body (lstm_blocks.h), the loop the inference kernels run, for one stream from the carried state and
    // without labels.  Kept of a step: the frames as float32 (xs), the activated gates (row t of act), c and h behind the frame
    // (row t + 1 of the stashes; row 0 is the window's initial state) and layer 0's h times the mask (h0m), which is what layer 1
    // reads; the h a layer carries to its own next step is never masked.
    if (own) {
        sh0[tid] = v.h[tid]; sh1[tid] = v.h[H + tid]; sc0[tid] = v.c[tid]; sc1[tid] = v.c[H + tid];
    }
    vad_forward_body<FrameT, 1, true, false>(v, frames, T, nullptr, logit, 0, 1, [&](int, int t, int k, float x) { xs[(size_t)t * C + k] = x; },
                                             [&](int layer, int, int t, int u, float gi, float gf, float gg, float go, float c, float h) {
        float *a = dss_uniform((layer == 0 ? act0 : act1) + (size_t)t * H4);
        a[u] = gi; a[H + u] = gf; a[2 * H + u] = gg; a[3 * H + u] = go;
        dss_uniform((layer == 0 ? sc0 : sc1) + (size_t)(t + 1) * H)[u] = c;
        dss_uniform((layer == 0 ? sh0 : sh1) + (size_t)(t + 1) * H)[u] = h;
        if (layer != 0) return h;
        const float hm = mask ? h * dss_uniform(mask + (size_t)t * H)[u] : h;
        dss_uniform(h0m + (size_t)t * H)[u] = hm;
        return hm;
    });
    __syncthreads();

    // ---- loss and dlogits: per frame in float64 from the float32 logits, the mean summed in frame order ---------------------
    // (what only this half uses is read from the descriptor here: read in front of the forward loop, these four pointers cost the
    // group kernel, whose descriptor lives in scalar registers, 500 register reloads in that loop and 2 % of a step)
    float *dl = dss_gp(d.dl), *dh0m = dss_gp(d.dh0m);
    double *lossf = dss_gp(d.lossf);
    const float *dg1 = dss_gp(d.dg1);
    for (int t = tid; t < T; t += VAD_THREADS) {
        const double z0 = logit[2 * t], z1 = logit[2 * t + 1];
        const int tg = targets[t] ? 1 : 0;
        double lse;
        lossf[t] = lstm_cross_entropy(z0, z1, tg, lse);
        dl[2 * t] = (float)((exp(z0 - lse) - (tg ? 0.0 : 1.0)) / (double)T);
        dl[2 * t + 1] = (float)((exp(z1 - lse) - (tg ? 1.0 : 0.0)) / (double)T);
    }
    __syncthreads();
    if (tid == 0) {
        double acc = 0.0;
        for (int t = 0; t < T; ++t) acc += lossf[t];
        *loss = acc / (double)T;
    }

    // ---- backward: layer 1 through time, then what it sends down through W_ih_l1 and the mask, then layer 0 -----------------
    vad_bptt_layer<1>(d, o, T, tid, dgs, part);
    {
        const float *Wih1 = dss_gp(d.p) + o.wih1;
        const int q = tid / VAD_MAXH, j = tid - q * VAD_MAXH;
        for (int t0 = 0; t0 < T; t0 += VAD_TP) {
            const int nst = min(VAD_TP, T - t0);
            if (rowt) {
#pragma unroll
                for (int tt = 0; tt < VAD_TP; ++tt) dg4[tid][tt] = tt < nst ? dg1[(size_t)(t0 + tt) * H4 + tid] : 0.f;
            }
            __syncthreads();
            if (j < H) {
                const float *W = Wih1 + (size_t)q * H * H;
                f4 acc = {0.f, 0.f, 0.f, 0.f};
                int r = 0;
                for (; r + 4 <= H; r += 4) {
                    float w[4];
#pragma unroll
                    for (int u = 0; u < 4; ++u) w[u] = W[(size_t)(r + u) * H + j];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const f4 g = *reinterpret_cast<const f4 *>(dg4[q * H + r + u]);
                        acc.x = __builtin_fmaf(w[u], g.x, acc.x); acc.y = __builtin_fmaf(w[u], g.y, acc.y);
                        acc.z = __builtin_fmaf(w[u], g.z, acc.z); acc.w = __builtin_fmaf(w[u], g.w, acc.w);
                    }
                }
                for (; r < H; ++r) {
                    const float w = W[(size_t)r * H + j];
                    const f4 g = *reinterpret_cast<const f4 *>(dg4[q * H + r]);
                    acc.x = __builtin_fmaf(w, g.x, acc.x); acc.y = __builtin_fmaf(w, g.y, acc.y);
                    acc.z = __builtin_fmaf(w, g.z, acc.z); acc.w = __builtin_fmaf(w, g.w, acc.w);
                }
                *reinterpret_cast<f4 *>(part4[q][j]) = acc;
            }
            __syncthreads();
            if (own) {
                for (int tt = 0; tt < nst; ++tt) {
                    float s = (part4[0][tid][tt] + part4[1][tid][tt]) + (part4[2][tid][tt] + part4[3][tid][tt]);
                    if (mask) s *= mask[(size_t)(t0 + tt) * H + tid];
                    dh0m[(size_t)(t0 + tt) * H + tid] = s;
                }
            }
        }
    }
    __syncthreads();
    vad_bptt_layer<0>(d, o, T, tid, dgs, part);
}

template <typename FrameT>
__global__ void __launch_bounds__(VAD_THREADS)
vad_train_window_kernel(DssVadTrainDev d, const FrameT *__restrict__ frames, int T, const unsigned char *__restrict__ targets,
                        const float *__restrict__ mask, double *__restrict__ loss)
{
    vad_train_window_body<FrameT>(d, frames, T, targets, mask, loss);
}

// ---- the parallel part: weight gradients and the RMSprop update --------------------------------------------------------------
// Workgroup b < 8H is gate row r of layer L (b = L 4H + r): its columns are [W_ih row | W_hh row | bias], column k's gradient is
// sum over t = 0 .. T-1, in that order, of dG[t][r] in[t][k] (one fused multiply-add per frame; the bias adds dG[t][r] itself).
// Workgroups 8H and 8H + 1 are the two classes of the head: [classifier.weight row | classifier.bias] against dlogits.
// The inputs: layer 0 reads the frames (xs) and its own h of the step before (row t of h0: row 0 is the window's initial h);
// layer 1 the masked h of layer 0 (h0m) and its own h of the step before; the head h1 of the step itself (row t + 1).
// The update is evaluated per element in float64 from the stored float32 values and rounded once: inside the bounds that
// cover torch's own float32 sequence (mul, addcmul, sqrt, add, addcdiv).  bias_ih and bias_hh get the same g and each its own
// square average; the packed bias is their float32 sum.
#define VTS_THREADS 256

__device__ __forceinline__ void vad_train_step_body(const DssVadTrainDev &d, const int b, const int T, const int apply, const double lr,
                                                    const double alpha, const double eps)
{
    const int C = d.v.C, H = d.v.H, H4 = 4 * H;
    const VadTrainOff o = vad_train_off(C, H);
    const bool head = b >= 2 * H4;
    const int L = head ? 2 : b / H4, r = head ? b - 2 * H4 : b - L * H4;
    LstmStepRow w;
    w.dg = dss_gp(head ? d.dl : (L ? d.dg1 : d.dg0)) + r;
    w.dgs = head ? 2 : H4;
    w.inA = dss_gp(head ? d.h1 + H : (L ? d.h0m : d.xs));
    w.nA = head || L ? H : C;              // (two columns per thread: at most 128 + 160 + 1 columns)
    w.inB = dss_gp(L ? d.h1 : d.h0);
    w.nB = head ? 0 : H;
    w.strideB = H;
    w.o_A = (head ? o.wc : (L ? o.wih1 : o.wih0)) + r * w.nA;
    w.o_B = (L ? o.whh1 : o.whh0) + r * H;
    w.o_bias = head ? o.bc + r : (L ? o.bih1 : o.bih0) + r;
    w.o_bias2 = (L ? o.bhh1 : o.bhh0) + r;
    w.wpk = head ? nullptr : dss_gp(L ? d.wT1 : d.wT0);
    w.bpk = dss_gp(L ? d.b1 : d.b0) + r;
    w.r = r; w.H4 = H4; w.kB = (w.nA + 3) & ~3;
    lstm_train_step_row<VTS_THREADS>(w, dss_gp(d.p), dss_gp(d.sq), dss_gp(d.g), T, apply, lr, alpha, eps);
}

__global__ void __launch_bounds__(VTS_THREADS)
vad_train_step_kernel(DssVadTrainDev d, int T, int apply, double lr, double alpha, double eps)
{
    vad_train_step_body(d, blockIdx.x, T, apply, lr, alpha, eps);
}

int dss_launch_vad_train_window(const DssVadTrainDev &d, const void *d_frames, int frames_f64, int T, const unsigned char *d_targets,
                                const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss, hipStream_t st)
{
    const int H = d.v.H, C = d.v.C;
    if (!vad_fits(C, H) || T < 1 || T > d.Tmax) {
        dss_set_error("VAD training kernel: %d hidden units / %d inputs / %d frames out of range (<= %d / <= %d / <= %d)", H, C, T,
                      VAD_MAXH, VAD_MAXC, d.Tmax);
        return DSS_EINVAL;
    }
    if (frames_f64) hipLaunchKernelGGL((vad_train_window_kernel<double>), dim3(1), dim3(VAD_THREADS), 0, st, d, (const double *)d_frames, T, d_targets, d_mask, d_loss);
    else hipLaunchKernelGGL((vad_train_window_kernel<float>), dim3(1), dim3(VAD_THREADS), 0, st, d, (const float *)d_frames, T, d_targets, d_mask, d_loss);
    DSS_HIP_CHECK(hipGetLastError());
    hipLaunchKernelGGL(vad_train_step_kernel, dim3(8 * H + 2), dim3(VTS_THREADS), 0, st, d, T, apply_step, lr, alpha, eps);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- several trainers in one launch (Part 15) ---------------------------------------------------------------------------------
// The same two launches with a model axis: blockIdx.y is the model, blockIdx.x keeps its meaning.  A workgroup reads its model's
// descriptor from a device table of M and its model's entry of the step's trial table (uniform addresses: scalar loads), then runs
// the body the single-trainer kernel runs, so a model's numbers do not depend on M, on its place in the group or on what the others
// do.  The entry describes a whole trial; the launch says which window of it: window w of `window` frames is frames t0 = w * window
// .. t0 + T of the trial, T = min(window, len - t0), its masks and targets from row t0 on, its loss in losses[w].  T <= 0 is a model
// that sits the step out (len == 0) or whose trial has run out: the test is uniform over the workgroup and comes before the first
// store and the first barrier, so nothing of that model is written.  Both tables are constant while a launch runs (dss_cp).
// The window kernel is held to the single trainer's six waves per SIMD (amdgpu_waves_per_eu): with the descriptor coming from a
// table the scheduler otherwise settles for four and spends the registers (118 VGPRs for the same instructions).
__device__ __forceinline__ int vad_group_window_frames(const DssVadGroupTrial &tr, int w, int window)
{
    return (int)min((long long)window, (long long)tr.len - (long long)w * window);
}

template <typename FrameT>
__global__ void __launch_bounds__(VAD_THREADS) __attribute__((amdgpu_waves_per_eu(6)))
vad_group_window_kernel(const DssVadTrainDev *__restrict__ models, const DssVadGroupTrial *__restrict__ trials, int w, int window)
{
    const DssVadGroupTrial &tr = *dss_cp(trials + blockIdx.y);
    const int T = vad_group_window_frames(tr, w, window);
    if (T <= 0) return;
    const DssVadTrainDev &d = *dss_cp(models + blockIdx.y);
    const size_t t0 = (size_t)w * window;
    vad_train_window_body<FrameT>(d, dss_gp((const FrameT *)tr.frames) + t0 * d.v.C, T, dss_gp(tr.targets) + t0,
                                  tr.mask ? dss_gp(tr.mask) + t0 * d.v.H : (const float *)nullptr, dss_gp(tr.losses) + w);
}

__global__ void __launch_bounds__(VTS_THREADS)
vad_group_step_kernel(const DssVadTrainDev *__restrict__ models, const DssVadGroupTrial *__restrict__ trials, int w, int window)
{
    const DssVadGroupTrial &tr = *dss_cp(trials + blockIdx.y);
    const int T = vad_group_window_frames(tr, w, window);
    if (T <= 0) return;
    const DssVadTrainDev &d = *dss_cp(models + blockIdx.y);
    vad_train_step_body(d, blockIdx.x, T, tr.apply, tr.lr, tr.alpha, tr.eps);
}

// a new trial: zeros in the carried (h, c), [2 layers][H] each, of every model that takes part in the step
__global__ void __launch_bounds__(VTS_THREADS)
vad_group_reset_kernel(const DssVadTrainDev *__restrict__ models, const DssVadGroupTrial *__restrict__ trials)
{
    if (dss_cp(trials + blockIdx.x)->len <= 0) return;
    const DssVadTrainDev &d = *dss_cp(models + blockIdx.x);
    float *h = dss_gp(d.v.h), *c = dss_gp(d.v.c);
    for (int k = threadIdx.x; k < 2 * d.v.H; k += VTS_THREADS) { h[k] = 0.f; c[k] = 0.f; }
}

int dss_launch_vad_train_group(const DssVadTrainDev *d_models, const DssVadGroupTrial *d_trials, int M, int C, int H, int n_windows,
                               int window, int reset, int frames_f64, hipStream_t st)
{
    if (M < 1 || M > DSS_VAD_GROUP_MAXM || !vad_fits(C, H) || n_windows < 1 || window < 1 || window > DSS_VAD_TRAIN_MAXT) {
        dss_set_error("VAD group kernels: %d models / %d hidden units / %d inputs / %d windows of %d frames out of range (<= %d / <= %d / <= %d / >= 1 / <= %d)",
                      M, H, C, n_windows, window, DSS_VAD_GROUP_MAXM, VAD_MAXH, VAD_MAXC, DSS_VAD_TRAIN_MAXT);
        return DSS_EINVAL;
    }
    if (reset) {
        hipLaunchKernelGGL(vad_group_reset_kernel, dim3(M), dim3(VTS_THREADS), 0, st, d_models, d_trials);
        DSS_HIP_CHECK(hipGetLastError());
    }
    for (int w = 0; w < n_windows; ++w) {
        if (frames_f64) hipLaunchKernelGGL((vad_group_window_kernel<double>), dim3(1, M), dim3(VAD_THREADS), 0, st, d_models, d_trials, w, window);
        else hipLaunchKernelGGL((vad_group_window_kernel<float>), dim3(1, M), dim3(VAD_THREADS), 0, st, d_models, d_trials, w, window);
        DSS_HIP_CHECK(hipGetLastError());
        hipLaunchKernelGGL(vad_group_step_kernel, dim3(8 * H + 2, M), dim3(VTS_THREADS), 0, st, d_models, d_trials, w, window);
        DSS_HIP_CHECK(hipGetLastError());
    }
    return DSS_OK;
}
