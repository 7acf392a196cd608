// csrc/vad_lstm.hip -- the neural voice-activity detector of the online path for many streams per launch (gfx950).
//
// Restates, for S independent streams advanced in lock-step by W frames per call (one amplifier packet = 4 frames),
//   UnidirectionalVoiceActivityDetector.forward     local/models.py:11-33   LSTM(C -> H) -> LSTM(H -> H) -> Linear(H -> 2)
//   FilterSpeechSegments.process, the model call    local/units.py:432-434  logits per frame, argmax -> raw speech label,
//                                                                           (h, c) of both layers carried across packets
// The reference runs torch.nn.LSTM; its arithmetic is torch's, not a fixed C sequence, so parity here is tolerance-level
// (the test states it: |logit - torch| <= 2e-5 on the reference-generated golden vector, equal labels on random frames) and
// fused multiply-adds are allowed -- unlike everywhere else in this library.  Gate order i, f, g, o (torch.nn.LSTM).
//
// One launch per tick instead of MIOpen's chain of small launches per layer and frame: a 640-thread workgroup owns SW (1 or 2)
// streams for the whole call; thread t owns gate row t (4H = 600 rows) of the layer being stepped and runs the row's
// dot product for all SW streams at once: the weights (copies with four consecutive inputs of a row side by side: one
// 16-byte load per lane, 1 KB of consecutive bytes per wave) come from L2 once per workgroup, the inputs of the SW
// streams from LDS as broadcast reads.  h lives in LDS, c
// in the registers of the thread that owns (stream, unit).  The time steps and the two layers are sequential; streams x
// gate rows are the parallel axes.  Weights 1.24 MB fp32 for H = 150: L2-resident after the first workgroup has read them.
#include "lstm_blocks.h"

// The forward pass of one workgroup: SW streams, W frames each, through both layers and the classifier.  Stream s of the call
// (s0 <= s < min(s0 + SW, S)) reads frames[(s * W + w) * C ..] and writes labels[s * W + w] and, unless logits is NULL,
// logits[(s * W + w) * 2 ..].  CARRY: (h, c) of both layers come from the handle and go back to it; otherwise the streams start
// from zeros (create_new_initial_state, models.py:22-24) and the handle's state is not touched.  Both kernels below run this
// body, so a frame's bits do not depend on which of them stepped it.
template <typename FrameT, int SW, bool CARRY>
__device__ __forceinline__ void vad_forward_body(const DssVadDev &v, const FrameT *__restrict__ frames, const int W, int *__restrict__ labels,
                                                 float *__restrict__ logits, const int s0, const int S)
{
    typedef typename LstmVec<SW>::type V;
    __shared__ __attribute__((aligned(16))) V xin[VAD_TP][VAD_MAXC];      // [frame of the chunk][input][stream of this workgroup]
    __shared__ __attribute__((aligned(16))) V h0s[VAD_TP][VAD_MAXH];      // layer 0's h of the chunk's frames (layer 1's inputs)
    __shared__ __attribute__((aligned(16))) V hs[2][VAD_MAXH];            // [layer][unit][stream]; units H .. Hp-1 stay zero
    __shared__ __attribute__((aligned(16))) V gates[4 * VAD_MAXH];        // [gate row][stream]
    __shared__ float lg[SW][2];
    const int tid = threadIdx.x, C = v.C, H = v.H, H4 = 4 * H;
    const int Cp = (C + 3) & ~3, Hp = (H + 3) & ~3;        // the padded input counts the weight copies were built for
    // the (stream, unit) this thread owns in the cell updates
    const int cs = SW == 1 ? 0 : tid / H, cu = tid - cs * H;
    const bool cell = tid < SW * H && s0 + cs < S;
    float c0 = 0.f, c1 = 0.f;
    for (int k = tid; k < 2 * VAD_MAXH * SW; k += VAD_THREADS) reinterpret_cast<float *>(hs)[k] = 0.f;
    for (int k = tid; k < VAD_TP * VAD_MAXH * SW; k += VAD_THREADS) reinterpret_cast<float *>(h0s)[k] = 0.f;
    for (int k = tid; k < VAD_TP * VAD_MAXC * SW; k += VAD_THREADS) reinterpret_cast<float *>(xin)[k] = 0.f;
    __syncthreads();
    if (CARRY && cell) {
        const size_t o = (size_t)(s0 + cs) * H + cu;
        reinterpret_cast<float *>(&hs[0][cu])[cs] = v.h[o];
        reinterpret_cast<float *>(&hs[1][cu])[cs] = v.h[(size_t)S * H + o];
        c0 = v.c[o]; c1 = v.c[(size_t)S * H + o];
    }
    const bool rowt = tid < H4;
    const float bias0 = rowt ? v.b0[tid] : 0.f, bias1 = rowt ? v.b1[tid] : 0.f;

    // Layer by layer over chunks of VAD_TP frames: a layer's recurrence is serial in time, the input halves of its gates are not --
    // one pass over W_ih forms them for all frames of the chunk (each gets the same terms in the same order as a frame on its
    // own), and a step then adds only W_hh h.  Layer 1's inputs are layer 0's h of the chunk's frames (h0s).
    for (int w0 = 0; w0 < W; w0 += VAD_TP) {
        const int nst = min(VAD_TP, W - w0);
        for (int idx = tid; idx < nst * C * SW; idx += VAD_THREADS) {       // the chunk's inputs (units.py:433: frames as float32)
            const int tt = idx / (C * SW), rem = idx - tt * (C * SW);
            const int sl = rem / C, k = rem - sl * C;
            reinterpret_cast<float *>(&xin[tt][k])[sl] = (s0 + sl < S) ? (float)frames[((size_t)(s0 + sl) * W + w0 + tt) * C + k] : 0.f;
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
                    const float h = lstm_cell(gi, gf, gg, go, layer == 0 ? c0 : c1);
                    reinterpret_cast<float *>(&hs[layer][cu])[cs] = h;
                    if (layer == 0) reinterpret_cast<float *>(&h0s[tt][cu])[cs] = h;
                }
                __syncthreads();
                if (layer == 1) {
                    // ---- classifier (models.py:20,32) and the raw label (units.py:434: argmax, the first maximum wins: equal
                    // logits are non-speech)
                    const int w = w0 + tt;
                    if (tid < SW * 2) {
                        const int sl = tid >> 1, cls = tid & 1;
                        float a = 0.f;
                        for (int k = 0; k < H; ++k) a = __builtin_fmaf(v.wc[cls * H + k], reinterpret_cast<const float *>(&hs[1][k])[sl], a);
                        a += v.bc[cls];
                        lg[sl][cls] = a;
                        if (logits && s0 + sl < S) logits[((size_t)(s0 + sl) * W + w) * 2 + cls] = a;
                    }
                    __syncthreads();
                    if (tid < SW && s0 + tid < S) labels[(size_t)(s0 + tid) * W + w] = lg[tid][1] > lg[tid][0] ? 1 : 0;
                }
            }
        }
    }
    if (CARRY && cell) {
        const size_t o = (size_t)(s0 + cs) * H + cu;
        v.h[o] = reinterpret_cast<const float *>(&hs[0][cu])[cs];
        v.h[(size_t)S * H + o] = reinterpret_cast<const float *>(&hs[1][cu])[cs];
        v.c[o] = c0;
        v.c[(size_t)S * H + o] = c1;
    }
}

// S streams advanced in lock-step by W frames from the handle's carried state: a workgroup owns SW of them.
template <typename FrameT, int SW>
__global__ void __launch_bounds__(VAD_THREADS)
vad_lstm_kernel(DssVadDev v, const FrameT *__restrict__ frames, int W, int *__restrict__ labels, float *__restrict__ logits)
{
    vad_forward_body<FrameT, SW, true>(v, frames, W, labels, logits, blockIdx.x * SW, v.S);
}

int dss_launch_vad(const DssVadDev &v, const void *d_frames, int frames_f64, int W, int *d_labels, float *d_logits, hipStream_t st)
{
    if (v.H < 1 || v.H > VAD_MAXH || 4 * v.H > VAD_THREADS || v.C < 1 || v.C > VAD_MAXC || 2 * v.H > VAD_THREADS) {
        dss_set_error("VAD kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", v.H, v.C, VAD_MAXH, VAD_MAXC);
        return DSS_EINVAL;
    }
    const dim3 block(VAD_THREADS);
    const int Wsel = v.S <= 256 ? 1 : 2;         // one stream per workgroup while that leaves no CU without work for long
#define VAD_LAUNCH(FT, WV) hipLaunchKernelGGL((vad_lstm_kernel<FT, WV>), dim3((v.S + WV - 1) / WV), block, 0, st, v, (const FT *)d_frames, W, d_labels, d_logits)
    if (frames_f64) { if (Wsel == 1) VAD_LAUNCH(double, 1); else VAD_LAUNCH(double, 2); }
    else { if (Wsel == 1) VAD_LAUNCH(float, 1); else VAD_LAUNCH(float, 2); }
#undef VAD_LAUNCH
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- a trial list in one launch (dss_vad_forward_trials_dev; the reference's validation pass, train_unidirectional_vad.py:181-215) ----
// Trial k is rows in_row .. in_row + len of one (N, C) array and starts from the zero state of both layers; its labels and logits go
// to rows out_row .. of the concatenated outputs.  One workgroup per trial, one stream wide: vad_forward_body<FrameT, 1> for the
// only stream of a call of len frames, so a trial's results are the bits vad_lstm_kernel<FrameT, 1> gives a one-stream handle
// stepped through all len frames in one call.  The table comes sorted longest trial first: workgroups are dispatched in index
// order, so the long trials start first and the short ones fill the CUs they leave (a trial is a serial chain of len steps;
// nothing else balances it).  The handle's persistent (h, c) are not touched: h lives in LDS and c in registers for the length of
// the trial.

template <typename FrameT>
__global__ void __launch_bounds__(VAD_THREADS, 5)         // 5 waves per SIMD = two trials per CU: one hides the other's L2 and barrier waits
vad_trials_kernel(DssVadDev v, const FrameT *__restrict__ frames, const DssVadTrialDesc *__restrict__ desc, int *__restrict__ labels,
                  float *__restrict__ logits)
{
    const DssVadTrialDesc d = desc[blockIdx.x];
    vad_forward_body<FrameT, 1, false>(v, frames + (size_t)d.in_row * v.C, d.len, labels + d.out_row,
                                       logits ? logits + (size_t)d.out_row * 2 : nullptr, 0, 1);
}

int dss_launch_vad_trials(const DssVadDev &v, const void *d_frames, int frames_f64, const DssVadTrialDesc *desc, int n_trials, int *d_labels,
                          float *d_logits, hipStream_t st)
{
    if (v.H < 1 || v.H > VAD_MAXH || 4 * v.H > VAD_THREADS || v.C < 1 || v.C > VAD_MAXC) {
        dss_set_error("VAD kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", v.H, v.C, VAD_MAXH, VAD_MAXC);
        return DSS_EINVAL;
    }
    if (n_trials < 1) return DSS_OK;
    if (frames_f64) hipLaunchKernelGGL((vad_trials_kernel<double>), dim3(n_trials), dim3(VAD_THREADS), 0, st, v, (const double *)d_frames, desc, d_labels, d_logits);
    else hipLaunchKernelGGL((vad_trials_kernel<float>), dim3(n_trials), dim3(VAD_THREADS), 0, st, v, (const float *)d_frames, desc, d_labels, d_logits);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- a trial list over the members of a group (dss_vad_group_forward_trials_dev; Part 17) --------------------------------------
// The same launch with a model per trial: the workgroup takes its entry of the trial table, then the detector of the member the
// entry names from the group's device table of trainer descriptors (DssVadTrainDev::v: the packed copies the trainer's forward
// half reads, so the weights are the member's current ones, in stream order behind its steps), and runs the body vad_trials_kernel
// runs -- a trial's bits are those of a VadLstmGPU holding that member's weights.  Both tables are constant while the launch
// runs (dss_cp: scalar loads, as for a kernel argument) and the weight pointers read from them are global pointers (dss_gp), so
// the weights' addresses stay in scalar registers.  v.h / v.c, the member's carried state, are not passed on: CARRY is off.
template <typename FrameT>
__global__ void __launch_bounds__(VAD_THREADS, 5)
vad_trials_group_kernel(const DssVadTrainDev *__restrict__ models, const FrameT *__restrict__ frames, const DssVadTrialDesc *__restrict__ desc,
                        int *__restrict__ labels, float *__restrict__ logits)
{
    const DssVadTrialDesc &d = *dss_cp(desc + blockIdx.x);
    const DssVadDev &t = dss_cp(models + d.model)->v;
    DssVadDev v;
    v.S = 1; v.C = t.C; v.H = t.H;
    v.wT0 = dss_gp(t.wT0); v.b0 = dss_gp(t.b0); v.wT1 = dss_gp(t.wT1); v.b1 = dss_gp(t.b1); v.wc = dss_gp(t.wc); v.bc = dss_gp(t.bc);
    v.h = nullptr; v.c = nullptr;
    vad_forward_body<FrameT, 1, false>(v, frames + (size_t)d.in_row * v.C, d.len, labels + d.out_row,
                                       logits ? logits + (size_t)d.out_row * 2 : nullptr, 0, 1);
}

int dss_launch_vad_trials_group(const DssVadTrainDev *d_models, int C, int H, const void *d_frames, int frames_f64,
                                const DssVadTrialDesc *desc, int n_trials, int *d_labels, float *d_logits, hipStream_t st)
{
    if (H < 1 || H > VAD_MAXH || 4 * H > VAD_THREADS || C < 1 || C > VAD_MAXC) {
        dss_set_error("VAD kernel: hidden size %d / %d inputs out of range (<= %d / <= %d)", H, C, VAD_MAXH, VAD_MAXC);
        return DSS_EINVAL;
    }
    if (n_trials < 1) return DSS_OK;
    if (frames_f64) hipLaunchKernelGGL((vad_trials_group_kernel<double>), dim3(n_trials), dim3(VAD_THREADS), 0, st, d_models, (const double *)d_frames, desc, d_labels, d_logits);
    else hipLaunchKernelGGL((vad_trials_group_kernel<float>), dim3(n_trials), dim3(VAD_THREADS), 0, st, d_models, (const float *)d_frames, desc, d_labels, d_logits);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}

// ---- scoring a trial list (dss_vad_score_trials_dev): what the validation pass derives from the logits of a trial --------------
// Per frame, in float64 from the float32 logits: loss = logsumexp(z) - z[target] (nn.CrossEntropyLoss), prob = softmax(z)[1].
// Per trial: the mean of the losses, summed IN FRAME ORDER by one thread (tiles of 256 frames go through LDS), and the number of
// frames whose label equals the target.  One workgroup per trial; the launch's trials and their lengths travel as kernel
// arguments (DssTrialLens), so the entry point needs no handle and no device scratch.
#define SCORE_THREADS 256
__global__ void __launch_bounds__(SCORE_THREADS)
vad_score_trials_kernel(DssTrialLens tl, const float *__restrict__ logits, const int *__restrict__ labels,
                        const unsigned char *__restrict__ targets, double *__restrict__ loss, int *__restrict__ correct,
                        float *__restrict__ prob)
{
    __shared__ double ls[SCORE_THREADS];
    __shared__ int cs[SCORE_THREADS];
    const int tid = threadIdx.x, k = blockIdx.x;
    long long off = tl.base;
    for (int j = 0; j < k; ++j) off += tl.len[j];
    const int L = tl.len[k];
    double acc = 0.0;
    int corr = 0;
    for (int t0 = 0; t0 < L; t0 += SCORE_THREADS) {
        const int t = t0 + tid;
        if (t < L) {
            const double z0 = logits[(off + t) * 2], z1 = logits[(off + t) * 2 + 1];
            const int tg = targets[off + t];
            const double m = fmax(z0, z1);
            const double lse = m + log(exp(z0 - m) + exp(z1 - m));
            ls[tid] = lse - (tg ? z1 : z0);
            cs[tid] = labels[off + t] == tg ? 1 : 0;
            if (prob) prob[off + t] = (float)exp(z1 - lse);
        }
        __syncthreads();
        if (tid == 0) {
            const int n = min(SCORE_THREADS, L - t0);
            for (int j = 0; j < n; ++j) { acc += ls[j]; corr += cs[j]; }
        }
        __syncthreads();
    }
    if (tid == 0) { loss[tl.first_trial + k] = acc / (double)L; correct[tl.first_trial + k] = corr; }
}

int dss_launch_vad_score_trials(const DssTrialLens &tl, const float *d_logits, const int *d_labels, const unsigned char *d_targets,
                                double *d_loss, int *d_correct, float *d_prob, hipStream_t st)
{
    hipLaunchKernelGGL(vad_score_trials_kernel, dim3(tl.n), dim3(SCORE_THREADS), 0, st, tl, d_logits, d_labels, d_targets, d_loss, d_correct, d_prob);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
