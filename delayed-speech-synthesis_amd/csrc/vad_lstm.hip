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

// The forward pass of one workgroup, as inference runs it: vad_forward_body (lstm_blocks.h, where the trainers' forward half finds
// it too) with labels, keeping nothing of a step; layer 1 reads layer 0's h as it is.  All three kernels below go through here.
template <typename FrameT, int SW, bool CARRY>
__device__ __forceinline__ void vad_forward_infer(const DssVadDev &v, const FrameT *__restrict__ frames, const int W, int *__restrict__ labels,
                                                  float *__restrict__ logits, const int s0, const int S)
{
    vad_forward_body<FrameT, SW, CARRY, true>(v, frames, W, labels, logits, s0, S, [](int, int, int, float) {},
                                              [](int, int, int, int, float, float, float, float, float, float h) { return h; });
}

// S streams advanced in lock-step by W frames from the handle's carried state: a workgroup owns SW of them.
template <typename FrameT, int SW>
__global__ void __launch_bounds__(VAD_THREADS)
vad_lstm_kernel(DssVadDev v, const FrameT *__restrict__ frames, int W, int *__restrict__ labels, float *__restrict__ logits)
{
    vad_forward_infer<FrameT, SW, true>(v, frames, W, labels, logits, blockIdx.x * SW, v.S);
}

int dss_launch_vad(const DssVadDev &v, const void *d_frames, int frames_f64, int W, int *d_labels, float *d_logits, hipStream_t st)
{
    if (!vad_fits(v.C, v.H)) {
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
// to rows out_row .. of the concatenated outputs.  One workgroup per trial, one stream wide: vad_forward_infer<FrameT, 1> for the
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
    vad_forward_infer<FrameT, 1, false>(v, frames + (size_t)d.in_row * v.C, d.len, labels + d.out_row,
                                        logits ? logits + (size_t)d.out_row * 2 : nullptr, 0, 1);
}

int dss_launch_vad_trials(const DssVadDev &v, const void *d_frames, int frames_f64, const DssVadTrialDesc *desc, int n_trials, int *d_labels,
                          float *d_logits, hipStream_t st)
{
    if (!vad_fits(v.C, v.H)) {
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
// runs (dss_cp: scalar loads, as for a kernel argument) and the weight pointers read from them are global pointers (vad_global_dev), so
// the weights' addresses stay in scalar registers.  v.h / v.c, the member's carried state, are not read: CARRY is off.
template <typename FrameT>
__global__ void __launch_bounds__(VAD_THREADS, 5)
vad_trials_group_kernel(const DssVadTrainDev *__restrict__ models, const FrameT *__restrict__ frames, const DssVadTrialDesc *__restrict__ desc,
                        int *__restrict__ labels, float *__restrict__ logits)
{
    const DssVadTrialDesc &d = *dss_cp(desc + blockIdx.x);
    const DssVadDev v = vad_global_dev(dss_cp(models + d.model)->v);
    vad_forward_infer<FrameT, 1, false>(v, frames + (size_t)d.in_row * v.C, d.len, labels + d.out_row,
                                        logits ? logits + (size_t)d.out_row * 2 : nullptr, 0, 1);
}

int dss_launch_vad_trials_group(const DssVadTrainDev *d_models, int C, int H, const void *d_frames, int frames_f64,
                                const DssVadTrialDesc *desc, int n_trials, int *d_labels, float *d_logits, hipStream_t st)
{
    if (!vad_fits(C, H)) {
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
    const long long off = dss_trial_row(tl, k);
    const int L = tl.len[k];
    double acc = 0.0;
    int corr = 0;
    for (int t0 = 0; t0 < L; t0 += SCORE_THREADS) {
        const int t = t0 + tid;
        if (t < L) {
            const double z0 = logits[(off + t) * 2], z1 = logits[(off + t) * 2 + 1];
            const int tg = targets[off + t];
            double lse;
            ls[tid] = lstm_cross_entropy(z0, z1, tg, lse);
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
