// csrc/dss_vad.cpp -- host side of the neural voice-activity detector (Part 5 of include/dss_hip.h; csrc/vad_lstm.hip) and of
// its trial-list forms (Part 8).
#include <string.h>

#include <vector>

#include "dss_host.h"

// ------------------------------------------------------------------------------------------------------
// neural voice-activity detector (Part 5 of include/dss_hip.h; csrc/vad_lstm.hip)
// ------------------------------------------------------------------------------------------------------
struct dss_vad {
    int device;
    DssVadDev d;
    DssDevBlocks blocks;
    float *w[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // wT0, b0, wT1, b1, wc, bc
    bool loaded = false;
    // trial lists (dss_vad_forward_trials_dev): the descriptor table of the last call, pinned staging and device
    DssPinnedStage tstage;
    DssDevArray<DssVadTrialDesc> d_tdesc;
};

int dss_vad_device_weights(dss_vad *v, int *device, int *n_inputs, int *hidden_units, float *w[6])
{
    if (!v || !v->loaded) { dss_set_error("the detector handle is NULL or has no weights loaded (dss_vad_load_weights)"); return DSS_EINVAL; }
    *device = v->device; *n_inputs = v->d.C; *hidden_units = v->d.H;
    for (int k = 0; k < 6; ++k) w[k] = v->w[k];
    return DSS_OK;
}

extern "C" dss_vad *dss_vad_create(int n_streams, int n_inputs, int hidden_units)
{
    if (n_streams <= 0 || n_inputs <= 0 || hidden_units <= 0) { dss_set_error("VAD dims must be positive"); return nullptr; }
    if (hidden_units > DSS_VAD_MAXH || n_inputs > DSS_VAD_MAXC) {
        dss_set_error("VAD kernel: %d hidden units / %d inputs out of range (<= %d / <= %d)", hidden_units, n_inputs, DSS_VAD_MAXH, DSS_VAD_MAXC);
        return nullptr;
    }
    if (dss_ensure_device()) return nullptr;
    dss_vad *v = new dss_vad;
    memset(&v->d, 0, sizeof(v->d));
    hipGetDevice(&v->device);
    v->d.S = n_streams; v->d.C = n_inputs; v->d.H = hidden_units;
    const size_t n = (size_t)2 * n_streams * hidden_units;
    if (v->blocks.alloc<float>(n, &v->d.h) || v->blocks.alloc<float>(n, &v->d.c) || hipMemset(v->d.h, 0, n * sizeof(float)) != hipSuccess ||
        hipMemset(v->d.c, 0, n * sizeof(float)) != hipSuccess) {
        dss_set_error("device allocation failed for the VAD state");
        dss_vad_destroy(v);
        return nullptr;
    }
    return v;
}

extern "C" void dss_vad_destroy(dss_vad *v)
{
    if (!v) return;
    hipSetDevice(v->device);
    v->blocks.free_all();
    v->tstage.destroy();
    delete v;
}

// torch.nn.LSTM parameter layout (host arrays): weight_ih_l0 [4H][C], weight_hh_l0 [4H][H], bias_ih_l0 / bias_hh_l0 [4H],
// weight_ih_l1 [4H][H], weight_hh_l1 [4H][H], bias_ih_l1 / bias_hh_l1 [4H], classifier weight [2][H] and bias [2]
extern "C" int dss_vad_load_weights(dss_vad *v, const float *w_ih0, const float *w_hh0, const float *b_ih0, const float *b_hh0,
                                    const float *w_ih1, const float *w_hh1, const float *b_ih1, const float *b_hh1,
                                    const float *cls_w, const float *cls_b)
{
    if (!v || !w_ih0 || !w_hh0 || !b_ih0 || !b_hh0 || !w_ih1 || !w_hh1 || !b_ih1 || !b_hh1 || !cls_w || !cls_b) {
        dss_set_error("dss_vad_load_weights: null argument"); return DSS_EINVAL;
    }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    const int C = v->d.C, H = v->d.H, H4 = 4 * H, Cp = (C + 3) & ~3, Hp = (H + 3) & ~3;
    // the kernel's copies: [inputs / 4][4H rows][4 consecutive inputs], input counts padded to multiples of 4 with zero weights
    std::vector<float> t0((size_t)(Cp + Hp) * H4, 0.f), t1((size_t)2 * Hp * H4, 0.f), b0(H4), b1(H4);
    dss_pack_rows(t0.data(), H4, 0, w_ih0, C);
    dss_pack_rows(t0.data(), H4, Cp, w_hh0, H);
    dss_pack_rows(t1.data(), H4, 0, w_ih1, H);
    dss_pack_rows(t1.data(), H4, Hp, w_hh1, H);
    for (int r = 0; r < H4; ++r) {
        b0[r] = b_ih0[r] + b_hh0[r];
        b1[r] = b_ih1[r] + b_hh1[r];
    }
    // upload beside the weights in use and switch only when every array has arrived: a failed load leaves the detector
    // as it was (an earlier model keeps running; without one, `loaded` stays false)
    float *nw[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = v->blocks.upload<float>(t0.data(), t0.size(), &nw[0]);
    rc |= v->blocks.upload<float>(b0.data(), b0.size(), &nw[1]);
    rc |= v->blocks.upload<float>(t1.data(), t1.size(), &nw[2]);
    rc |= v->blocks.upload<float>(b1.data(), b1.size(), &nw[3]);
    rc |= v->blocks.upload<float>(cls_w, (size_t)2 * H, &nw[4]);
    rc |= v->blocks.upload<float>(cls_b, 2, &nw[5]);
    if (rc) { for (float *p : nw) v->blocks.release(p); return DSS_ENOMEM; }
    DSS_HIP_CHECK(hipDeviceSynchronize());                    // no launch may still read the arrays about to be freed
    for (int k = 0; k < 6; ++k) { v->blocks.release(v->w[k]); v->w[k] = nw[k]; }
    v->d.wT0 = v->w[0]; v->d.b0 = v->w[1]; v->d.wT1 = v->w[2]; v->d.b1 = v->w[3]; v->d.wc = v->w[4]; v->d.bc = v->w[5];
    v->loaded = true;
    return DSS_OK;
}

// zero the recurrent state of one stream (create_new_initial_state, models.py:22-24), or of all (stream < 0)
extern "C" int dss_vad_reset(dss_vad *v, int stream)
{
    if (!v || stream >= v->d.S) { dss_set_error("bad VAD / stream"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    const size_t SH = (size_t)v->d.S * v->d.H, H = v->d.H;
    for (float *p : {v->d.h, v->d.c}) {
        if (stream < 0) { DSS_HIP_CHECK(hipMemset(p, 0, 2 * SH * sizeof(float))); continue; }
        for (int layer = 0; layer < 2; ++layer) DSS_HIP_CHECK(hipMemset(p + layer * SH + (size_t)stream * H, 0, H * sizeof(float)));
    }
    return DSS_OK;
}

// the same, enqueued on the stream the steps run on (dss_vad_reset uses the null stream and waits: it is ordered against
// steps on a blocking stream only)
extern "C" int dss_vad_reset_async(dss_vad *v, int stream, void *hip_stream)
{
    if (!v || stream >= v->d.S) { dss_set_error("bad VAD / stream"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t SH = (size_t)v->d.S * v->d.H, H = v->d.H;
    for (float *p : {v->d.h, v->d.c}) {
        if (stream < 0) { DSS_HIP_CHECK(hipMemsetAsync(p, 0, 2 * SH * sizeof(float), st)); continue; }
        for (int layer = 0; layer < 2; ++layer) DSS_HIP_CHECK(hipMemsetAsync(p + layer * SH + (size_t)stream * H, 0, H * sizeof(float), st));
    }
    return DSS_OK;
}

// d_frames: (S, n_frames, C) float64 (frames_are_f64, as the extractor returns them) or float32; d_labels: (S, n_frames) int32;
// d_logits: (S, n_frames, 2) float32 or NULL.  All device pointers; asynchronous on hip_stream.
extern "C" int dss_vad_step_dev(dss_vad *v, const void *d_frames, int frames_are_f64, int n_frames, int *d_labels, float *d_logits,
                                void *hip_stream)
{
    if (!v || !d_frames || !d_labels || n_frames <= 0) { dss_set_error("dss_vad_step_dev: bad arguments"); return DSS_EINVAL; }
    if (!v->loaded) { dss_set_error("dss_vad_step_dev: no weights loaded (dss_vad_load_weights)"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    return dss_launch_vad(v->d, d_frames, frames_are_f64, n_frames, d_labels, d_logits, (hipStream_t)hip_stream);
}

// host copies of the recurrent state, [2 layers][S][H] each (either may be NULL); set == 0 reads, set != 0 writes
extern "C" int dss_vad_state(dss_vad *v, float *h, float *c, int set)
{
    if (!v) return DSS_EINVAL;
    DSS_HIP_CHECK(hipSetDevice(v->device));
    const size_t n = (size_t)2 * v->d.S * v->d.H * sizeof(float);
    DSS_HIP_CHECK(hipDeviceSynchronize());
    if (h) DSS_HIP_CHECK(set ? hipMemcpy(v->d.h, h, n, hipMemcpyHostToDevice) : hipMemcpy(h, v->d.h, n, hipMemcpyDeviceToHost));
    if (c) DSS_HIP_CHECK(set ? hipMemcpy(v->d.c, c, n, hipMemcpyHostToDevice) : hipMemcpy(c, v->d.c, n, hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_vad_forward_trials_dev(dss_vad *v, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                                          const long long *first, const int *len, int *d_labels, float *d_logits, void *hip_stream)
{
    if (!v || !d_frames || !d_labels) { dss_set_error("dss_vad_forward_trials_dev: bad arguments"); return DSS_EINVAL; }
    if (!v->loaded) { dss_set_error("dss_vad_forward_trials_dev: no weights loaded (dss_vad_load_weights)"); return DSS_EINVAL; }
    long long total = 0;
    int rc = dss_trials_check(N, n_trials, first, len, &total);
    if (rc) return rc;
    if (!n_trials) return DSS_OK;
    DSS_HIP_CHECK(hipSetDevice(v->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const std::vector<long long> out_row = trials_offsets(n_trials, [&](int i) { return len[i]; });
    const std::vector<int> order = trials_longest_first(n_trials, len);
    DssVadTrialDesc *desc = (DssVadTrialDesc *)v->tstage.acquire(sizeof(DssVadTrialDesc) * (size_t)n_trials);
    if (!desc) { dss_set_error("pinned staging for the trial table failed"); return DSS_ENOMEM; }
    for (int k = 0; k < n_trials; ++k) { const int i = order[k]; desc[k] = DssVadTrialDesc{first[i], out_row[i], len[i], 0}; }
    rc = v->d_tdesc.grow(v->blocks, (size_t)n_trials);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpyAsync(v->d_tdesc, desc, sizeof(DssVadTrialDesc) * (size_t)n_trials, hipMemcpyHostToDevice, st));
    if ((rc = v->tstage.commit(st))) return rc;
    return dss_launch_vad_trials(v->d, d_frames, frames_are_f64, v->d_tdesc, n_trials, d_labels, d_logits, st);
}

extern "C" int dss_vad_score_trials_dev(const float *d_logits, const int *d_labels, const unsigned char *d_targets, int n_trials,
                                        const int *len, double *d_loss, int *d_correct, float *d_prob, void *hip_stream)
{
    if (!d_logits || !d_labels || !d_targets || !d_loss || !d_correct) { dss_set_error("dss_vad_score_trials_dev: null argument"); return DSS_EINVAL; }
    return trials_reduce("dss_vad_score_trials_dev", n_trials, len, [&](const DssTrialLens &tl) {
        return dss_launch_vad_score_trials(tl, d_logits, d_labels, d_targets, d_loss, d_correct, d_prob, (hipStream_t)hip_stream);
    });
}
