// csrc/dss_vad_train.cpp -- host side of Part 9 of include/dss_hip.h: training the neural voice-activity detector
// (csrc/vad_train.hip).  Owns the trainer's device memory (master parameters, gradients, square averages, packed copies, the
// carried state, the workspace of one window) and the order of the launches; every number is produced by the kernels.
#include <vector>

#include "dss_host.h"

struct dss_vad_trainer {
    int device = 0;
    int C = 0, H = 0, Tmax = 0;
    long np = 0;                       // elements of the flat parameter array
    size_t n_wT0 = 0, n_wT1 = 0;       // elements of the packed copies
    DssVadTrainDev d;
    DssDevBlocks blocks;               // every device allocation of the handle
    bool loaded = false;
};

static int check_sizes(const char *who, int n_inputs, int hidden_units, int max_window)
{
    if (n_inputs < 1 || hidden_units < 1 || max_window < 1) {
        dss_set_error("%s: %d inputs / %d hidden units / max_window %d must be positive", who, n_inputs, hidden_units, max_window);
        return DSS_EINVAL;
    }
    if (hidden_units > DSS_VAD_MAXH || n_inputs > DSS_VAD_MAXC) {
        dss_set_error("%s: %d hidden units / %d inputs out of range (<= %d / <= %d)", who, hidden_units, n_inputs, DSS_VAD_MAXH, DSS_VAD_MAXC);
        return DSS_EINVAL;
    }
    if (max_window > DSS_VAD_TRAIN_MAXT) {
        dss_set_error("%s: max_window %d out of range (<= %d)", who, max_window, DSS_VAD_TRAIN_MAXT);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" int dss_vad_trainer_check(int n_inputs, int hidden_units, int max_window, int T, int len, int window)
{
    int rc = check_sizes("dss_vad_trainer_check", n_inputs, hidden_units, max_window);
    if (rc) return rc;
    if (T < 1 || T > max_window) {
        dss_set_error("a window of %d frames: must be 1 .. max_window = %d", T, max_window);
        return DSS_EINVAL;
    }
    if (len < 1) { dss_set_error("a trial of %d frames: must be at least 1", len); return DSS_EINVAL; }
    if (window < 1 || window > max_window) {
        dss_set_error("windows of %d frames: must be 1 .. max_window = %d", window, max_window);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" void dss_vad_trainer_destroy(dss_vad_trainer *tr)
{
    if (!tr) return;
    hipSetDevice(tr->device);
    hipDeviceSynchronize();
    tr->blocks.free_all();
    delete tr;
}

extern "C" dss_vad_trainer *dss_vad_trainer_create(int n_inputs, int hidden_units, int max_window)
{
    if (check_sizes("dss_vad_trainer_create", n_inputs, hidden_units, max_window)) return nullptr;
    if (dss_ensure_device()) return nullptr;
    dss_vad_trainer *tr = new dss_vad_trainer;
    hipGetDevice(&tr->device);
    const int C = n_inputs, H = hidden_units, H4 = 4 * H, Cp = (C + 3) & ~3, Hp = (H + 3) & ~3;
    const size_t Tm = (size_t)max_window;
    tr->C = C; tr->H = H; tr->Tmax = max_window;
    tr->np = dss_vad_train_param_count(C, H);
    tr->n_wT0 = (size_t)(Cp + Hp) * H4;
    tr->n_wT1 = (size_t)2 * Hp * H4;
    DssVadTrainDev &d = tr->d;
    memset(&d, 0, sizeof(d));
    d.v.S = 1; d.v.C = C; d.v.H = H; d.Tmax = max_window;
    int rc = tr->blocks.alloc((size_t)tr->np, &d.p) | tr->blocks.alloc((size_t)tr->np, &d.g) | tr->blocks.alloc((size_t)tr->np, &d.sq);
    rc |= tr->blocks.alloc(tr->n_wT0, &d.wT0) | tr->blocks.alloc((size_t)H4, &d.b0) | tr->blocks.alloc(tr->n_wT1, &d.wT1) | tr->blocks.alloc((size_t)H4, &d.b1);
    rc |= tr->blocks.alloc((size_t)2 * H, &d.v.h) | tr->blocks.alloc((size_t)2 * H, &d.v.c);
    rc |= tr->blocks.alloc(Tm * C, &d.xs) | tr->blocks.alloc(Tm * H4, &d.act0) | tr->blocks.alloc(Tm * H4, &d.act1);
    rc |= tr->blocks.alloc((Tm + 1) * H, &d.c0) | tr->blocks.alloc((Tm + 1) * H, &d.c1) | tr->blocks.alloc((Tm + 1) * H, &d.h0) | tr->blocks.alloc((Tm + 1) * H, &d.h1);
    rc |= tr->blocks.alloc(Tm * H, &d.h0m) | tr->blocks.alloc(Tm * 2, &d.logit) | tr->blocks.alloc(Tm * 2, &d.dl) | tr->blocks.alloc(Tm, &d.lossf);
    rc |= tr->blocks.alloc(Tm * H4, &d.dg0) | tr->blocks.alloc(Tm * H4, &d.dg1) | tr->blocks.alloc(Tm * H, &d.dh0m);
    if (rc) {
        dss_set_error("device allocation failed for the detector's trainer (%d inputs, %d hidden units, max_window %d)", C, H, max_window);
        dss_vad_trainer_destroy(tr);
        return nullptr;
    }
    d.v.wT0 = d.wT0; d.v.b0 = d.b0; d.v.wT1 = d.wT1; d.v.b1 = d.b1;
    d.v.wc = d.p + (tr->np - 2 - 2 * H);           // classifier.weight and classifier.bias: the last two tensors of the flat array
    d.v.bc = d.p + (tr->np - 2);
    return tr;
}

extern "C" int dss_vad_trainer_load(dss_vad_trainer *tr, const float *w_ih0, const float *w_hh0, const float *b_ih0, const float *b_hh0,
                                    const float *w_ih1, const float *w_hh1, const float *b_ih1, const float *b_hh1,
                                    const float *cls_w, const float *cls_b)
{
    if (!tr || !w_ih0 || !w_hh0 || !b_ih0 || !b_hh0 || !w_ih1 || !w_hh1 || !b_ih1 || !b_hh1 || !cls_w || !cls_b) {
        dss_set_error("dss_vad_trainer_load: null argument"); return DSS_EINVAL;
    }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    const int C = tr->C, H = tr->H, H4 = 4 * H, Cp = (C + 3) & ~3, Hp = (H + 3) & ~3;
    // the flat master copy (state_dict order) and the packed copies of dss_vad_load_weights: [inputs / 4][4H rows][4 consecutive
    // inputs], input counts padded to multiples of 4 with zero weights; b = b_ih + b_hh in float32
    std::vector<float> flat;
    flat.reserve((size_t)tr->np);
    const float *src[10] = {w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, cls_w, cls_b};
    const size_t cnt[10] = {(size_t)H4 * C, (size_t)H4 * H, (size_t)H4, (size_t)H4, (size_t)H4 * H, (size_t)H4 * H, (size_t)H4, (size_t)H4,
                            (size_t)2 * H, 2};
    for (int k = 0; k < 10; ++k) flat.insert(flat.end(), src[k], src[k] + cnt[k]);
    std::vector<float> t0(tr->n_wT0, 0.f), t1(tr->n_wT1, 0.f), b0(H4), b1(H4);
    dss_pack_rows(t0.data(), H4, 0, w_ih0, C);
    dss_pack_rows(t0.data(), H4, Cp, w_hh0, H);
    dss_pack_rows(t1.data(), H4, 0, w_ih1, H);
    dss_pack_rows(t1.data(), H4, Hp, w_hh1, H);
    for (int r = 0; r < H4; ++r) {
        b0[r] = b_ih0[r] + b_hh0[r];
        b1[r] = b_ih1[r] + b_hh1[r];
    }
    DssVadTrainDev &d = tr->d;
    DSS_HIP_CHECK(hipDeviceSynchronize());                    // no window may still be running on the arrays about to change
    DSS_HIP_CHECK(hipMemcpy(d.p, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemcpy(d.wT0, t0.data(), t0.size() * sizeof(float), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemcpy(d.wT1, t1.data(), t1.size() * sizeof(float), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemcpy(d.b0, b0.data(), b0.size() * sizeof(float), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemcpy(d.b1, b1.data(), b1.size() * sizeof(float), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemset(d.g, 0, (size_t)tr->np * sizeof(float)));
    DSS_HIP_CHECK(hipMemset(d.sq, 0, (size_t)tr->np * sizeof(float)));
    DSS_HIP_CHECK(hipMemset(d.v.h, 0, (size_t)2 * H * sizeof(float)));
    DSS_HIP_CHECK(hipMemset(d.v.c, 0, (size_t)2 * H * sizeof(float)));
    tr->loaded = true;
    return DSS_OK;
}

extern "C" long dss_vad_trainer_param_count(int n_inputs, int hidden_units)
{
    if (n_inputs < 1 || hidden_units < 1) return 0;
    return dss_vad_train_param_count(n_inputs, hidden_units);
}

extern "C" int dss_vad_trainer_read(dss_vad_trainer *tr, int what, float *out)
{
    if (!tr || !out || what < 0 || what > 2) { dss_set_error("dss_vad_trainer_read: bad arguments (what = 0 parameters, 1 gradients, 2 square averages)"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    DSS_HIP_CHECK(hipDeviceSynchronize());
    const float *src = what == 0 ? tr->d.p : what == 1 ? tr->d.g : tr->d.sq;
    DSS_HIP_CHECK(hipMemcpy(out, src, (size_t)tr->np * sizeof(float), hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_vad_trainer_state(dss_vad_trainer *tr, float *h, float *c, int set)
{
    if (!tr) { dss_set_error("dss_vad_trainer_state: null trainer"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    const size_t n = (size_t)2 * tr->H * sizeof(float);
    DSS_HIP_CHECK(hipDeviceSynchronize());
    if (h) DSS_HIP_CHECK(set ? hipMemcpy(tr->d.v.h, h, n, hipMemcpyHostToDevice) : hipMemcpy(h, tr->d.v.h, n, hipMemcpyDeviceToHost));
    if (c) DSS_HIP_CHECK(set ? hipMemcpy(tr->d.v.c, c, n, hipMemcpyHostToDevice) : hipMemcpy(c, tr->d.v.c, n, hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_vad_trainer_reset_state(dss_vad_trainer *tr, void *hip_stream)
{
    if (!tr) { dss_set_error("dss_vad_trainer_reset_state: null trainer"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    const size_t n = (size_t)2 * tr->H * sizeof(float);
    DSS_HIP_CHECK(hipMemsetAsync(tr->d.v.h, 0, n, (hipStream_t)hip_stream));
    DSS_HIP_CHECK(hipMemsetAsync(tr->d.v.c, 0, n, (hipStream_t)hip_stream));
    return DSS_OK;
}

extern "C" int dss_vad_trainer_window_dev(dss_vad_trainer *tr, const void *d_frames, int frames_are_f64, int T, const unsigned char *d_targets,
                                          const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss,
                                          void *hip_stream)
{
    if (!tr || !d_frames || !d_targets || !d_loss) { dss_set_error("dss_vad_trainer_window_dev: null argument"); return DSS_EINVAL; }
    if (!tr->loaded) { dss_set_error("dss_vad_trainer_window_dev: no parameters loaded (dss_vad_trainer_load)"); return DSS_EINVAL; }
    int rc = dss_vad_trainer_check(tr->C, tr->H, tr->Tmax, T, 1, 1);
    if (rc) return rc;
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    return dss_launch_vad_train_window(tr->d, d_frames, frames_are_f64, T, d_targets, d_mask, apply_step, lr, alpha, eps, d_loss,
                                       (hipStream_t)hip_stream);
}

extern "C" int dss_vad_trainer_trial_dev(dss_vad_trainer *tr, const void *d_frames, int frames_are_f64, int len, const unsigned char *d_targets,
                                         const float *d_masks, int window, double lr, double alpha, double eps, double *d_losses,
                                         void *hip_stream)
{
    if (!tr || !d_frames || !d_targets || !d_losses) { dss_set_error("dss_vad_trainer_trial_dev: null argument"); return DSS_EINVAL; }
    if (!tr->loaded) { dss_set_error("dss_vad_trainer_trial_dev: no parameters loaded (dss_vad_trainer_load)"); return DSS_EINVAL; }
    int rc = dss_vad_trainer_check(tr->C, tr->H, tr->Tmax, 1, len, window);
    if (rc) return rc;
    rc = dss_vad_trainer_reset_state(tr, hip_stream);
    if (rc) return rc;
    const size_t fsz = frames_are_f64 ? sizeof(double) : sizeof(float);
    int w = 0;
    for (int t0 = 0; t0 < len; t0 += window, ++w) {          // x.split(window): the last window is the remainder
        const int T = len - t0 < window ? len - t0 : window;
        rc = dss_launch_vad_train_window(tr->d, (const char *)d_frames + (size_t)t0 * tr->C * fsz, frames_are_f64, T, d_targets + t0,
                                         d_masks ? d_masks + (size_t)t0 * tr->H : nullptr, 1, lr, alpha, eps, d_losses + w,
                                         (hipStream_t)hip_stream);
        if (rc) return rc;
    }
    return w;
}

int dss_vad_trainer_view(dss_vad_trainer *tr, DssVadTrainDev *d, int *device, int *loaded)
{
    if (!tr || !d || !device || !loaded) { dss_set_error("dss_vad_trainer_view: null argument"); return DSS_EINVAL; }
    *d = tr->d;
    *device = tr->device;
    *loaded = tr->loaded ? 1 : 0;
    return DSS_OK;
}

extern "C" int dss_vad_trainer_publish(dss_vad_trainer *tr, dss_vad *v, void *hip_stream)
{
    if (!tr || !tr->loaded) { dss_set_error("dss_vad_trainer_publish: the trainer is NULL or has no parameters loaded"); return DSS_EINVAL; }
    int device = 0, C = 0, H = 0;
    float *w[6];
    int rc = dss_vad_device_weights(v, &device, &C, &H, w);
    if (rc) return rc;
    if (C != tr->C || H != tr->H || device != tr->device) {
        dss_set_error("dss_vad_trainer_publish: the detector has %d inputs / %d hidden units on device %d, the trainer %d / %d on device %d",
                      C, H, device, tr->C, tr->H, tr->device);
        return DSS_EINVAL;
    }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const DssVadTrainDev &d = tr->d;
    const float *src[6] = {d.wT0, d.b0, d.wT1, d.b1, d.v.wc, d.v.bc};
    const size_t cnt[6] = {tr->n_wT0, (size_t)4 * H, tr->n_wT1, (size_t)4 * H, (size_t)2 * H, 2};
    for (int k = 0; k < 6; ++k) DSS_HIP_CHECK(hipMemcpyAsync(w[k], src[k], cnt[k] * sizeof(float), hipMemcpyDeviceToDevice, st));
    return DSS_OK;
}
