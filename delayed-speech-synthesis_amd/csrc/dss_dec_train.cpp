// csrc/dss_dec_train.cpp -- host side of Part 10 of include/dss_hip.h: training the bidirectional decoder (csrc/dec_train.hip).
// Owns the trainer's device memory (master parameters, gradients, square averages, packed copies, the workspace of one trial)
// and the order of the launches; every number is produced by the kernels.
#include <vector>

#include "dss_host.h"

struct dss_dec_trainer {
    int device = 0;
    int C = 0, H = 0, O = 0, Tmax = 0;
    long np = 0;                       // elements of the flat parameter array
    size_t n_wT[2] = {0, 0};           // elements of a packed copy, per layer
    DssDecTrainDev d;
    DssDevBlocks blocks;               // every device allocation of the handle
    bool loaded = false;
};

static int check_sizes(const char *who, int n_inputs, int hidden_units, int n_outputs, int max_frames)
{
    if (n_inputs < 1 || hidden_units < 1 || n_outputs < 1 || max_frames < 1) {
        dss_set_error("%s: %d inputs / %d hidden units / %d outputs / max_frames %d must be positive", who, n_inputs, hidden_units, n_outputs,
                      max_frames);
        return DSS_EINVAL;
    }
    if (hidden_units > DSS_DEC_MAXH || n_inputs > DSS_DEC_MAXC || n_outputs > DSS_DEC_MAXO) {
        dss_set_error("%s: %d hidden units / %d inputs / %d outputs out of range (<= %d / <= %d / <= %d)", who, hidden_units, n_inputs,
                      n_outputs, DSS_DEC_MAXH, DSS_DEC_MAXC, DSS_DEC_MAXO);
        return DSS_EINVAL;
    }
    if (max_frames > DSS_DEC_TRAIN_MAXT) {
        dss_set_error("%s: max_frames %d out of range (<= %d)", who, max_frames, DSS_DEC_TRAIN_MAXT);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" int dss_dec_trainer_check(int n_inputs, int hidden_units, int n_outputs, int max_frames, int T)
{
    int rc = check_sizes("dss_dec_trainer_check", n_inputs, hidden_units, n_outputs, max_frames);
    if (rc) return rc;
    if (T < 1 || T > max_frames) {
        dss_set_error("a trial of %d frames: must be 1 .. max_frames = %d", T, max_frames);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" long dss_dec_trainer_param_count(int n_inputs, int hidden_units, int n_outputs)
{
    if (n_inputs < 1 || hidden_units < 1 || n_outputs < 1) return 0;
    return dss_dec_train_param_count(n_inputs, hidden_units, n_outputs);
}

extern "C" void dss_dec_trainer_destroy(dss_dec_trainer *tr)
{
    if (!tr) return;
    hipSetDevice(tr->device);
    hipDeviceSynchronize();
    tr->blocks.free_all();
    delete tr;
}

extern "C" dss_dec_trainer *dss_dec_trainer_create(int n_inputs, int hidden_units, int n_outputs, int max_frames)
{
    if (check_sizes("dss_dec_trainer_create", n_inputs, hidden_units, n_outputs, max_frames)) return nullptr;
    if (dss_ensure_device()) return nullptr;
    dss_dec_trainer *tr = new dss_dec_trainer;
    hipGetDevice(&tr->device);
    const int C = n_inputs, H = hidden_units, O = n_outputs, H4 = 4 * H, Hp = (H + 3) & ~3;
    const size_t Tm = (size_t)max_frames;
    tr->C = C; tr->H = H; tr->O = O; tr->Tmax = max_frames;
    tr->np = dss_dec_train_param_count(C, H, O);
    tr->n_wT[0] = (size_t)(((C + 3) & ~3) + Hp) * H4;
    tr->n_wT[1] = (size_t)(((2 * H + 3) & ~3) + Hp) * H4;
    DssDecTrainDev &d = tr->d;
    memset(&d, 0, sizeof(d));
    d.C = C; d.H = H; d.O = O; d.Tmax = max_frames;
    int rc = tr->blocks.alloc((size_t)tr->np, &d.p) | tr->blocks.alloc((size_t)tr->np, &d.g) | tr->blocks.alloc((size_t)tr->np, &d.sq);
    for (int L = 0; L < 2; ++L)
        for (int dir = 0; dir < 2; ++dir) {
            rc |= tr->blocks.alloc(tr->n_wT[L], &d.wT[L][dir]) | tr->blocks.alloc((size_t)H4, &d.b[L][dir]);
            rc |= tr->blocks.alloc(Tm * H4, &d.act[L][dir]) | tr->blocks.alloc((Tm + 1) * H, &d.c[L][dir]) | tr->blocks.alloc((Tm + 1) * H, &d.h[L][dir]);
            rc |= tr->blocks.alloc(Tm * H4, &d.dg[L][dir]);
        }
    rc |= tr->blocks.alloc(Tm * C, &d.xs) | tr->blocks.alloc(Tm * 2 * H, &d.midm) | tr->blocks.alloc(Tm * 2 * H, &d.top);
    rc |= tr->blocks.alloc(Tm * O, &d.feat) | tr->blocks.alloc(Tm * O, &d.dfeat) | tr->blocks.alloc(Tm, &d.lossf);
    rc |= tr->blocks.alloc(Tm * 2 * H, &d.dtop) | tr->blocks.alloc(Tm * 2 * H, &d.dmid);
    if (rc) {
        dss_set_error("device allocation failed for the decoder's trainer (%d inputs, %d hidden units, %d outputs, max_frames %d)", C, H, O,
                      max_frames);
        dss_dec_trainer_destroy(tr);
        return nullptr;
    }
    return tr;
}

extern "C" int dss_dec_trainer_load(dss_dec_trainer *tr, const float *const *w)
{
    if (!tr || !w) { dss_set_error("dss_dec_trainer_load: null argument"); return DSS_EINVAL; }
    for (int k = 0; k < 18; ++k) if (!w[k]) { dss_set_error("dss_dec_trainer_load: null array %d", k); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    const int C = tr->C, H = tr->H, O = tr->O, H4 = 4 * H, Hp = (H + 3) & ~3;
    // the flat master copy (state_dict order) and the packed copies of dss_dec_load_weights: [inputs / 4][4H rows][4 consecutive
    // inputs], input counts padded to multiples of 4 with zero weights; b = b_ih + b_hh in float32
    std::vector<float> flat;
    flat.reserve((size_t)tr->np);
    DssDecTrainDev &d = tr->d;
    DSS_HIP_CHECK(hipDeviceSynchronize());                    // no trial may still be running on the arrays about to change
    for (int L = 0; L < 2; ++L) {
        const int Cin = L ? 2 * H : C, Cp = (Cin + 3) & ~3;
        for (int dir = 0; dir < 2; ++dir) {
            const float *w_ih = w[(L * 2 + dir) * 4 + 0], *w_hh = w[(L * 2 + dir) * 4 + 1];
            const float *b_ih = w[(L * 2 + dir) * 4 + 2], *b_hh = w[(L * 2 + dir) * 4 + 3];
            flat.insert(flat.end(), w_ih, w_ih + (size_t)H4 * Cin);
            flat.insert(flat.end(), w_hh, w_hh + (size_t)H4 * H);
            flat.insert(flat.end(), b_ih, b_ih + H4);
            flat.insert(flat.end(), b_hh, b_hh + H4);
            std::vector<float> t(tr->n_wT[L], 0.f), b(H4);
            dss_pack_rows(t.data(), H4, 0, w_ih, Cin);
            dss_pack_rows(t.data(), H4, Cp, w_hh, H);
            for (int r = 0; r < H4; ++r) b[r] = b_ih[r] + b_hh[r];
            DSS_HIP_CHECK(hipMemcpy(d.wT[L][dir], t.data(), t.size() * sizeof(float), hipMemcpyHostToDevice));
            DSS_HIP_CHECK(hipMemcpy(d.b[L][dir], b.data(), b.size() * sizeof(float), hipMemcpyHostToDevice));
        }
    }
    flat.insert(flat.end(), w[16], w[16] + (size_t)O * 2 * H);
    flat.insert(flat.end(), w[17], w[17] + O);
    if ((long)flat.size() != tr->np) { dss_set_error("dss_dec_trainer_load: internal size mismatch"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipMemcpy(d.p, flat.data(), flat.size() * sizeof(float), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemset(d.g, 0, (size_t)tr->np * sizeof(float)));
    DSS_HIP_CHECK(hipMemset(d.sq, 0, (size_t)tr->np * sizeof(float)));
    tr->loaded = true;
    return DSS_OK;
}

extern "C" int dss_dec_trainer_read(dss_dec_trainer *tr, int what, float *out)
{
    if (!tr || !out || what < 0 || what > 2) { dss_set_error("dss_dec_trainer_read: bad arguments (what = 0 parameters, 1 gradients, 2 square averages)"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    DSS_HIP_CHECK(hipDeviceSynchronize());
    const float *src = what == 0 ? tr->d.p : what == 1 ? tr->d.g : tr->d.sq;
    DSS_HIP_CHECK(hipMemcpy(out, src, (size_t)tr->np * sizeof(float), hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_dec_trainer_features(dss_dec_trainer *tr, int T, float *out)
{
    if (!tr || !out || T < 1 || T > tr->Tmax) { dss_set_error("dss_dec_trainer_features: bad arguments (1 <= T <= max_frames)"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    DSS_HIP_CHECK(hipDeviceSynchronize());
    DSS_HIP_CHECK(hipMemcpy(out, tr->d.feat, (size_t)T * tr->O * sizeof(float), hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_dec_trainer_trial_dev(dss_dec_trainer *tr, const void *d_frames, int frames_are_f64, int T, const float *d_targets,
                                         const float *d_mask, int apply_step, double lr, double alpha, double eps, double *d_loss,
                                         void *hip_stream)
{
    if (!tr || !d_frames || !d_targets || !d_loss) { dss_set_error("dss_dec_trainer_trial_dev: null argument"); return DSS_EINVAL; }
    if (!tr->loaded) { dss_set_error("dss_dec_trainer_trial_dev: no parameters loaded (dss_dec_trainer_load)"); return DSS_EINVAL; }
    int rc = dss_dec_trainer_check(tr->C, tr->H, tr->O, tr->Tmax, T);
    if (rc) return rc;
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    return dss_launch_dec_train_trial(tr->d, d_frames, frames_are_f64, T, d_targets, d_mask, apply_step, lr, alpha, eps, d_loss,
                                      (hipStream_t)hip_stream);
}

int dss_dec_trainer_view(dss_dec_trainer *tr, DssDecTrainDev *d, int *device, int *loaded)
{
    if (!tr || !d || !device || !loaded) { dss_set_error("dss_dec_trainer_view: null argument"); return DSS_EINVAL; }
    *d = tr->d;
    *device = tr->device;
    *loaded = tr->loaded ? 1 : 0;
    return DSS_OK;
}

extern "C" int dss_dec_trainer_publish(dss_dec_trainer *tr, dss_dec *v, void *hip_stream)
{
    if (!tr || !tr->loaded) { dss_set_error("dss_dec_trainer_publish: the trainer is NULL or has no parameters loaded"); return DSS_EINVAL; }
    int device = 0, C = 0, H = 0, O = 0;
    float *w[10];
    int rc = dss_dec_device_weights(v, &device, &C, &H, &O, w);
    if (rc) return rc;
    if (C != tr->C || H != tr->H || O != tr->O || device != tr->device) {
        dss_set_error("dss_dec_trainer_publish: the decoder has %d inputs / %d hidden units / %d outputs on device %d, the trainer %d / %d / %d on device %d",
                      C, H, O, device, tr->C, tr->H, tr->O, tr->device);
        return DSS_EINVAL;
    }
    DSS_HIP_CHECK(hipSetDevice(tr->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const DssDecTrainDev &d = tr->d;
    const long np = tr->np;
    for (int L = 0; L < 2; ++L)
        for (int dir = 0; dir < 2; ++dir) {
            DSS_HIP_CHECK(hipMemcpyAsync(w[L * 2 + dir], d.wT[L][dir], tr->n_wT[L] * sizeof(float), hipMemcpyDeviceToDevice, st));
            DSS_HIP_CHECK(hipMemcpyAsync(w[4 + L * 2 + dir], d.b[L][dir], (size_t)4 * H * sizeof(float), hipMemcpyDeviceToDevice, st));
        }
    // regressor.weight and regressor.bias: the last two tensors of the flat array
    DSS_HIP_CHECK(hipMemcpyAsync(w[8], d.p + (np - O - (long)O * 2 * H), (size_t)O * 2 * H * sizeof(float), hipMemcpyDeviceToDevice, st));
    DSS_HIP_CHECK(hipMemcpyAsync(w[9], d.p + (np - O), (size_t)O * sizeof(float), hipMemcpyDeviceToDevice, st));
    return DSS_OK;
}
