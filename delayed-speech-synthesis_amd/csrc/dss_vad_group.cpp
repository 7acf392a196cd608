// csrc/dss_vad_group.cpp -- host side of Part 15 of include/dss_hip.h: several detectors of equal sizes trained side by side, one
// pair of launches per window (the group kernels of csrc/vad_train.hip).  A group owns M trainers of Part 9 -- so loading,
// reading, state access and publishing a member are Part 9's own functions on that member -- a device table of their M
// descriptors, written once, and a ring of trial tables (DssGroupTables, dss_host.h).  At the end, the detector half of Part 17:
// the members over one trial list (the group kernel of csrc/vad_lstm.hip).
#include <vector>

#include "dss_host.h"

struct dss_vad_group {
    int device = 0;
    int M = 0, C = 0, H = 0, Tmax = 0;
    std::vector<dss_vad_trainer *> tr;
    DssGroupTables<DssVadTrainDev, DssVadGroupTrial> tables;
    // trial lists (dss_vad_group_forward_trials_dev): the descriptor table of the last call, pinned staging and device
    DssDevBlocks blocks;
    DssPinnedStage tstage;
    DssDevArray<DssVadTrialDesc> d_tdesc;
};

extern "C" int dss_vad_group_check(int n_models, int n_inputs, int hidden_units, int max_window)
{
    int rc = dss_vad_trainer_check(n_inputs, hidden_units, max_window, 1, 1, 1);
    if (rc) return rc;
    if (n_models < 1 || n_models > DSS_VAD_GROUP_MAXM) {
        dss_set_error("a group of %d models: must be 1 .. %d (more models: more groups)", n_models, DSS_VAD_GROUP_MAXM);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" void dss_vad_group_destroy(dss_vad_group *g)
{
    if (!g) return;
    hipSetDevice(g->device);
    hipDeviceSynchronize();
    g->tables.destroy();
    g->blocks.free_all();
    g->tstage.destroy();
    for (dss_vad_trainer *t : g->tr) dss_vad_trainer_destroy(t);
    delete g;
}

extern "C" dss_vad_group *dss_vad_group_create(int n_models, int n_inputs, int hidden_units, int max_window)
{
    if (dss_vad_group_check(n_models, n_inputs, hidden_units, max_window)) return nullptr;
    if (dss_ensure_device()) return nullptr;
    dss_vad_group *g = new dss_vad_group;
    hipGetDevice(&g->device);
    g->M = n_models; g->C = n_inputs; g->H = hidden_units; g->Tmax = max_window;
    std::vector<DssVadTrainDev> table((size_t)n_models);
    for (int m = 0; m < n_models; ++m) {
        dss_vad_trainer *t = dss_vad_trainer_create(n_inputs, hidden_units, max_window);
        if (!t) { dss_vad_group_destroy(g); return nullptr; }
        g->tr.push_back(t);
        int device = 0, loaded = 0;
        dss_vad_trainer_view(t, &table[m], &device, &loaded);
    }
    if (g->tables.init(table)) {
        dss_set_error("device allocation failed for the tables of a group of %d detector trainers", n_models);
        dss_vad_group_destroy(g);
        return nullptr;
    }
    return g;
}

static dss_vad_trainer *member(dss_vad_group *g, int m, const char *who)
{
    if (!g || m < 0 || m >= g->M) {
        dss_set_error("%s: model %d of a group of %d (or a NULL group)", who, m, g ? g->M : 0);
        return nullptr;
    }
    return g->tr[(size_t)m];
}

extern "C" int dss_vad_group_load(dss_vad_group *g, int m, const float *w_ih0, const float *w_hh0, const float *b_ih0, const float *b_hh0,
                                  const float *w_ih1, const float *w_hh1, const float *b_ih1, const float *b_hh1, const float *cls_w,
                                  const float *cls_b)
{
    dss_vad_trainer *t = member(g, m, "dss_vad_group_load");
    return t ? dss_vad_trainer_load(t, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, cls_w, cls_b) : DSS_EINVAL;
}

extern "C" int dss_vad_group_read(dss_vad_group *g, int m, int what, float *out)
{
    dss_vad_trainer *t = member(g, m, "dss_vad_group_read");
    return t ? dss_vad_trainer_read(t, what, out) : DSS_EINVAL;
}

extern "C" int dss_vad_group_state(dss_vad_group *g, int m, float *h, float *c, int set)
{
    dss_vad_trainer *t = member(g, m, "dss_vad_group_state");
    return t ? dss_vad_trainer_state(t, h, c, set) : DSS_EINVAL;
}

extern "C" int dss_vad_group_publish(dss_vad_group *g, int m, dss_vad *v, void *hip_stream)
{
    dss_vad_trainer *t = member(g, m, "dss_vad_group_publish");
    return t ? dss_vad_trainer_publish(t, v, hip_stream) : DSS_EINVAL;
}

// One step: the checks, the table through the ring, the launches.  window == 0: dss_vad_group_window_dev (one window of len
// frames each, no reset, apply_step honoured); else dss_vad_group_trial_dev.  Returns the number of window pairs launched.
static int group_step(dss_vad_group *g, const dss_vad_group_trial *trials, int window, int frames_are_f64, void *hip_stream, const char *who)
{
    if (!g || !trials) { dss_set_error("%s: null argument", who); return DSS_EINVAL; }
    const bool whole_trials = window != 0;
    if (whole_trials && (window < 1 || window > g->Tmax)) {
        dss_set_error("%s: windows of %d frames: must be 1 .. max_window = %d", who, window, g->Tmax);
        return DSS_EINVAL;
    }
    const int win = whole_trials ? window : g->Tmax;
    int n_windows = 0;
    for (int m = 0; m < g->M; ++m) {
        const dss_vad_group_trial &t = trials[m];
        if (t.len == 0) continue;
        if (t.len < 0) { dss_set_error("%s: model %d: %d frames: must be 0 (sits out) or more", who, m, t.len); return DSS_EINVAL; }
        if (!whole_trials && t.len > g->Tmax) {
            dss_set_error("%s: model %d: a window of %d frames: must be 0 (sits out) .. max_window = %d", who, m, t.len, g->Tmax);
            return DSS_EINVAL;
        }
        if (!t.d_frames || !t.d_targets || !t.d_losses) {
            dss_set_error("%s: model %d: null frames, targets or losses for %d frames", who, m, t.len);
            return DSS_EINVAL;
        }
        DssVadTrainDev d;
        int device = 0, loaded = 0;
        dss_vad_trainer_view(g->tr[(size_t)m], &d, &device, &loaded);
        if (!loaded) { dss_set_error("%s: model %d has no parameters loaded (dss_vad_group_load)", who, m); return DSS_EINVAL; }
        const int nw = (int)(((long long)t.len + win - 1) / win);
        if (nw > n_windows) n_windows = nw;
    }
    if (!n_windows) { dss_set_error("%s: every model sits out (all len are 0): nothing to launch", who); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)hip_stream;
    DssVadGroupTrial *slot = g->tables.acquire();
    if (!slot) { dss_set_error("%s: waiting for a free trial table failed", who); return DSS_ENODEV; }
    for (int m = 0; m < g->M; ++m) {
        const dss_vad_group_trial &t = trials[m];
        DssVadGroupTrial &e = slot[m];
        e.frames = t.d_frames; e.targets = t.d_targets; e.mask = t.d_mask; e.losses = t.d_losses;
        e.lr = t.lr; e.alpha = t.alpha; e.eps = t.eps;
        e.len = t.len; e.apply = whole_trials ? 1 : t.apply_step;
    }
    const DssVadGroupTrial *d_slot = nullptr;
    int rc = g->tables.upload(st, &d_slot);
    if (rc) return rc;
    rc = dss_launch_vad_train_group(g->tables.d_models, d_slot, g->M, g->C, g->H, n_windows, win, whole_trials ? 1 : 0, frames_are_f64, st);
    // behind the last launch, not only the copy: the device table of the slot is read until the step's last window has run
    int rc2 = g->tables.commit_after_launch(st);
    return rc ? rc : rc2 ? rc2 : n_windows;
}

extern "C" int dss_vad_group_window_dev(dss_vad_group *g, const dss_vad_group_trial *trials, int frames_are_f64, void *hip_stream)
{
    int rc = group_step(g, trials, 0, frames_are_f64, hip_stream, "dss_vad_group_window_dev");
    return rc < 0 ? rc : DSS_OK;
}

extern "C" int dss_vad_group_trial_dev(dss_vad_group *g, const dss_vad_group_trial *trials, int window, int frames_are_f64, void *hip_stream)
{
    if (g && window == 0) {
        dss_set_error("dss_vad_group_trial_dev: windows of 0 frames: must be 1 .. max_window = %d", g->Tmax);
        return DSS_EINVAL;
    }
    return group_step(g, trials, window, frames_are_f64, hip_stream, "dss_vad_group_trial_dev");
}

// Part 17: the members' detectors over a trial list, each trial on the member it names, in one launch.  The checks come first and
// need no device beyond the one the group was created on; the table is Part 8's, sorted longest first across all models, with
// the member in the entry.
extern "C" int dss_vad_group_forward_trials_dev(dss_vad_group *g, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                                                const long long *first, const int *len, const int *model, int *d_labels, float *d_logits,
                                                void *hip_stream)
{
    // (an empty list uses neither the frames nor the outputs: empty device arrays may have no address)
    if (!g || (n_trials > 0 && (!d_frames || !d_labels || !model))) { dss_set_error("dss_vad_group_forward_trials_dev: null argument"); return DSS_EINVAL; }
    long long total = 0;
    int rc = dss_trials_check(N, n_trials, first, len, &total);
    if (rc) return rc;
    std::vector<char> used((size_t)g->M, 0);
    for (int i = 0; i < n_trials; ++i) {
        if (model[i] < 0 || model[i] >= g->M) {
            dss_set_error("dss_vad_group_forward_trials_dev: trial %d names model %d of a group of %d", i, model[i], g->M);
            return DSS_EINVAL;
        }
        used[(size_t)model[i]] = 1;
    }
    for (int m = 0; m < g->M; ++m) {
        if (!used[(size_t)m]) continue;
        DssVadTrainDev d;
        int device = 0, loaded = 0;
        dss_vad_trainer_view(g->tr[(size_t)m], &d, &device, &loaded);
        if (!loaded) { dss_set_error("dss_vad_group_forward_trials_dev: model %d has no parameters loaded (dss_vad_group_load)", m); return DSS_EINVAL; }
    }
    if (!n_trials) return DSS_OK;
    DSS_HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const std::vector<long long> out_row = trials_offsets(n_trials, [&](int i) { return len[i]; });
    const std::vector<int> order = trials_longest_first(n_trials, len);
    DssVadTrialDesc *desc = (DssVadTrialDesc *)g->tstage.acquire(sizeof(DssVadTrialDesc) * (size_t)n_trials);
    if (!desc) { dss_set_error("pinned staging for the trial table failed"); return DSS_ENOMEM; }
    for (int k = 0; k < n_trials; ++k) { const int i = order[k]; desc[k] = DssVadTrialDesc{first[i], out_row[i], len[i], model[i]}; }
    rc = g->d_tdesc.grow(g->blocks, (size_t)n_trials);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpyAsync(g->d_tdesc, desc, sizeof(DssVadTrialDesc) * (size_t)n_trials, hipMemcpyHostToDevice, st));
    if ((rc = g->tstage.commit(st))) return rc;
    return dss_launch_vad_trials_group(g->tables.d_models, g->C, g->H, d_frames, frames_are_f64, g->d_tdesc, n_trials, d_labels, d_logits, st);
}
