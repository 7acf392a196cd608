// csrc/dss_dec_group.cpp -- host side of Part 13 of include/dss_hip.h: several decoders of equal sizes trained side by side, one
// set of seven launches per step (the group kernels of csrc/dec_train.hip).  A group owns M trainers of Part 10 -- so loading,
// reading and publishing a member are Part 10's own functions on that member -- a device table of their M descriptors, written
// once, and a ring of trial tables (DssGroupTables, dss_host.h).
#include <vector>

#include "dss_host.h"

struct dss_dec_group {
    int device = 0;
    int M = 0, C = 0, H = 0, O = 0, Tmax = 0;
    std::vector<dss_dec_trainer *> tr;
    DssGroupTables<DssDecTrainDev, DssDecGroupTrial> tables;
};

extern "C" int dss_dec_group_check(int n_models, int n_inputs, int hidden_units, int n_outputs, int max_frames)
{
    int rc = dss_dec_trainer_check(n_inputs, hidden_units, n_outputs, max_frames, 1);
    if (rc) return rc;
    if (n_models < 1 || n_models > DSS_DEC_GROUP_MAXM) {
        dss_set_error("a group of %d models: must be 1 .. %d (more models: more groups)", n_models, DSS_DEC_GROUP_MAXM);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" void dss_dec_group_destroy(dss_dec_group *g)
{
    if (!g) return;
    hipSetDevice(g->device);
    hipDeviceSynchronize();
    g->tables.destroy();
    for (dss_dec_trainer *t : g->tr) dss_dec_trainer_destroy(t);
    delete g;
}

extern "C" dss_dec_group *dss_dec_group_create(int n_models, int n_inputs, int hidden_units, int n_outputs, int max_frames)
{
    if (dss_dec_group_check(n_models, n_inputs, hidden_units, n_outputs, max_frames)) return nullptr;
    if (dss_ensure_device()) return nullptr;
    dss_dec_group *g = new dss_dec_group;
    hipGetDevice(&g->device);
    g->M = n_models; g->C = n_inputs; g->H = hidden_units; g->O = n_outputs; g->Tmax = max_frames;
    std::vector<DssDecTrainDev> table((size_t)n_models);
    for (int m = 0; m < n_models; ++m) {
        dss_dec_trainer *t = dss_dec_trainer_create(n_inputs, hidden_units, n_outputs, max_frames);
        if (!t) { dss_dec_group_destroy(g); return nullptr; }
        g->tr.push_back(t);
        int device = 0, loaded = 0;
        dss_dec_trainer_view(t, &table[m], &device, &loaded);
    }
    if (g->tables.init(table)) {
        dss_set_error("device allocation failed for the tables of a group of %d decoder trainers", n_models);
        dss_dec_group_destroy(g);
        return nullptr;
    }
    return g;
}

static dss_dec_trainer *member(dss_dec_group *g, int m, const char *who)
{
    if (!g || m < 0 || m >= g->M) {
        dss_set_error("%s: model %d of a group of %d (or a NULL group)", who, m, g ? g->M : 0);
        return nullptr;
    }
    return g->tr[(size_t)m];
}

extern "C" int dss_dec_group_load(dss_dec_group *g, int m, const float *const *w)
{
    dss_dec_trainer *t = member(g, m, "dss_dec_group_load");
    return t ? dss_dec_trainer_load(t, w) : DSS_EINVAL;
}

extern "C" int dss_dec_group_read(dss_dec_group *g, int m, int what, float *out)
{
    dss_dec_trainer *t = member(g, m, "dss_dec_group_read");
    return t ? dss_dec_trainer_read(t, what, out) : DSS_EINVAL;
}

extern "C" int dss_dec_group_features(dss_dec_group *g, int m, int T, float *out)
{
    dss_dec_trainer *t = member(g, m, "dss_dec_group_features");
    return t ? dss_dec_trainer_features(t, T, out) : DSS_EINVAL;
}

extern "C" int dss_dec_group_publish(dss_dec_group *g, int m, dss_dec *dec, void *hip_stream)
{
    dss_dec_trainer *t = member(g, m, "dss_dec_group_publish");
    return t ? dss_dec_trainer_publish(t, dec, hip_stream) : DSS_EINVAL;
}

extern "C" int dss_dec_group_step_dev(dss_dec_group *g, const dss_dec_group_trial *trials, int frames_are_f64, double *d_losses,
                                      void *hip_stream)
{
    if (!g || !trials || !d_losses) { dss_set_error("dss_dec_group_step_dev: null argument"); return DSS_EINVAL; }
    int max_T = 0;
    for (int m = 0; m < g->M; ++m) {
        const dss_dec_group_trial &t = trials[m];
        if (t.T == 0) continue;
        if (t.T < 0 || t.T > g->Tmax) {
            dss_set_error("dss_dec_group_step_dev: model %d: a trial of %d frames: must be 0 (sits out) .. max_frames = %d", m, t.T, g->Tmax);
            return DSS_EINVAL;
        }
        if (!t.d_frames || !t.d_targets) {
            dss_set_error("dss_dec_group_step_dev: model %d: null frames or targets for a trial of %d frames", m, t.T);
            return DSS_EINVAL;
        }
        DssDecTrainDev d;
        int device = 0, loaded = 0;
        dss_dec_trainer_view(g->tr[(size_t)m], &d, &device, &loaded);
        if (!loaded) {
            dss_set_error("dss_dec_group_step_dev: model %d has no parameters loaded (dss_dec_group_load)", m);
            return DSS_EINVAL;
        }
        if (t.T > max_T) max_T = t.T;
    }
    if (!max_T) { dss_set_error("dss_dec_group_step_dev: every model sits out (all T are 0): nothing to launch"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)hip_stream;
    DssDecGroupTrial *slot = g->tables.acquire();
    if (!slot) { dss_set_error("dss_dec_group_step_dev: waiting for a free trial table failed"); return DSS_ENODEV; }
    for (int m = 0; m < g->M; ++m) {
        const dss_dec_group_trial &t = trials[m];
        DssDecGroupTrial &e = slot[m];
        e.frames = t.d_frames; e.targets = t.d_targets; e.mask = t.d_mask; e.loss = d_losses + m;
        e.lr = t.lr; e.alpha = t.alpha; e.eps = t.eps;
        e.T = t.T; e.apply = t.apply_step;
    }
    const DssDecGroupTrial *d_slot = nullptr;
    int rc = g->tables.upload(st, &d_slot);
    if (rc) return rc;
    rc = dss_launch_dec_train_group(g->tables.d_models, d_slot, g->M, g->C, g->H, g->O, max_T, frames_are_f64, st);
    // behind the launches, not only the copy: the device table of the slot is read until the step's last launch has run
    int rc2 = g->tables.commit_after_launch(st);
    return rc ? rc : rc2;
}
