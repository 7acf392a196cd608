// csrc/dss_dec_group.cpp -- host side of Part 13 of include/dss_hip.h: several decoders of equal sizes trained side by side, one
// set of seven launches per step (the group kernels of csrc/dec_train.hip).  A group owns M trainers of Part 10 -- so loading,
// reading and publishing a member are Part 10's own functions on that member -- a device table of their M descriptors, written
// once, and a ring of trial tables (DssGroupTables, dss_host.h).  At the end, the decoder half of Part 17: the members over one
// trial list (the group kernels of csrc/bilstm_decoder.hip).
#include <vector>

#include "dss_host.h"

struct dss_dec_group {
    int device = 0;
    int M = 0, C = 0, H = 0, O = 0, Tmax = 0;
    std::vector<dss_dec_trainer *> tr;
    DssGroupTables<DssDecTrainDev, DssDecGroupTrial> tables;
    // trial lists (dss_dec_group_forward_trials_dev): the stream, workgroup and block tables of the last call, pinned staging and
    // device (8-byte words), and the two concatenated layer buffers, (rows, 2H) floats each, grown on demand
    DssDevBlocks blocks;
    DssPinnedStage tstage;
    DssDevArray<long long> d_ttab;
    DssDevArray<float> d_mid, d_top;
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
    g->blocks.free_all();
    g->tstage.destroy();
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

// Part 17: the members' decoders over a trial list, each trial on the member it names.  The list is cut, at trial borders and in
// list order, into sets of launches whose frames fit max_rows rows of the two layer buffers.  Within a set every model's trials
// are sorted longest first (ties in list order) and take consecutive stream slots and consecutive buffer rows, so a model's rows
// are one range: its streams are dealt to layer workgroups of W (the model's remainder gets a partly filled one), its rows to
// regressor blocks of DSS_DEC_RROWS.  The set's workgroups are then sorted by their longest stream, which is their first, across
// the models: the long chains are dispatched first.  All sets' tables travel in one copy.
#define DSS_DEC_GROUP_ROWS (1LL << 19)        // default max_rows: 2 x 400 MB of layer outputs at H = 100

extern "C" int dss_dec_group_forward_trials_dev(dss_dec_group *g, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                                                const long long *first, const int *len, const int *model, long long max_rows, float *d_feats,
                                                void *hip_stream)
{
    const char *who = "dss_dec_group_forward_trials_dev";
    // (an empty list uses neither the frames nor the outputs: empty device arrays may have no address)
    if (!g || (n_trials > 0 && (!d_frames || !d_feats || !model))) { dss_set_error("%s: null argument", who); return DSS_EINVAL; }
    if (max_rows < 0) { dss_set_error("%s: max_rows = %lld: must be 0 (the default) or more", who, max_rows); return DSS_EINVAL; }
    long long total = 0;
    int rc = dss_trials_check(N, n_trials, first, len, &total);
    if (rc) return rc;
    if (!max_rows) max_rows = DSS_DEC_GROUP_ROWS;
    std::vector<char> used((size_t)g->M, 0);
    for (int i = 0; i < n_trials; ++i) {
        if (model[i] < 0 || model[i] >= g->M) { dss_set_error("%s: trial %d names model %d of a group of %d", who, i, model[i], g->M); return DSS_EINVAL; }
        if (first[i] > 0x7fffffffLL) { dss_set_error("%s: trial %d starts behind row 2^31 - 1", who, i); return DSS_EINVAL; }
        if (len[i] > max_rows) { dss_set_error("%s: trial %d has %d frames, max_rows is %lld", who, i, len[i], max_rows); return DSS_EINVAL; }
        used[(size_t)model[i]] = 1;
    }
    for (int m = 0; m < g->M; ++m) {
        if (!used[(size_t)m]) continue;
        DssDecTrainDev d;
        int device = 0, loaded = 0;
        dss_dec_trainer_view(g->tr[(size_t)m], &d, &device, &loaded);
        if (!loaded) { dss_set_error("%s: model %d has no parameters loaded (dss_dec_group_load)", who, m); return DSS_EINVAL; }
    }
    if (!n_trials) return DSS_OK;
    const int W = dss_dec_streams_per_wg(n_trials);
    const std::vector<long long> out_row = trials_offsets(n_trials, [&](int i) { return len[i]; });
    struct Set { size_t w0, w1, b0, b1; };
    std::vector<Set> sets;
    std::vector<DssDecGroupStream> streams;
    std::vector<DssDecGroupWg> wgs;
    std::vector<DssDecGroupBlock> rblocks;
    streams.reserve((size_t)n_trials);
    long long need_rows = 0;
    for (int i0 = 0; i0 < n_trials;) {
        int i1 = i0;
        long long rows = 0;
        while (i1 < n_trials && rows + len[i1] <= max_rows) rows += len[i1++];
        std::vector<int> idx((size_t)(i1 - i0));
        for (int i = i0; i < i1; ++i) idx[(size_t)(i - i0)] = i;
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return model[a] != model[b] ? model[a] < model[b] : len[a] > len[b]; });
        Set set{wgs.size(), 0, rblocks.size(), 0};
        long long buf = 0;
        for (size_t a = 0; a < idx.size();) {
            const int m = model[idx[a]];
            size_t b = a;
            while (b < idx.size() && model[idx[b]] == m) ++b;
            const long long row0 = buf;
            const size_t slot0 = streams.size();
            for (size_t k = a; k < b; ++k) {
                const int i = idx[k];
                streams.push_back(DssDecGroupStream{first[i], out_row[i], buf, len[i], m});
                buf += len[i];
            }
            for (size_t k = a; k < b; k += (size_t)W)
                wgs.push_back(DssDecGroupWg{m, (int)(slot0 + (k - a)), (int)std::min((size_t)W, b - k), 0});
            size_t s = slot0;
            for (long long r = row0; r < buf; r += DSS_DEC_RROWS) {
                while (r >= streams[s].buf_row + streams[s].len) ++s;
                rblocks.push_back(DssDecGroupBlock{r, m, (int)s, (int)std::min((long long)DSS_DEC_RROWS, buf - r), 0});
            }
            a = b;
        }
        std::stable_sort(wgs.begin() + (long)set.w0, wgs.end(),
                         [&](const DssDecGroupWg &a, const DssDecGroupWg &b) { return streams[(size_t)a.slot0].len > streams[(size_t)b.slot0].len; });
        set.w1 = wgs.size(); set.b1 = rblocks.size();
        sets.push_back(set);
        need_rows = std::max(need_rows, rows);
        i0 = i1;
    }
    DSS_HIP_CHECK(hipSetDevice(g->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t sb = streams.size() * sizeof(DssDecGroupStream), wb = wgs.size() * sizeof(DssDecGroupWg), bb = rblocks.size() * sizeof(DssDecGroupBlock);
    char *stage = (char *)g->tstage.acquire(sb + wb + bb);
    if (!stage) { dss_set_error("pinned staging for the trial tables failed"); return DSS_ENOMEM; }
    memcpy(stage, streams.data(), sb);
    memcpy(stage + sb, wgs.data(), wb);
    memcpy(stage + sb + wb, rblocks.data(), bb);
    const size_t lay = (size_t)need_rows * 2 * (size_t)g->H;
    if ((rc = g->d_ttab.grow(g->blocks, (sb + wb + bb) / sizeof(long long))) || (rc = g->d_mid.grow(g->blocks, lay)) || (rc = g->d_top.grow(g->blocks, lay))) {
        dss_set_error("%s: device allocation failed for the tables or for two layer buffers of %lld rows", who, need_rows);
        return rc;
    }
    char *d_tab = (char *)(long long *)g->d_ttab;
    DSS_HIP_CHECK(hipMemcpyAsync(d_tab, stage, sb + wb + bb, hipMemcpyHostToDevice, st));
    if ((rc = g->tstage.commit(st))) return rc;
    const DssDecGroupStream *d_streams = (const DssDecGroupStream *)d_tab;
    const DssDecGroupWg *d_wgs = (const DssDecGroupWg *)(d_tab + sb);
    const DssDecGroupBlock *d_blocks = (const DssDecGroupBlock *)(d_tab + sb + wb);
    for (const Set &s : sets) {
        rc = dss_launch_decoder_trials_group(g->tables.d_models, g->C, g->H, g->O, d_frames, frames_are_f64, W, d_streams, d_wgs + s.w0,
                                             (int)(s.w1 - s.w0), d_blocks + s.b0, (int)(s.b1 - s.b0), g->d_mid, g->d_top, d_feats, st);
        if (rc) return rc;
    }
    return DSS_OK;
}
