// csrc/dss_dec.cpp -- host side of the bidirectional recurrent decoder (Part 6 of include/dss_hip.h; csrc/bilstm_decoder.hip)
// and of its trial-list forms (Part 8).
#include <string.h>

#include <algorithm>
#include <vector>

#include "dss_host.h"

// ------------------------------------------------------------------------------------------------------
// bidirectional recurrent decoder (Part 6 of include/dss_hip.h; csrc/bilstm_decoder.hip)
// ------------------------------------------------------------------------------------------------------
struct dss_dec {
    int device;
    DssDecDev d;
    DssDevBlocks blocks;
    float *w[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // wT[2][2], b[2][2], wr, br
    bool loaded = false;
    int *d_meta = nullptr;        // [2][S_max]: frame counts, input rows of a ragged call (dss_dec_forward_rows_dev)
    DssPinnedRing meta;           //   their pinned staging
    // trial lists (dss_dec_forward_trials_dev): per trial, longest first: output row | frame count, first row; pinned staging
    // and device
    DssPinnedStage tstage;
    DssDevArray<int> d_tmeta;
    DssDevArray<long long> d_tout;
};

int dss_dec_device_weights(dss_dec *v, int *device, int *n_inputs, int *hidden_units, int *n_outputs, float *w[10])
{
    if (!v || !v->loaded) { dss_set_error("the decoder handle is NULL or has no weights loaded (dss_dec_load_weights)"); return DSS_EINVAL; }
    *device = v->device; *n_inputs = v->d.C; *hidden_units = v->d.H; *n_outputs = v->d.O;
    for (int k = 0; k < 10; ++k) w[k] = v->w[k];
    return DSS_OK;
}

extern "C" dss_dec *dss_dec_create(int max_streams, int max_frames, int n_inputs, int hidden_units, int n_outputs)
{
    if (max_streams <= 0 || max_frames <= 0 || n_inputs <= 0 || hidden_units <= 0 || n_outputs <= 0) {
        dss_set_error("decoder dims must be positive"); return nullptr;
    }
    if (hidden_units > DSS_DEC_MAXH || n_inputs > DSS_DEC_MAXC || n_outputs > DSS_DEC_MAXO) {
        dss_set_error("decoder kernel: %d hidden units / %d inputs / %d outputs out of range (<= %d / <= %d / <= %d)", hidden_units, n_inputs,
                      n_outputs, DSS_DEC_MAXH, DSS_DEC_MAXC, DSS_DEC_MAXO);
        return nullptr;
    }
    if (dss_ensure_device()) return nullptr;
    dss_dec *v = new dss_dec;
    memset(&v->d, 0, sizeof(v->d));
    hipGetDevice(&v->device);
    v->d.S_max = max_streams; v->d.T_max = max_frames; v->d.C = n_inputs; v->d.H = hidden_units; v->d.O = n_outputs;
    const size_t n = (size_t)max_streams * max_frames * 2 * hidden_units;
    if (v->blocks.alloc<float>(n, &v->d.mid) || v->blocks.alloc<float>(n, &v->d.top) || v->blocks.alloc<int>((size_t)2 * max_streams, &v->d_meta) ||
        v->meta.init((size_t)2 * max_streams)) {
        dss_set_error("device allocation failed for the decoder's layer outputs");
        dss_dec_destroy(v);
        return nullptr;
    }
    return v;
}

extern "C" void dss_dec_destroy(dss_dec *v)
{
    if (!v) return;
    hipSetDevice(v->device);
    v->blocks.free_all();
    v->tstage.destroy();
    v->meta.destroy();
    delete v;
}

// w: 18 host arrays in torch.nn.LSTM's own layout, in state_dict order of the reference class:
//   for layer in (0, 1): for direction in (forward, reverse): weight_ih [4H][Cin], weight_hh [4H][H], bias_ih [4H], bias_hh [4H]
//   (Cin = n_inputs for layer 0, 2H for layer 1), then regressor.weight [O][2H], regressor.bias [O]
extern "C" int dss_dec_load_weights(dss_dec *v, const float *const *w)
{
    if (!v || !w) { dss_set_error("dss_dec_load_weights: null argument"); return DSS_EINVAL; }
    for (int k = 0; k < 18; ++k) if (!w[k]) { dss_set_error("dss_dec_load_weights: null array %d", k); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    const int H = v->d.H, H4 = 4 * H, Hp = (H + 3) & ~3;
    // upload beside the weights in use and switch only when every array has arrived (see dss_vad_load_weights)
    float *nw[10] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    int rc = 0;
    for (int layer = 0; layer < 2; ++layer) {
        const int Cin = layer ? 2 * H : v->d.C, Cp = (Cin + 3) & ~3;
        for (int dir = 0; dir < 2; ++dir) {
            const float *w_ih = w[(layer * 2 + dir) * 4 + 0], *w_hh = w[(layer * 2 + dir) * 4 + 1];
            const float *b_ih = w[(layer * 2 + dir) * 4 + 2], *b_hh = w[(layer * 2 + dir) * 4 + 3];
            // the kernel's copy: [inputs / 4][4H rows][4 consecutive inputs], input counts padded to multiples of 4 with zero weights
            std::vector<float> t((size_t)(Cp + Hp) * H4, 0.f), b(H4);
            dss_pack_rows(t.data(), H4, 0, w_ih, Cin);
            dss_pack_rows(t.data(), H4, Cp, w_hh, H);
            for (int r = 0; r < H4; ++r) b[r] = b_ih[r] + b_hh[r];
            rc |= v->blocks.upload<float>(t.data(), t.size(), &nw[layer * 2 + dir]);
            rc |= v->blocks.upload<float>(b.data(), b.size(), &nw[4 + layer * 2 + dir]);
        }
    }
    rc |= v->blocks.upload<float>(w[16], (size_t)v->d.O * 2 * H, &nw[8]);
    rc |= v->blocks.upload<float>(w[17], (size_t)v->d.O, &nw[9]);
    if (rc) { for (float *p : nw) v->blocks.release(p); return DSS_ENOMEM; }
    DSS_HIP_CHECK(hipDeviceSynchronize());
    for (int k = 0; k < 10; ++k) { v->blocks.release(v->w[k]); v->w[k] = nw[k]; }
    for (int layer = 0; layer < 2; ++layer)
        for (int dir = 0; dir < 2; ++dir) { v->d.wT[layer][dir] = v->w[layer * 2 + dir]; v->d.b[layer][dir] = v->w[4 + layer * 2 + dir]; }
    v->d.wr = v->w[8]; v->d.br = v->w[9];
    v->loaded = true;
    return DSS_OK;
}

// d_frames: (n_streams, n_frames, n_inputs) float64 (frames_are_f64: as the extractor returns them; cast to float32 like
// units.py:503) or float32; d_feats: (n_streams, n_frames, n_outputs) float32.  Device pointers; asynchronous on hip_stream.
// Every call starts from the zero state (units.py:499-508: a fresh state per segment).
extern "C" int dss_dec_forward_dev(dss_dec *v, const void *d_frames, int frames_are_f64, int n_streams, int n_frames, float *d_feats,
                                   void *hip_stream)
{
    if (!v || !d_frames || !d_feats) { dss_set_error("dss_dec_forward_dev: bad arguments"); return DSS_EINVAL; }
    if (!v->loaded) { dss_set_error("dss_dec_forward_dev: no weights loaded (dss_dec_load_weights)"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    return dss_launch_decoder(v->d, d_frames, frames_are_f64, n_streams, n_frames, d_feats, nullptr, nullptr, 0, (hipStream_t)hip_stream);
}

// Ragged form (segments of different lengths closing on the same tick): stream i has counts[i] <= n_frames frames, read from
// row in_rows[i] (NULL: i) of d_frames, a buffer of row_frames frames per row; its backward direction starts at its own last
// frame.  counts / in_rows are HOST arrays.  d_feats is (n_streams, n_frames, n_outputs); rows beyond counts[i] stay untouched.
extern "C" int dss_dec_forward_rows_dev(dss_dec *v, const void *d_frames, int frames_are_f64, int row_frames, const int *in_rows,
                                        const int *counts, int n_streams, int n_frames, float *d_feats, void *hip_stream)
{
    if (!v || !d_frames || !d_feats || !counts) { dss_set_error("dss_dec_forward_rows_dev: bad arguments"); return DSS_EINVAL; }
    if (!v->loaded) { dss_set_error("dss_dec_forward_rows_dev: no weights loaded (dss_dec_load_weights)"); return DSS_EINVAL; }
    if (n_streams < 1 || n_streams > v->d.S_max || n_frames < 1 || n_frames > v->d.T_max || row_frames < n_frames) {
        dss_set_error("dss_dec_forward_rows_dev: %d streams x %d frames (rows of %d) exceed the handle's %d x %d", n_streams, n_frames,
                      row_frames, v->d.S_max, v->d.T_max);
        return DSS_EINVAL;
    }
    for (int i = 0; i < n_streams; ++i) {
        if (counts[i] < 0 || counts[i] > n_frames) { dss_set_error("stream %d: %d frames outside [0, %d]", i, counts[i], n_frames); return DSS_EINVAL; }
        if (in_rows && in_rows[i] < 0) { dss_set_error("stream %d: negative input row", i); return DSS_EINVAL; }
    }
    DSS_HIP_CHECK(hipSetDevice(v->device));
    hipStream_t s = (hipStream_t)hip_stream;
    int *h = v->meta.acquire();
    if (!h) { dss_set_error("pinned staging ring failed"); return DSS_ENODEV; }
    const size_t S = (size_t)v->d.S_max;
    memcpy(h, counts, sizeof(int) * n_streams);
    if (in_rows) memcpy(h + S, in_rows, sizeof(int) * n_streams);
    DSS_HIP_CHECK(hipMemcpyAsync(v->d_meta, h, sizeof(int) * n_streams, hipMemcpyHostToDevice, s));
    if (in_rows) DSS_HIP_CHECK(hipMemcpyAsync(v->d_meta + S, h + S, sizeof(int) * n_streams, hipMemcpyHostToDevice, s));
    int rc = v->meta.commit(s);
    if (rc) return rc;
    return dss_launch_decoder(v->d, d_frames, frames_are_f64, n_streams, n_frames, d_feats, v->d_meta, in_rows ? v->d_meta + S : nullptr,
                              row_frames, s);
}

extern "C" int dss_dec_forward_trials_dev(dss_dec *v, const void *d_frames, int frames_are_f64, long long N, int n_trials,
                                          const long long *first, const int *len, float *d_feats, void *hip_stream)
{
    if (!v || !d_frames || !d_feats) { dss_set_error("dss_dec_forward_trials_dev: bad arguments"); return DSS_EINVAL; }
    if (!v->loaded) { dss_set_error("dss_dec_forward_trials_dev: no weights loaded (dss_dec_load_weights)"); return DSS_EINVAL; }
    long long total = 0;
    int rc = dss_trials_check(N, n_trials, first, len, &total);
    if (rc) return rc;
    for (int i = 0; i < n_trials; ++i) {
        if (len[i] > v->d.T_max) {
            dss_set_error("dss_dec_forward_trials_dev: trial %d has %d frames, the handle takes %d (max_frames)", i, len[i], v->d.T_max);
            return DSS_EINVAL;
        }
        if (first[i] > 0x7fffffffLL) { dss_set_error("dss_dec_forward_trials_dev: trial %d starts behind row 2^31 - 1", i); return DSS_EINVAL; }
    }
    if (!n_trials) return DSS_OK;
    DSS_HIP_CHECK(hipSetDevice(v->device));
    hipStream_t st = (hipStream_t)hip_stream;
    const size_t n = (size_t)n_trials;
    const std::vector<long long> out_row = trials_offsets(n_trials, [&](int i) { return len[i]; });
    const std::vector<int> order = trials_longest_first(n_trials, len);
    long long *tout = (long long *)v->tstage.acquire((sizeof(long long) + 2 * sizeof(int)) * n);      // [n] output rows, then [2][n] ints
    if (!tout) { dss_set_error("pinned staging for the trial table failed"); return DSS_ENOMEM; }
    int *tmeta = (int *)(tout + n);
    for (int k = 0; k < n_trials; ++k) { const int i = order[k]; tmeta[k] = len[i]; tmeta[n + k] = (int)first[i]; tout[k] = out_row[i]; }
    if ((rc = v->d_tmeta.grow(v->blocks, 2 * n)) || (rc = v->d_tout.grow(v->blocks, n))) return rc;
    DSS_HIP_CHECK(hipMemcpyAsync(v->d_tmeta, tmeta, sizeof(int) * 2 * n, hipMemcpyHostToDevice, st));
    DSS_HIP_CHECK(hipMemcpyAsync(v->d_tout, tout, sizeof(long long) * n, hipMemcpyHostToDevice, st));
    if ((rc = v->tstage.commit(st))) return rc;
    // chunks of max_streams trials share the handle's layer buffers one after the other; longest first, so a chunk's trials are of
    // similar length and its padded (trials x longest) grid holds little padding
    for (int k0 = 0; k0 < n_trials; k0 += v->d.S_max) {
        const int S = std::min(v->d.S_max, n_trials - k0), T = len[order[k0]];
        rc = dss_launch_decoder_trials(v->d, d_frames, frames_are_f64, S, T, d_feats, v->d_tmeta + k0, v->d_tmeta + n + k0, v->d_tout + k0, st);
        if (rc) return rc;
    }
    return DSS_OK;
}

extern "C" int dss_dec_mse_trials_dev(const float *d_feats, const float *d_targets, int n_outputs, int n_trials, const int *len,
                                      double *d_mse, void *hip_stream)
{
    if (!d_feats || !d_targets || !d_mse || n_outputs < 1) { dss_set_error("dss_dec_mse_trials_dev: bad arguments"); return DSS_EINVAL; }
    return trials_reduce("dss_dec_mse_trials_dev", n_trials, len, [&](const DssTrialLens &tl) {
        return dss_launch_dec_mse_trials(tl, d_feats, d_targets, n_outputs, d_mse, (hipStream_t)hip_stream);
    });
}
