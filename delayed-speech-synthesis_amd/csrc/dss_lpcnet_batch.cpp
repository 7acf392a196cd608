// csrc/dss_lpcnet_batch.cpp -- the batched vocoder of the C ABI (include/dss_hip.h), its lanes, and the xiph drop-in
// symbols on top of it.  Owns the decoder state, the per-call scratch and the launch ordering; the arithmetic runs in
// lpcnet_frame.hip and the lpcnet_sample*.hip kernels.
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <vector>

#include "dss_host.h"

// ------------------------------------------------------------------------------------------------------
// batched decoder
// ------------------------------------------------------------------------------------------------------
struct dss_lpcnet_batch {
    int device;
    HostModel *host_model;        // keeps the model (and its device copy) alive
    const DssModelDev *model;
    DssBatchDev d;
    DssDevBlocks blocks;          // a lane's: its scratch; a parent's: the decoder state too
    int last_utts = 0, last_frames = 0;
    int force_utts = 0, force_frames = 0;   // shape force_exc / trace_logits were sized for (dss_lpcnet_batch_force_excitation)
    int trace = 0, timing = 0;
    int pair = 0;                 // 0 auto, -1 never, 2 always: two utterances per workgroup (dss_lpcnet_batch_set_multi)
    int max_rows = 0;             // rows one call may carry (= scratch rows); d.max_utts = decoder slots (a lane: its parent's)
    dss_lpcnet_batch *parent = nullptr;   // a lane (dss_lpcnet_batch_create_lane): decoder state aliases the parent's arrays
    int lanes = 0;                // live lanes of this (parent) batch
    bool dead = false;            // destroyed by the caller while lanes were alive: freed with the last lane
    float *d_feat = nullptr;      // staging for the host-buffer entry point
    short *d_pcm = nullptr;
    int *d_slots = nullptr;       // [max_rows] slot list of a ragged call
    int *d_counts = nullptr;      // [max_rows] frame counts of a ragged call
    int *d_order = nullptr;       // [max_rows] dispatch order of a ragged call: rows by decreasing frame count
    DssPinnedRing meta;           // pinned staging of those three lists ([3][max_rows] ints per slot of the ring)
    hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
    double ms_sum[2] = {0, 0};
    int ms_n = 0;
};

// per-call scratch (rows x frames), the staging buffers and the events: what a plain batch and a lane both own
static int batch_alloc_scratch(dss_lpcnet_batch *b, int max_rows, int max_frames)
{
    DssBatchDev &d = b->d;
    b->max_rows = max_rows; d.max_frames = max_frames;
    const size_t B = max_rows, F = max_frames;
    int rc = 0;
    rc |= b->blocks.alloc<float>(B * (F + 2) * 84, &d.in_buf);
    rc |= b->blocks.alloc<float>(B * (F + 2) * 128, &d.c1_buf);
    rc |= b->blocks.alloc<float>(B * F * 128, &d.c2_buf);
    rc |= b->blocks.alloc<float>(B * F * 128, &d.d1_buf);
    rc |= b->blocks.alloc<float>(B * F * 128, &d.cond_buf);
    rc |= b->blocks.alloc<float>(B * (F + 2) * 16, &d.lpc_buf);
    rc |= b->blocks.alloc<float>(B * F * DSS_COND_STRIDE, &d.frame_out);
    rc |= b->blocks.alloc<int>(B, &d.fc0);
    rc |= b->blocks.alloc<float>(B * F * 20, &b->d_feat);
    rc |= b->blocks.alloc<short>(B * F * DSS_FRAME_SIZE, &b->d_pcm);
    rc |= b->blocks.alloc<int>(B, &b->d_slots);
    rc |= b->blocks.alloc<int>(B, &b->d_counts);
    rc |= b->blocks.alloc<int>(B, &b->d_order);
    rc |= b->meta.init(3 * B);
    for (int i = 0; i < 3; ++i) rc |= (hipEventCreate(&b->ev[i]) != hipSuccess);
    return rc;
}

extern "C" dss_lpcnet_batch *dss_lpcnet_batch_create(int max_utts, int max_frames)
{
    if (max_utts <= 0 || max_frames <= 0) { dss_set_error("batch dims must be positive"); return nullptr; }
    HostModel *hm; const DssModelDev *m;
    if (get_model(&hm, &m, true)) return nullptr;            // holds one reference from here on (dropped by destroy)
    dss_lpcnet_batch *b = new dss_lpcnet_batch;
    memset(&b->d, 0, sizeof(b->d));
    hipGetDevice(&b->device);
    b->host_model = hm;
    b->model = m;
    DssBatchDev &d = b->d;
    d.max_utts = max_utts;
    const size_t B = max_utts;
    int rc = 0;
    rc |= b->blocks.alloc<float>(B * DSS_GRU_A, &d.gru_a_state);
    rc |= b->blocks.alloc<float>(B * DSS_GRU_B, &d.gru_b_state);
    rc |= b->blocks.alloc<float>(B * 16, &d.last_sig);
    rc |= b->blocks.alloc<int>(B, &d.last_exc);
    rc |= b->blocks.alloc<float>(B, &d.deemph);
    rc |= b->blocks.alloc<uint32_t>(B * 4, &d.rng);
    rc |= b->blocks.alloc<int>(B, &d.frame_count);
    rc |= b->blocks.alloc<float>(B * 2 * 84, &d.conv1_mem);
    rc |= b->blocks.alloc<float>(B * 2 * 128, &d.conv2_mem);
    rc |= b->blocks.alloc<float>(B * 2 * 16, &d.old_lpc);
    rc |= batch_alloc_scratch(b, max_utts, max_frames);
    if (rc) {
        dss_set_error("device allocation failed for batch %d x %d", max_utts, max_frames);
        dss_lpcnet_batch_destroy(b);
        return nullptr;
    }
    if (dss_launch_lpcnet_reset(*m, d, -1, 0) || hipDeviceSynchronize() != hipSuccess) { dss_lpcnet_batch_destroy(b); return nullptr; }
    return b;
}

// A lane: a second launch context on the decoder states of `parent`.  It owns scratch for max_rows x max_frames and nothing
// else; its rows name the parent's slots (ragged calls with a slot list).  Lanes exist so that calls touching DIFFERENT slots
// can be in flight on different streams at once (the asynchronous segment synthesis of the gated streaming mode).
extern "C" dss_lpcnet_batch *dss_lpcnet_batch_create_lane(dss_lpcnet_batch *parent, int max_rows, int max_frames)
{
    if (!parent || parent->parent || parent->dead || max_rows <= 0 || max_frames <= 0) {
        dss_set_error("dss_lpcnet_batch_create_lane: needs a live batch that is not itself a lane, and positive dims");
        return nullptr;
    }
    if (hipSetDevice(parent->device) != hipSuccess) { dss_set_error("hipSetDevice failed"); return nullptr; }
    dss_lpcnet_batch *b = new dss_lpcnet_batch;
    b->d = parent->d;                              // the state arrays (and max_utts = the slot count) are the parent's
    DssBatchDev &d = b->d;
    d.in_buf = d.c1_buf = d.c2_buf = d.d1_buf = d.cond_buf = d.lpc_buf = d.frame_out = nullptr;
    d.fc0 = nullptr; d.slot_of = d.count_of = d.row_of = nullptr; d.utt0 = 0;
    d.trace_exc = d.trace_pcm = d.trace_logits = nullptr; d.force_exc = nullptr;
    b->device = parent->device;
    b->host_model = parent->host_model;
    b->model = parent->model;
    b->pair = parent->pair;
    b->parent = parent;
    parent->lanes += 1;
    if (batch_alloc_scratch(b, max_rows, max_frames)) {
        dss_set_error("device allocation failed for lane %d x %d", max_rows, max_frames);
        dss_lpcnet_batch_destroy(b);
        return nullptr;
    }
    return b;
}

static void batch_free(dss_lpcnet_batch *b)
{
    b->blocks.free_all();
    b->meta.destroy();
    for (int i = 0; i < 3; ++i) if (b->ev[i]) hipEventDestroy(b->ev[i]);
    if (!b->parent) release_model(b->host_model);
    delete b;
}

extern "C" void dss_lpcnet_batch_destroy(dss_lpcnet_batch *b)
{
    if (!b) return;
    hipSetDevice(b->device);
    hipDeviceSynchronize();                        // nothing of this object may still be in flight on any stream
    if (b->parent) {
        dss_lpcnet_batch *p = b->parent;
        batch_free(b);
        if (--p->lanes == 0 && p->dead) batch_free(p);
        return;
    }
    if (b->lanes > 0) { b->dead = true; return; }  // its lanes still run on its state: freed with the last of them
    batch_free(b);
}

extern "C" int dss_lpcnet_batch_reset(dss_lpcnet_batch *b, int utt)
{
    if (!b || utt >= b->d.max_utts) { dss_set_error("bad batch/utt"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(b->device));
    int rc = dss_launch_lpcnet_reset(*b->model, b->d, utt, 0);
    if (rc) return rc;
    DSS_HIP_CHECK(hipStreamSynchronize(0));
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_reset_async(dss_lpcnet_batch *b, int utt, void *hip_stream)
{
    if (!b || utt >= b->d.max_utts) { dss_set_error("bad batch/utt"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(b->device));
    return dss_launch_lpcnet_reset(*b->model, b->d, utt, (hipStream_t)hip_stream);
}

extern "C" int dss_lpcnet_batch_enable_trace(dss_lpcnet_batch *b, int on)
{
    if (!b) return DSS_EINVAL;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    if (on && !b->d.trace_exc) {
        const size_t n = (size_t)b->max_rows * b->d.max_frames * DSS_FRAME_SIZE;
        int rc = b->blocks.alloc<float>(n, &b->d.trace_exc);
        rc |= b->blocks.alloc<float>(n, &b->d.trace_pcm);
        if (rc) return DSS_ENOMEM;
    }
    b->trace = on;      // 1 = excitation/pcm trace, 2 = diagnostic phase stamps (development only)
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_force_excitation(dss_lpcnet_batch *b, const unsigned char *exc, int n_utts, int n_frames)
{
    if (!b) return DSS_EINVAL;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    if (!exc) {                                   // back to free running
        b->blocks.release(b->d.force_exc);
        b->blocks.release(b->d.trace_logits);
        b->d.force_exc = nullptr; b->d.trace_logits = nullptr;
        b->force_utts = b->force_frames = 0;
        return DSS_OK;
    }
    if (n_utts <= 0 || n_utts > b->max_rows || n_frames <= 0 || n_frames > b->d.max_frames) {
        dss_set_error("forced excitation shape out of range"); return DSS_EINVAL;
    }
    if (!b->trace) { dss_set_error("teacher forcing needs dss_lpcnet_batch_enable_trace(b, 1 or 17) first"); return DSS_EINVAL; }
    const size_t n = (size_t)n_utts * n_frames * DSS_FRAME_SIZE;
    b->blocks.release(b->d.force_exc);
    b->blocks.release(b->d.trace_logits);
    b->d.force_exc = nullptr; b->d.trace_logits = nullptr;
    b->force_utts = b->force_frames = 0;
    unsigned char *de = nullptr;
    if (b->blocks.upload<unsigned char>(exc, n, &de)) return DSS_ENOMEM;
    b->d.force_exc = de;
    if (b->blocks.alloc<float>(n * 256, &b->d.trace_logits)) return DSS_ENOMEM;
    b->force_utts = n_utts; b->force_frames = n_frames;
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_set_multi(dss_lpcnet_batch *b, int utterances_per_workgroup)
{
    if (!b) return DSS_EINVAL;
    const int u = utterances_per_workgroup;
    if (!(u == 0 || u == -1 || u == 1 || u == 2)) { dss_set_error("utterances per workgroup: 0 (auto), 1 or -1 (always one), 2 (always two)"); return DSS_EINVAL; }
    if (u == 2 && !dss_pair_fits(*b->model)) { dss_set_error("two utterances per workgroup do not fit beside this model in LDS (or it needs the extended paths)"); return DSS_EINVAL; }
    b->pair = u == 1 ? -1 : u;
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_enable_timing(dss_lpcnet_batch *b, int on)
{
    if (!b) return DSS_EINVAL;
    b->timing = on ? 1 : 0;
    b->ms_sum[0] = b->ms_sum[1] = 0; b->ms_n = 0;
    return DSS_OK;
}

extern "C" double dss_lpcnet_batch_kernel_ms(dss_lpcnet_batch *b, int which)
{
    if (!b || b->ms_n == 0 || which < 0 || which > 1) return 0.0;
    double v = b->ms_sum[which] / b->ms_n;
    return v;
}

static int check_batch_shape(dss_lpcnet_batch *b, int n_utts, int n_frames, int feat_stride)
{
    if (b->dead) { dss_set_error("this batch was destroyed (only its lanes are alive)"); return DSS_EINVAL; }
    if (n_utts <= 0 || n_utts > b->max_rows || n_frames <= 0 || n_frames > b->d.max_frames || feat_stride < DSS_NB_FEATURES) {
        dss_set_error("shape out of range: %d utts (max %d), %d frames (max %d), stride %d", n_utts, b->max_rows, n_frames,
                      b->d.max_frames, feat_stride);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

// frame-rate network, then the persistent sample-rate kernel, on stream s; b->d.slot_of / count_of select the
// uniform (NULL) or the ragged form
static int run_batch(dss_lpcnet_batch *b, const float *d_features, int n_utts, int n_frames, int feat_stride, short *d_pcm,
                     hipStream_t s, int *d_frames_done = nullptr)
{
    // the kernels index the forced excitation and the logit trace with the CALL's shape: it must be the shape they were
    // sized for, and a uniform call (the trace build would launch a ragged one as if every row were full)
    if (b->d.force_exc || b->d.trace_logits) {
        if (n_utts != b->force_utts || n_frames != b->force_frames || b->d.slot_of || b->d.count_of) {
            dss_set_error("teacher forcing was set up for %d x %d frames, uniform calls only; this call is %d x %d%s",
                          b->force_utts, b->force_frames, n_utts, n_frames, (b->d.slot_of || b->d.count_of) ? " (ragged)" : "");
            return DSS_EINVAL;
        }
    }
    if (b->timing) DSS_HIP_CHECK(hipEventRecord(b->ev[0], s));
    int rc = dss_launch_frame_network(*b->model, b->d, d_features, n_utts, n_frames, feat_stride, s);
    if (rc) return rc;
    if (b->timing) DSS_HIP_CHECK(hipEventRecord(b->ev[1], s));
    rc = dss_launch_sample_network(*b->model, b->d, n_utts, n_frames, d_pcm, b->trace, b->pair, s, d_frames_done);
    if (rc) return rc;
    if (b->timing) {
        DSS_HIP_CHECK(hipEventRecord(b->ev[2], s));
        DSS_HIP_CHECK(hipEventSynchronize(b->ev[2]));
        float fr = 0, sm = 0;
        DSS_HIP_CHECK(hipEventElapsedTime(&fr, b->ev[0], b->ev[1]));
        DSS_HIP_CHECK(hipEventElapsedTime(&sm, b->ev[1], b->ev[2]));
        b->ms_sum[0] += sm; b->ms_sum[1] += fr; b->ms_n += 1;
    }
    b->last_utts = n_utts; b->last_frames = n_frames;
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_synthesize_dev(dss_lpcnet_batch *b, const float *d_features, int n_utts, int n_frames,
                                               int feat_stride, short *d_pcm, void *hip_stream)
{
    if (!b || !d_features || !d_pcm) { dss_set_error("null argument"); return DSS_EINVAL; }
    int rc = check_batch_shape(b, n_utts, n_frames, feat_stride);
    if (rc) return rc;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    b->d.slot_of = nullptr; b->d.count_of = nullptr; b->d.row_of = nullptr;
    return run_batch(b, d_features, n_utts, n_frames, feat_stride, d_pcm, (hipStream_t)hip_stream);
}

// Validate and upload the slot list / frame counts of a ragged call (either may be NULL).  The lists go through a pinned
// ring (dss_host.h): the upload neither waits for what is queued on `s` nor can a later call overwrite it before it has run.
static int stage_ragged(dss_lpcnet_batch *b, const int *slots, const int *counts, int n_utts, int n_frames, hipStream_t s)
{
    b->d.slot_of = nullptr; b->d.count_of = nullptr; b->d.row_of = nullptr;
    if (slots) {
        std::string seen((size_t)b->d.max_utts, 0);
        for (int i = 0; i < n_utts; ++i) {
            if (slots[i] < 0 || slots[i] >= b->d.max_utts) { dss_set_error("row %d: slot %d out of range (max %d)", i, slots[i], b->d.max_utts); return DSS_EINVAL; }
            if (seen[slots[i]]) { dss_set_error("row %d: slot %d appears twice in one call (a decoder is sequential)", i, slots[i]); return DSS_EINVAL; }
            seen[slots[i]] = 1;
        }
    } else if (n_utts > b->d.max_utts) {
        dss_set_error("%d rows without a slot list, %d decoder slots", n_utts, b->d.max_utts); return DSS_EINVAL;
    }
    if (counts)
        for (int i = 0; i < n_utts; ++i)
            if (counts[i] < 0 || counts[i] > n_frames) { dss_set_error("row %d: %d frames outside [0, %d]", i, counts[i], n_frames); return DSS_EINVAL; }
    if (!slots && !counts) return DSS_OK;
    int *h = b->meta.acquire();
    if (!h) { dss_set_error("pinned staging ring failed"); return DSS_ENODEV; }
    const size_t R = (size_t)b->max_rows;
    if (slots) {
        memcpy(h, slots, sizeof(int) * n_utts);
        DSS_HIP_CHECK(hipMemcpyAsync(b->d_slots, h, sizeof(int) * n_utts, hipMemcpyHostToDevice, s));
        b->d.slot_of = b->d_slots;
    }
    if (counts) {
        memcpy(h + R, counts, sizeof(int) * n_utts);
        DSS_HIP_CHECK(hipMemcpyAsync(b->d_counts, h + R, sizeof(int) * n_utts, hipMemcpyHostToDevice, s));
        b->d.count_of = b->d_counts;
        // Dispatch order: workgroups start in grid order, so the longest rows go first whatever order the caller used
        // (and the pair kernel's two rows of a workgroup are neighbours in length).  Results do not depend on it.
        int *order = h + 2 * R;
        for (int i = 0; i < n_utts; ++i) order[i] = i;
        std::stable_sort(order, order + n_utts, [&](int x, int y) { return counts[x] > counts[y]; });
        DSS_HIP_CHECK(hipMemcpyAsync(b->d_order, order, sizeof(int) * n_utts, hipMemcpyHostToDevice, s));
        b->d.row_of = b->d_order;
    }
    return b->meta.commit(s);
}

extern "C" int dss_lpcnet_batch_synthesize_ragged_dev(dss_lpcnet_batch *b, const float *d_features, const int *slots,
                                                      const int *counts, int n_utts, int n_frames, int feat_stride,
                                                      short *d_pcm, void *hip_stream)
{
    if (!b || !d_features || !d_pcm) { dss_set_error("null argument"); return DSS_EINVAL; }
    int rc = check_batch_shape(b, n_utts, n_frames, feat_stride);
    if (rc) return rc;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    hipStream_t s = (hipStream_t)hip_stream;
    rc = stage_ragged(b, slots, counts, n_utts, n_frames, s);
    if (rc) return rc;
    return run_batch(b, d_features, n_utts, n_frames, feat_stride, d_pcm, s);
}

// The ragged call with per-frame delivery: PCM goes straight into fine-grained host memory and host_frames_done[row] counts the
// frames of each row already there (include/dss_hip.h).  Everything is checked before anything is enqueued.
extern "C" int dss_lpcnet_batch_synthesize_ragged_progress_dev(dss_lpcnet_batch *b, const float *d_features, const int *slots,
                                                               const int *counts, int n_utts, int n_frames, int feat_stride,
                                                               short *host_pcm, int *host_frames_done, void *hip_stream)
{
    if (!b || !d_features || !host_pcm || !host_frames_done) { dss_set_error("null argument"); return DSS_EINVAL; }
    int rc = check_batch_shape(b, n_utts, n_frames, feat_stride);
    if (rc) return rc;
    if ((b->trace & 15) || b->d.force_exc || b->d.trace_logits) {
        dss_set_error("progressive calls run without trace or teacher forcing (trace %d%s)", b->trace, b->d.force_exc ? ", forced excitation" : "");
        return DSS_EINVAL;
    }
    DSS_HIP_CHECK(hipSetDevice(b->device));
    void *d_pcm = nullptr, *d_done = nullptr;
    rc = dss_fine_host_view(host_pcm, (size_t)n_utts * n_frames * DSS_FRAME_SIZE * sizeof(short), 16, "host_pcm", &d_pcm);
    if (rc) return rc;
    rc = dss_fine_host_view(host_frames_done, (size_t)n_utts * sizeof(int), sizeof(int), "host_frames_done", &d_done);
    if (rc) return rc;
    for (int i = 0; i < n_utts; ++i) __atomic_store_n(host_frames_done + i, 0, __ATOMIC_RELAXED);   // before anything is enqueued
    hipStream_t s = (hipStream_t)hip_stream;
    rc = stage_ragged(b, slots, counts, n_utts, n_frames, s);
    if (rc) return rc;
    return run_batch(b, d_features, n_utts, n_frames, feat_stride, (short *)d_pcm, s, (int *)d_done);
}

extern "C" int dss_lpcnet_batch_synthesize_ragged(dss_lpcnet_batch *b, const float *features, const int *slots,
                                                  const int *counts, int n_utts, int n_frames, int feat_stride, short *pcm)
{
    if (!b || !features || !pcm) { dss_set_error("null argument"); return DSS_EINVAL; }
    int rc = check_batch_shape(b, n_utts, n_frames, feat_stride);
    if (rc) return rc;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    rc = stage_ragged(b, slots, counts, n_utts, n_frames, nullptr);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy2D(b->d_feat, DSS_NB_FEATURES * sizeof(float), features, (size_t)feat_stride * sizeof(float),
                              DSS_NB_FEATURES * sizeof(float), (size_t)n_utts * n_frames, hipMemcpyHostToDevice));
    rc = run_batch(b, b->d_feat, n_utts, n_frames, DSS_NB_FEATURES, b->d_pcm, nullptr);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(pcm, b->d_pcm, (size_t)n_utts * n_frames * DSS_FRAME_SIZE * sizeof(short), hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_synthesize(dss_lpcnet_batch *b, const float *features, int n_utts, int n_frames,
                                           int feat_stride, short *pcm)
{
    if (!b || !features || !pcm) { dss_set_error("null argument"); return DSS_EINVAL; }
    if (check_batch_shape(b, n_utts, n_frames, feat_stride)) return DSS_EINVAL;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    // pack the first 20 floats of every row (feature files carry 36, LPCNet.pyx:97,115)
    DSS_HIP_CHECK(hipMemcpy2D(b->d_feat, DSS_NB_FEATURES * sizeof(float), features, (size_t)feat_stride * sizeof(float),
                              DSS_NB_FEATURES * sizeof(float), (size_t)n_utts * n_frames, hipMemcpyHostToDevice));
    int rc = dss_lpcnet_batch_synthesize_dev(b, b->d_feat, n_utts, n_frames, DSS_NB_FEATURES, b->d_pcm, nullptr);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(pcm, b->d_pcm, (size_t)n_utts * n_frames * DSS_FRAME_SIZE * sizeof(short), hipMemcpyDeviceToHost));
    return DSS_OK;
}

extern "C" int dss_lpcnet_batch_tap(dss_lpcnet_batch *b, int utt, int which, float *out, size_t n_floats)
{
    if (!b || !out || utt < 0 || utt >= b->last_utts) { dss_set_error("bad tap arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(b->device));
    DSS_HIP_CHECK(hipDeviceSynchronize());
    const int F = b->last_frames;
    if (which >= 0 && which <= 2) {
        const int width = which == 0 ? 3 * DSS_GRU_A : which == 1 ? 3 * DSS_GRU_B : DSS_LPC_ORDER;
        const int off = which == 0 ? 0 : which == 1 ? 3 * DSS_GRU_A : 3 * DSS_GRU_A + 3 * DSS_GRU_B;
        if (n_floats < (size_t)F * width) { dss_set_error("tap buffer too small"); return DSS_EINVAL; }
        DSS_HIP_CHECK(hipMemcpy2D(out, width * sizeof(float), b->d.frame_out + (size_t)utt * F * DSS_COND_STRIDE + off,
                                  DSS_COND_STRIDE * sizeof(float), width * sizeof(float), F, hipMemcpyDeviceToHost));
        return DSS_OK;
    }
    if (which == 5 && b->d.trace_logits) {
        const size_t n = (size_t)F * DSS_FRAME_SIZE * 256;
        if (n_floats < n) { dss_set_error("tap buffer too small"); return DSS_EINVAL; }
        DSS_HIP_CHECK(hipMemcpy(out, b->d.trace_logits + (size_t)utt * n, n * sizeof(float), hipMemcpyDeviceToHost));
        return DSS_OK;
    }
    if ((which == 3 || which == 4) && b->d.trace_exc) {
        const size_t n = (size_t)F * DSS_FRAME_SIZE;
        if (n_floats < n) { dss_set_error("tap buffer too small"); return DSS_EINVAL; }
        const float *src = (which == 3 ? b->d.trace_exc : b->d.trace_pcm) + (size_t)utt * n;
        DSS_HIP_CHECK(hipMemcpy(out, src, n * sizeof(float), hipMemcpyDeviceToHost));
        return DSS_OK;
    }
    dss_set_error("unknown tap %d (or trace not enabled)", which);
    return DSS_EINVAL;
}

// ------------------------------------------------------------------------------------------------------
// xiph drop-in symbols: one state = a batch of one utterance, one frame per call
// ------------------------------------------------------------------------------------------------------
// One frame per call is a fixed sequence of ten small launches between two tiny copies (what an unchanged decode_online.py
// pays per 10 ms, local/units.py:531-538).  From its second call on, a state replays that sequence from a HIP graph captured
// once on a stream of its own: pinned staging for the 80 bytes in and the 320 bytes out, one hipGraphLaunch, one wait.
struct LPCNetState {
    dss_lpcnet_batch *b;
    hipStream_t stream = nullptr;
    hipGraphExec_t exec = nullptr;
    float *h_feat = nullptr;          // pinned
    short *h_pcm = nullptr;           // pinned
    long calls = 0;
    int graph_off = 0;                // capture failed once (or DSS_LEVEL1_EAGER is set): eager launches from then on
};

extern "C" LPCNetState *lpcnet_create(void)
{
    dss_lpcnet_batch *b = dss_lpcnet_batch_create(1, 1);
    if (!b) return nullptr;
    LPCNetState *st = new LPCNetState;
    st->b = b;
    st->graph_off = getenv("DSS_LEVEL1_EAGER") != nullptr;
    return st;
}

extern "C" int lpcnet_init(LPCNetState *st)
{
    if (!st) return -1;
    if (st->stream) hipStreamSynchronize(st->stream);
    return dss_lpcnet_batch_reset(st->b, -1);
}

extern "C" void lpcnet_destroy(LPCNetState *st)
{
    if (!st) return;
    hipSetDevice(st->b->device);
    if (st->stream) hipStreamSynchronize(st->stream);
    if (st->exec) hipGraphExecDestroy(st->exec);
    if (st->stream) hipStreamDestroy(st->stream);
    if (st->h_feat) hipHostFree(st->h_feat);
    if (st->h_pcm) hipHostFree(st->h_pcm);
    dss_lpcnet_batch_destroy(st->b);
    delete st;
}

// one frame through the captured graph; DSS_OK, or an error after which the caller falls back to the eager path for good
#define DSS_EINTERNAL_REPLAY (-1000)      // the replay itself failed (the frame was enqueued): see lpcnet_synthesize
static int level1_graph_frame(LPCNetState *st, const float *features, short *output)
{
    dss_lpcnet_batch *b = st->b;
    DSS_HIP_CHECK(hipSetDevice(b->device));
    if (!st->stream) {
        DSS_HIP_CHECK(hipStreamCreateWithFlags(&st->stream, hipStreamNonBlocking));
        DSS_HIP_CHECK(hipHostMalloc((void **)&st->h_feat, DSS_NB_FEATURES * sizeof(float), hipHostMallocDefault));
        DSS_HIP_CHECK(hipHostMalloc((void **)&st->h_pcm, DSS_FRAME_SIZE * sizeof(short), hipHostMallocDefault));
    }
    memcpy(st->h_feat, features, DSS_NB_FEATURES * sizeof(float));
    if (!st->exec) {
        hipGraph_t graph = nullptr;
        DSS_HIP_CHECK(hipStreamBeginCapture(st->stream, hipStreamCaptureModeThreadLocal));
        hipError_t e1 = hipMemcpyAsync(b->d_feat, st->h_feat, DSS_NB_FEATURES * sizeof(float), hipMemcpyHostToDevice, st->stream);
        b->d.slot_of = nullptr; b->d.count_of = nullptr; b->d.row_of = nullptr;
        const int rc = e1 == hipSuccess ? run_batch(b, b->d_feat, 1, 1, DSS_NB_FEATURES, b->d_pcm, st->stream) : DSS_ENODEV;
        hipError_t e2 = hipMemcpyAsync(st->h_pcm, b->d_pcm, DSS_FRAME_SIZE * sizeof(short), hipMemcpyDeviceToHost, st->stream);
        hipError_t e3 = hipStreamEndCapture(st->stream, &graph);             // always ends the capture
        if (rc || e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || !graph) {
            if (graph) hipGraphDestroy(graph);
            (void)hipGetLastError();
            dss_set_error("level-1 graph capture failed; staying on eager launches");
            return DSS_ENODEV;
        }
        hipError_t e4 = hipGraphInstantiate(&st->exec, graph, nullptr, nullptr, 0);
        hipGraphDestroy(graph);
        if (e4 != hipSuccess) { st->exec = nullptr; dss_set_error("hipGraphInstantiate failed: %s", hipGetErrorString(e4)); return DSS_ENODEV; }
    }
    // From here on the frame IS enqueued: a failure must not be answered with an eager re-run (the decoder state may have
    // advanced already), so it gets its own code: the caller zero-fills this frame and stays eager afterwards.
    if (hipGraphLaunch(st->exec, st->stream) != hipSuccess || hipStreamSynchronize(st->stream) != hipSuccess) {
        dss_set_error("level-1 graph replay failed: %s", hipGetErrorString(hipGetLastError()));
        return DSS_EINTERNAL_REPLAY;
    }
    memcpy(output, st->h_pcm, DSS_FRAME_SIZE * sizeof(short));
    b->last_utts = 1; b->last_frames = 1;
    return DSS_OK;
}

// The xiph ABI gives this call no error channel (void; cLPCNet.pxd:13) and its caller is a live prosthesis loop
// (local/units.py:534-535): never abort the process.  On failure the frame is ZERO-FILLED (silence), the reason is
// kept in dss_last_error(), counted in dss_error_count(), and printed to stderr the first time and then every 1000th.
static std::atomic<long> g_synth_failures{0};

extern "C" long dss_error_count(void) { return g_synth_failures.load(); }

static void synth_failed(short *output, int N)
{
    if (output && N > 0) memset(output, 0, sizeof(short) * (size_t)N);
    const long k = g_synth_failures.fetch_add(1);
    if (k == 0 || k % 1000 == 0) fprintf(stderr, "libdss_hip: lpcnet_synthesize failed (%ld so far), frame zero-filled: %s\n", k + 1, dss_last_error());
}

extern "C" void lpcnet_synthesize(LPCNetState *st, const float *features, short *output, int N)
{
    if (!st || !features || !output) { dss_set_error("lpcnet_synthesize: null argument"); synth_failed(output, N); return; }
    if (N != DSS_FRAME_SIZE) {           // the reference only ever asks for one 160-sample frame (LPCNet.pyx:39)
        dss_set_error("lpcnet_synthesize: N must be %d, got %d", DSS_FRAME_SIZE, N);
        synth_failed(output, N);
        return;
    }
    // first call of a state: eager (it also sets the kernels' attributes); traced or timed states stay eager
    if (st->calls++ > 0 && !st->graph_off && !st->b->trace && !st->b->timing) {
        const int grc = level1_graph_frame(st, features, output);
        if (grc == DSS_OK) return;
        st->graph_off = 1;               // eager launches from now on
        // a failed capture or instantiation enqueued nothing: this frame runs eagerly below.  A failed replay may have
        // advanced the decoder: silence for this one frame, no second pass over the same features.
        if (grc == DSS_EINTERNAL_REPLAY) { synth_failed(output, N); return; }
    }
    if (dss_lpcnet_batch_synthesize(st->b, features, 1, 1, DSS_NB_FEATURES, output)) synth_failed(output, N);
}

extern "C" int lpcnet_get_size(void) { return (int)sizeof(LPCNetState); }

// ---- encoder half of the bound ABI (cLPCNet.pxd:15-19; LPCNet.pyx:43-87) -----------------------------------------
// The feature ENCODER (pitch search, Bark cepstrum of a PCM frame) is corpus preparation (prepare_corpus.py:72-73), which
// drives it 160 samples at a time on one state.  The encoder this library has (Parts 16 and 18) is this project's statement
// of the published method, with parity to xiph's code unpinned, so it never stands in for xiph's silently: the symbols are
// bound to it only where the environment says DSS_LPCNET_ENCODER=1 when lpcnet_encoder_create() is called.  Otherwise create
// returns NULL, which the reference's wrapper turns into MemoryError (LPCNet.pyx:53-56), so a caller finds out at
// construction time, not from features of another method.  A state wraps a one-stream handle of Part 18.
struct LPCNetEncState { dss_fenc_streams *h; };

static bool encoder_opted_in()
{
    const char *e = getenv("DSS_LPCNET_ENCODER");
    return e && !strcmp(e, "1");
}

extern "C" LPCNetEncState *lpcnet_encoder_create(void)
{
    if (!encoder_opted_in()) {
        dss_set_error("LPCNet feature encoder is not provided by libdss_hip (corpus preparation is outside the accelerated path)");
        return nullptr;
    }
    dss_fenc_streams *h = dss_fenc_streams_create(1);
    if (!h) {
        char why[400];
        snprintf(why, sizeof(why), "%s", dss_last_error());
        dss_set_error("LPCNet feature encoder (DSS_LPCNET_ENCODER=1): %s", why);
        return nullptr;
    }
    return new LPCNetEncState{h};
}
extern "C" int lpcnet_encoder_init(LPCNetEncState *st)
{
    if (!st) return -1;
    return dss_fenc_streams_reset(st->h, nullptr, 0, nullptr) ? -1 : 0;
}
extern "C" void lpcnet_encoder_destroy(LPCNetEncState *st)
{
    if (!st) return;
    dss_fenc_streams_destroy(st->h);
    delete st;
}
// The published form quantises four frames through packet codebooks that are not at hand, and the reference never calls it:
// a failing stub whatever the environment says.
extern "C" int lpcnet_compute_features(LPCNetEncState *, const short *, float (*features)[36])
{
    if (features) memset(features, 0, sizeof(float) * 4 * 36);
    dss_set_error("lpcnet_compute_features: encoder not provided by libdss_hip");
    return -1;
}
extern "C" long long dss_lpcnet_encoder_frames(LPCNetEncState *st, const short *pcm, int n_frames, float *out36)
{
    if (!st || n_frames < 0 || (n_frames && (!pcm || !out36))) { dss_set_error("dss_lpcnet_encoder_frames: bad arguments"); return DSS_EINVAL; }
    return dss_fenc_streams_push(st->h, pcm, n_frames, nullptr, out36);
}
extern "C" int lpcnet_compute_single_frame_features(LPCNetEncState *st, const short *pcm, float *features)
{
    if (!st) {
        if (features) memset(features, 0, sizeof(float) * 36);
        dss_set_error("lpcnet_compute_single_frame_features: encoder not provided by libdss_hip");
        return -1;
    }
    if (pcm && features && dss_fenc_streams_push(st->h, pcm, 1, nullptr, features) == 1) return 0;
    if (!pcm || !features) dss_set_error("lpcnet_compute_single_frame_features: null argument");
    if (features) memset(features, 0, sizeof(float) * 36);
    const long k = g_synth_failures.fetch_add(1);
    if (k == 0 || k % 1000 == 0)
        fprintf(stderr, "libdss_hip: lpcnet_compute_single_frame_features failed (%ld so far), features zero-filled: %s\n", k + 1, dss_last_error());
    return -1;
}
// cLPCNet.pxd:22-23 declares decode_packet inside a stray header block; nothing calls it

extern "C" int dss_selftest_exp10(const float *x, const float *comp, float *out, long n)
{
    if (!x || !comp || !out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    int rc = dss_ensure_device();
    if (rc) return rc;
    DssDevBlocks mem;
    float *dx = nullptr, *dc = nullptr, *dout = nullptr;
    rc = mem.upload<float>(x, (size_t)n, &dx) | mem.upload<float>(comp, (size_t)n, &dc) | mem.alloc<float>((size_t)n, &dout);
    if (!rc) rc = dss_launch_exp10_selftest(dx, dc, dout, n, 0);
    if (!rc && hipMemcpy(out, dout, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = DSS_ENODEV;
    mem.free_all();
    return rc;
}

extern "C" int dss_selftest_lin2ulaw(unsigned start_bits, unsigned stride, long n, unsigned char *out)
{
    if (!out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    int rc = dss_ensure_device();
    if (rc) return rc;
    DssDevBlocks mem;
    unsigned char *dout = nullptr;
    rc = mem.alloc<unsigned char>((size_t)n, &dout);
    if (!rc) rc = dss_launch_lin2ulaw_selftest(start_bits, stride, n, dout, 0);
    if (!rc && hipMemcpy(out, dout, (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) rc = DSS_ENODEV;
    mem.free_all();
    return rc;
}
