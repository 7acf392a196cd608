// csrc/dss_host.h -- host-side helpers shared by the C ABI's translation units (dss_capi.cpp, dss_async.cpp).
#pragma once

#include "dss_common.h"

// Selects (and on first use picks: LOCAL_RANK, else 0) this thread's device; DSS_ENODEV without one.
int dss_ensure_device(void);

// The device view of `bytes` at p, which must lie inside one block from dss_host_alloc_fine and be `align`-byte aligned;
// DSS_EINVAL with a message otherwise (pageable or cached page-locked memory, a short block, misalignment).
int dss_fine_host_view(void *p, size_t bytes, size_t align, const char *what, void **dev);

// The device arrays of an inference detector (Part 5), for dss_vad_trainer_publish: the handle's device, its sizes and
// the six weight arrays wT0, b0, wT1, b1, wc, bc, writable.  DSS_EINVAL with a message for NULL or a handle without weights.
struct dss_vad;
int dss_vad_device_weights(dss_vad *v, int *device, int *n_inputs, int *hidden_units, float *w[6]);

// The same for an inference decoder (Part 6), for dss_dec_trainer_publish: the ten arrays wT[layer][direction] (four), b[layer][direction]
// (four), wr, br.
struct dss_dec;
int dss_dec_device_weights(dss_dec *v, int *device, int *n_inputs, int *hidden_units, int *n_outputs, float *w[10]);

// The device descriptor of a decoder's trainer (Part 10), the device it lives on and whether parameters are loaded, for the
// group of Part 13, which steps several trainers with one set of launches.
struct dss_dec_trainer;
int dss_dec_trainer_view(dss_dec_trainer *tr, DssDecTrainDev *d, int *device, int *loaded);

// Small host -> device uploads that must not stall, and must not be overwritten, while earlier calls are still queued.
//
// hipMemcpyAsync from pageable memory may wait for the stream's earlier work (the runtime stages it), which would hold the
// host for the length of a queued vocoder launch; from pinned memory it is asynchronous, but then the pinned words must
// stay untouched until the copy has run.  A ring of K pinned slots, each guarded by an event recorded behind the copies
// issued from it: acquire() hands out the next slot and waits only if the call K calls ago has not reached its copies yet.
struct DssPinnedRing {
    static const int K = 8;
    int *host[K] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev[K] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    bool pending[K] = {false, false, false, false, false, false, false, false};
    size_t ints = 0;
    int next = 0, cur = -1;

    int init(size_t n_ints)
    {
        ints = n_ints;
        for (int k = 0; k < K; ++k) {
            if (hipHostMalloc((void **)&host[k], n_ints * sizeof(int), hipHostMallocDefault) != hipSuccess) return DSS_ENOMEM;
            if (hipEventCreateWithFlags(&ev[k], hipEventDisableTiming) != hipSuccess) return DSS_ENOMEM;
        }
        return DSS_OK;
    }
    void destroy()
    {
        for (int k = 0; k < K; ++k) {
            if (pending[k] && ev[k]) hipEventSynchronize(ev[k]);
            if (host[k]) hipHostFree(host[k]);
            if (ev[k]) hipEventDestroy(ev[k]);
            host[k] = nullptr; ev[k] = nullptr; pending[k] = false;
        }
    }
    // the slot this call may fill (nullptr on a HIP error)
    int *acquire()
    {
        cur = next;
        next = (next + 1) % K;
        if (pending[cur]) {
            if (hipEventSynchronize(ev[cur]) != hipSuccess) return nullptr;
            pending[cur] = false;
        }
        return host[cur];
    }
    // call after the copies out of the acquired slot have been issued on s
    int commit(hipStream_t s)
    {
        if (cur < 0) return DSS_EINVAL;
        DSS_HIP_CHECK(hipEventRecord(ev[cur], s));
        pending[cur] = true;
        return DSS_OK;
    }
};

// One grow-only page-locked block for a call's variable-size table (the trial lists of Part 8): acquire(bytes) waits until the
// copies of the call before it have run (its event), so the block is never rewritten under a queued copy, and hipMemcpyAsync out
// of it is asynchronous (pageable memory would be staged by the runtime, and may hold the host behind the stream's earlier work).
struct DssPinnedStage {
    void *host = nullptr;
    size_t cap = 0;
    hipEvent_t ev = nullptr;
    bool pending = false;

    void *acquire(size_t bytes)
    {
        if (pending) {
            if (hipEventSynchronize(ev) != hipSuccess) return nullptr;
            pending = false;
        }
        if (bytes > cap) {
            if (host) { hipHostFree(host); host = nullptr; cap = 0; }
            if (hipHostMalloc(&host, bytes, hipHostMallocDefault) != hipSuccess) { host = nullptr; return nullptr; }
            cap = bytes;
        }
        if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; return nullptr; }
        return host;
    }
    // call after the copies out of the block have been issued on s
    int commit(hipStream_t s)
    {
        DSS_HIP_CHECK(hipEventRecord(ev, s));
        pending = true;
        return DSS_OK;
    }
    void destroy()
    {
        if (pending && ev) hipEventSynchronize(ev);
        if (host) hipHostFree(host);
        if (ev) hipEventDestroy(ev);
        host = nullptr; ev = nullptr; cap = 0; pending = false;
    }
};
