// csrc/dss_host.h -- host-side helpers shared by the C ABI's translation units (one dss_*.cpp per operator).
#pragma once

#include <algorithm>
#include <vector>

#include "dss_common.h"

// What crosses from one host file to another without being part of the library's interface stays out of its symbol table.
#define DSS_LOCAL __attribute__((visibility("hidden")))

// Selects (and on first use picks: LOCAL_RANK, else 0) this thread's device; DSS_ENODEV without one.
int dss_ensure_device(void);

// The loaded LPCNet model (dss_lpcnet_model.cpp) and its copy on the calling thread's device.  With acquire set the caller owns
// one reference from then on (release_model()); a superseded model dies with its last user.
struct HostModel;
DSS_LOCAL int get_model(HostModel **out_hm, const DssModelDev **out, bool acquire);
DSS_LOCAL void release_model(HostModel *hm);

// Trial lists (Part 8; the tables of Parts 7, 11 and the HGA): list positions, longest trial first (ties in list order): the long
// trials start first, the short ones fill the tail.  Lengths are int or long long (Part 11).
template <typename L>
static std::vector<int> trials_longest_first(int n_trials, const L *len)
{
    std::vector<int> order((size_t)n_trials);
    for (int i = 0; i < n_trials; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return len[a] > len[b]; });
    return order;
}

// Where every trial's output starts, in list order, and behind them the list's total: trial i emits count(i) frames (or rows).
// The limits on these sums are the *_check_* functions', which run first.
template <typename F>
static std::vector<long long> trials_offsets(int n_trials, F count)
{
    std::vector<long long> off((size_t)n_trials + 1);
    for (int i = 0; i < n_trials; ++i) off[i + 1] = off[i] + count(i);
    return off;
}

// the chunks of a reduction over a trial list: DSS_TRIAL_CHUNK trials per launch, their lengths as kernel arguments
template <typename F>
static int trials_reduce(const char *what, int n_trials, const int *len, F launch)
{
    if (n_trials < 0 || (n_trials && !len)) { dss_set_error("%s: bad trial list", what); return DSS_EINVAL; }
    for (int i = 0; i < n_trials; ++i)
        if (len[i] < 1) { dss_set_error("%s: trial %d has %d frames (at least 1)", what, i, len[i]); return DSS_EINVAL; }
    if (dss_ensure_device()) return DSS_ENODEV;
    DssTrialLens tl;
    long long base = 0;
    for (int i0 = 0; i0 < n_trials; i0 += DSS_TRIAL_CHUNK) {
        tl.base = base; tl.first_trial = i0; tl.n = std::min(DSS_TRIAL_CHUNK, n_trials - i0);
        memset(tl.len, 0, sizeof(tl.len));
        for (int k = 0; k < tl.n; ++k) { tl.len[k] = len[i0 + k]; base += len[i0 + k]; }
        int rc = launch(tl);
        if (rc) return rc;
    }
    return DSS_OK;
}

// A row-major [4H][n] gate matrix (torch.nn.LSTM's layout) into the kernels' packed copy, as the copy's inputs k0 .. k0 + n: W_ih at
// 0, W_hh behind W_ih's input count padded to a multiple of 4.  The layout itself is lstm_packed_index (lstm_blocks.h), which the
// training kernels' update of the same copy uses.  `packed` starts out zeroed: the padded inputs keep zero weights.
DSS_LOCAL void dss_pack_rows(float *packed, int H4, int k0, const float *w, int n);

static inline size_t dss_headroom(size_t need) { return need + need / 4 + 64; }

// One owner for the device memory of a handle (and of the model, per device).  Every block allocated through it is remembered
// and freed by free_all(), with the owner's device selected; the device descriptors that kernels take by value keep raw pointers.
struct DSS_LOCAL DssDevBlocks {
    std::vector<void *> blocks;

    int alloc_bytes(size_t bytes, void **p);        // exactly `bytes`, as they come
    void release(const void *p);        // frees one block early and forgets it (NULL: nothing)
    void free_all();                    // copes with whatever a create path that failed halfway had allocated so far

    // count elements, zeroed, and 16 spare bytes behind them: several kernels read a full vector at the tail
    template <typename T>
    int alloc(size_t count, T **p)
    {
        void *d = nullptr;
        int rc = alloc_bytes(count * sizeof(T) + 16, &d);
        if (rc) return rc;
        DSS_HIP_CHECK(hipMemset(d, 0, count * sizeof(T)));
        *p = (T *)d;
        return DSS_OK;
    }
    // the same block filled from the host, with a blocking copy
    template <typename T>
    int upload(const T *host, size_t count, T **p)
    {
        void *d = nullptr;
        int rc = alloc_bytes(count * sizeof(T) + 16, &d);
        if (rc) return rc;
        DSS_HIP_CHECK(hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice));
        *p = (T *)d;
        return DSS_OK;
    }
};

// first and one-past-last row that a trial list covers: trial i spans first[i] .. first[i] + len[i] - lead[i] (lead may be NULL)
template <typename L>
static void trials_hull(int n_trials, const long long *first, const L *len, const int *lead, long long *lo, long long *hi)
{
    *lo = first[0]; *hi = first[0] + (len[0] - (lead ? lead[0] : 0));
    for (int i = 1; i < n_trials; ++i) {
        *lo = std::min(*lo, first[i]);
        *hi = std::max(*hi, first[i] + (long long)(len[i] - (lead ? lead[i] : 0)));
    }
}

// A device array that only grows: nothing when need <= cap, else the old block is freed through the owner (hipFree waits for the
// device, so the buffer of a call still queued is not freed under it) and exactly `need` elements are allocated, or with
// grow_headroom dss_headroom(need), so that a slightly longer list next time does not allocate again.  No spare bytes, not zeroed,
// contents not kept.  Reads as its pointer.
template <typename T>
struct DSS_LOCAL DssDevArray {
    T *p = nullptr;
    size_t cap = 0;

    operator T *() const { return p; }
    int grow(DssDevBlocks &blocks, size_t need) { return need <= cap ? DSS_OK : regrow(blocks, need); }
    int grow_headroom(DssDevBlocks &blocks, size_t need) { return need <= cap ? DSS_OK : regrow(blocks, dss_headroom(need)); }
    int regrow(DssDevBlocks &blocks, size_t count)
    {
        blocks.release(p);
        p = nullptr; cap = 0;
        const int rc = blocks.alloc_bytes(count * sizeof(T), (void **)&p);
        if (!rc) cap = count;
        return rc;
    }
};

// A table that a call fills on the host and its kernels read: upload() grows the device twin (upload_exact(): without headroom)
// and copies host.size() elements on st, nothing for an empty table.  The source is pageable and rewritten by the next call: one
// call per handle in flight.
template <typename T>
struct DSS_LOCAL DssDevTable {
    std::vector<T> host;
    DssDevArray<T> dev;

    int upload_exact(DssDevBlocks &blocks, hipStream_t st) { return upload(blocks, st, false); }
    int upload(DssDevBlocks &blocks, hipStream_t st, bool headroom = true)
    {
        const int rc = headroom ? dev.grow_headroom(blocks, host.size()) : dev.grow(blocks, host.size());
        if (rc || host.empty()) return rc;
        DSS_HIP_CHECK(hipMemcpyAsync(dev.p, host.data(), sizeof(T) * host.size(), hipMemcpyHostToDevice, st));
        return DSS_OK;
    }
};

// cos, sin of 2 pi j / n for j = 0 .. n - 1, interleaved: the DFT tables of Parts 7, 11, 12 and 16
DSS_LOCAL std::vector<double> dss_twiddles(int n);

// The end of a *_destroy whose handle owns nothing but its blocks: queued work ends before its memory goes.
template <typename H>
static void dss_destroy_handle(H *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    h->blocks.free_all();
    delete h;
}

// The tail of a host-buffer form: wait for the null stream, then count elements to the host.
template <typename T>
static int dss_fetch(T *out, const T *d, size_t count)
{
    DSS_HIP_CHECK(hipStreamSynchronize(nullptr));
    DSS_HIP_CHECK(hipMemcpy(out, d, sizeof(T) * count, hipMemcpyDeviceToHost));
    return DSS_OK;
}

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

// The same for a detector's trainer (Part 9), for the group of Part 15.
struct dss_vad_trainer;
int dss_vad_trainer_view(dss_vad_trainer *tr, DssVadTrainDev *d, int *device, int *loaded);

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

// The tables of a group of trainers stepped by one set of launches (Parts 13 and 15), over the two plain structs the group kernels
// read: a device table of the members' M descriptors, written once, and a ring of trial tables.  A step fills the next page-locked
// slot (acquire), copies it to the slot's device table in stream order (upload) and launches on that table, so a step enqueued
// while earlier ones still run never rewrites a table they read; a slot is reused only after the event behind its step's LAST
// launch (commit_after_launch: the device table is read until then, not only by the copy).  The ninth step in flight waits for
// the first.  The members' own memory is the members'.
template <typename Model, typename Trial>
struct DssGroupTables {
    int M = 0;
    Model *d_models = nullptr;                            // [M]
    Trial *d_trials[DssPinnedRing::K] = {};               // [K][M]
    DssDevBlocks blocks;
    DssPinnedRing ring;
    bool ring_ok = false;

    int init(const std::vector<Model> &table)
    {
        M = (int)table.size();
        const size_t tb = (size_t)M * sizeof(Trial);
        bool ok = blocks.alloc_bytes(table.size() * sizeof(Model), (void **)&d_models) == DSS_OK &&
                  hipMemcpy(d_models, table.data(), table.size() * sizeof(Model), hipMemcpyHostToDevice) == hipSuccess;
        for (int k = 0; ok && k < DssPinnedRing::K; ++k)
            ok = blocks.alloc_bytes(tb, (void **)&d_trials[k]) == DSS_OK && hipMemset(d_trials[k], 0, tb) == hipSuccess;
        ring_ok = true;
        if (ok) ok = ring.init((tb + sizeof(int) - 1) / sizeof(int)) == DSS_OK;
        return ok ? DSS_OK : DSS_ENOMEM;
    }
    void destroy()
    {
        blocks.free_all();
        if (ring_ok) ring.destroy();
    }
    // the host slot this step may fill (nullptr on a HIP error)
    Trial *acquire() { return (Trial *)ring.acquire(); }
    // the acquired slot to its device table; *d_slot is what the step's launches read
    int upload(hipStream_t s, const Trial **d_slot)
    {
        DSS_HIP_CHECK(hipMemcpyAsync(d_trials[ring.cur], ring.host[ring.cur], (size_t)M * sizeof(Trial), hipMemcpyHostToDevice, s));
        *d_slot = d_trials[ring.cur];
        return DSS_OK;
    }
    int commit_after_launch(hipStream_t s) { return ring.commit(s); }
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
