// csrc/dss_fenc_stream.cpp -- host side of Part 18 of include/dss_hip.h: the LPC feature encoder on streams.
//
// Owns the tables (dss_fenc_setup, the ones of Part 16), one DssFencStreamState per stream on the device, the counts of a push
// (a page-locked stage, so that the caller's array is free when the call returns) and the staging of the host-buffer form; the
// arithmetic runs in csrc/feature_encoder_stream.hip only.  The check is a handle-free host function, testable without a device.
#include <vector>

#include "dss_host.h"
#include "feature_encoder.h"

struct dss_fenc_streams {
    int device = 0, S = 0;
    DssFencDev d = {};
    DssDevBlocks blocks;
    DssFencStreamState *d_states = nullptr;           // [S]
    std::vector<long long> seen;                      // frames per stream since its reset (the device keeps its own count)
    DssPinnedStage counts_stage;
    DssDevArray<int> d_counts;
    // staging of the host-buffer form
    DssDevArray<short> d_audio;
    DssDevArray<float> d_out;
};

extern "C" long long dss_fenc_streams_check(int n_streams, int frames_max, const int *counts)
{
    if (n_streams < 1) { dss_set_error("feature encoder streams: %d streams (at least 1)", n_streams); return DSS_EINVAL; }
    if (frames_max < 0) { dss_set_error("feature encoder streams: frames_max is %d", frames_max); return DSS_EINVAL; }
    if (frames_max > 0x7fffffff / (2 * FENC_FRAME)) { dss_set_error("feature encoder streams: %d frames are too many for one push", frames_max); return DSS_EINVAL; }
    if (!counts) return (long long)n_streams * frames_max;
    long long total = 0;
    for (int s = 0; s < n_streams; ++s) {
        if (counts[s] < 0 || counts[s] > frames_max) {
            dss_set_error("feature encoder streams: stream %d is to take %d frames, outside 0 .. frames_max = %d", s, counts[s], frames_max);
            return DSS_EINVAL;
        }
        total += counts[s];
    }
    return total;
}

extern "C" void dss_fenc_streams_destroy(dss_fenc_streams *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    h->counts_stage.destroy();
    h->blocks.free_all();
    delete h;
}

extern "C" dss_fenc_streams *dss_fenc_streams_create(int n_streams)
{
    if (dss_fenc_streams_check(n_streams, 0, nullptr) < 0) return nullptr;
    if (dss_ensure_device()) return nullptr;
    dss_fenc_streams *h = new dss_fenc_streams;
    hipGetDevice(&h->device);
    h->S = n_streams;
    h->seen.assign((size_t)n_streams, 0);
    if (dss_fenc_setup(h->blocks, &h->d) || h->blocks.alloc((size_t)n_streams, &h->d_states)) { dss_fenc_streams_destroy(h); return nullptr; }
    return h;
}

extern "C" int dss_fenc_streams_reset(dss_fenc_streams *h, const int *streams, int n, void *hip_stream)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    hipStream_t st = (hipStream_t)hip_stream;
    if (!streams) {
        DSS_HIP_CHECK(hipSetDevice(h->device));
        DSS_HIP_CHECK(hipMemsetAsync(h->d_states, 0, sizeof(DssFencStreamState) * (size_t)h->S, st));
        h->seen.assign((size_t)h->S, 0);
        return DSS_OK;
    }
    if (n < 0) { dss_set_error("feature encoder streams: a list of %d streams", n); return DSS_EINVAL; }
    for (int k = 0; k < n; ++k)
        if (streams[k] < 0 || streams[k] >= h->S) {
            dss_set_error("feature encoder streams: stream %d in a reset, outside 0 .. %d", streams[k], h->S - 1);
            return DSS_EINVAL;
        }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    for (int k = 0; k < n; ++k) {
        DSS_HIP_CHECK(hipMemsetAsync(h->d_states + streams[k], 0, sizeof(DssFencStreamState), st));
        h->seen[(size_t)streams[k]] = 0;
    }
    return DSS_OK;
}

// The argument checks of both forms; the number of frames the push encodes, or DSS_EINVAL.
static long long streams_check(const dss_fenc_streams *h, int frames_max, const int *counts)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    return dss_fenc_streams_check(h->S, frames_max, counts);
}

static int streams_run(dss_fenc_streams *h, const short *d_audio, int frames_max, const int *counts, float *d_out36, hipStream_t st)
{
    const int *d_counts = nullptr;
    if (counts) {
        const size_t bytes = sizeof(int) * (size_t)h->S;
        int *stage = (int *)h->counts_stage.acquire(bytes);
        if (!stage) { dss_set_error("feature encoder streams: no page-locked memory for the counts"); return DSS_ENOMEM; }
        memcpy(stage, counts, bytes);
        int rc = h->d_counts.grow(h->blocks, (size_t)h->S);
        if (rc) return rc;
        DSS_HIP_CHECK(hipMemcpyAsync(h->d_counts.p, stage, bytes, hipMemcpyHostToDevice, st));
        rc = h->counts_stage.commit(st);
        if (rc) return rc;
        d_counts = h->d_counts;
    }
    const int rc = dss_launch_fenc_streams(h->d, d_audio, h->S, frames_max, d_counts, h->d_states, d_out36, st);
    if (rc) return rc;
    for (int s = 0; s < h->S; ++s) h->seen[(size_t)s] += counts ? counts[s] : frames_max;
    return DSS_OK;
}

extern "C" long long dss_fenc_streams_push_dev(dss_fenc_streams *h, const short *d_audio, int frames_max, const int *counts,
                                               float *d_out36, void *hip_stream)
{
    const long long total = streams_check(h, frames_max, counts);
    if (total <= 0) return total;
    if (!d_audio || !d_out36) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    const int rc = streams_run(h, d_audio, frames_max, counts, d_out36, (hipStream_t)hip_stream);
    return rc ? rc : total;
}

extern "C" long long dss_fenc_streams_push(dss_fenc_streams *h, const short *audio, int frames_max, const int *counts, float *out36)
{
    const long long total = streams_check(h, frames_max, counts);
    if (total <= 0) return total;
    if (!audio || !out36) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    const size_t frames = (size_t)h->S * (size_t)frames_max;
    int rc = h->d_audio.grow_headroom(h->blocks, frames * FENC_FRAME);
    if (!rc) rc = h->d_out.grow_headroom(h->blocks, frames * FENC_OUT);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(h->d_audio, audio, sizeof(short) * frames * FENC_FRAME, hipMemcpyHostToDevice));
    rc = streams_run(h, h->d_audio, frames_max, counts, h->d_out, nullptr);
    if (!rc) rc = dss_fetch(out36, h->d_out.p, frames * FENC_OUT);
    return rc ? rc : total;
}

extern "C" int dss_fenc_streams_frames_seen(dss_fenc_streams *h, long long *out)
{
    if (!h || !out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    for (int s = 0; s < h->S; ++s) out[s] = h->seen[(size_t)s];
    return DSS_OK;
}
