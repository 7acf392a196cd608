// csrc/dss_fenc.cpp -- host side of Part 16 of include/dss_hip.h: the LPC feature encoder over a trial list.
//
// Owns the tables (window, twiddles and the derived tables of lpc_from_cepstrum, uploaded without any LPCNet model), the
// descriptor and tile tables of a call, the score scratch and the staging of the host-buffer form; the arithmetic runs in
// csrc/feature_encoder.hip only.  The checks are handle-free host functions, so they are testable without a device.
#include <math.h>

#include <vector>

#include "dss_host.h"
#include "feature_encoder.h"
#include "lpc_tables.h"

struct dss_fenc {
    int device = 0;
    DssFencDev d = {};
    DssDevBlocks blocks;
    // per call (one call per handle in flight)
    DssDevTable<DssFencTrial> desc;
    DssDevTable<DssFencTile> tiles;
    DssDevArray<double> d_scores;
    long long last_subframes = 0;
    hipStream_t last_stream = nullptr;
    // staging of the host-buffer form
    DssDevArray<short> d_audio;
    DssDevArray<float> d_out;
    // development timing: events around the three launches of a call
    bool timing = false, stamped = false;
    hipEvent_t stamps[4] = {nullptr, nullptr, nullptr, nullptr};
};

extern "C" long long dss_fenc_frame_offsets(const long long *offsets, int n_trials, long long *out)
{
    if (n_trials < 0 || !offsets) { dss_set_error("feature encoder: bad trial list"); return DSS_EINVAL; }
    if (offsets[0] < 0) { dss_set_error("feature encoder: the first offset is negative"); return DSS_EINVAL; }
    long long total = 0;
    if (out) out[0] = 0;
    for (int i = 0; i < n_trials; ++i) {
        if (offsets[i + 1] < offsets[i]) {
            dss_set_error("feature encoder: trial %d ends at sample %lld, before its start %lld", i, offsets[i + 1], offsets[i]);
            return DSS_EINVAL;
        }
        const long long frames = (offsets[i + 1] - offsets[i]) / FENC_FRAME;
        if (frames > 0x7fffffffLL / (2 * FENC_FRAME)) { dss_set_error("feature encoder: trial %d is too long", i); return DSS_EINVAL; }
        total += frames;
        if (out) out[i + 1] = total;
    }
    return total;
}

extern "C" void dss_fenc_destroy(dss_fenc *f)
{
    if (!f) return;
    for (hipEvent_t e : f->stamps)
        if (e) hipEventDestroy(e);
    dss_destroy_handle(f);
}

int dss_fenc_setup(DssDevBlocks &blocks, DssFencDev *d)
{
    std::vector<float> win(FENC_WINDOW);
    const std::vector<double> tw = dss_twiddles(FENC_WINDOW);
    for (int k = 0; k < FENC_FRAME; ++k) {
        const double s = sin(.5 * M_PI * (k + .5) / FENC_FRAME);
        win[k] = win[FENC_WINDOW - 1 - k] = (float)sin(.5 * M_PI * s * s);
    }
    const LpcTables T;
    float *p32 = nullptr;
    double *p64 = nullptr;
    int rc = blocks.upload(win.data(), win.size(), &p32);             d->window = p32;
    if (!rc) { rc = blocks.upload(tw.data(), tw.size(), &p64);         d->tw = p64; }
    if (!rc) { rc = blocks.upload(T.dct, (size_t)324, &p32);           d->lpc.dct_table = p32; }
    if (!rc) { rc = blocks.upload(T.cos_kl.data(), T.cos_kl.size(), &p32); d->lpc.cos_kl = p32; }
    if (!rc) { rc = blocks.upload(T.ia, (size_t)160, &p32);            d->lpc.interp_a = p32; }
    if (!rc) { rc = blocks.upload(T.ib, (size_t)160, &p32);            d->lpc.interp_b = p32; }
    if (!rc) { rc = blocks.upload(T.lagw, (size_t)17, &p64);           d->lpc.lag_window = p64; }
    d->idct_scale = sqrt(2. / DSS_NB_BANDS);
    return rc;
}

extern "C" dss_fenc *dss_fenc_create(void)
{
    if (dss_ensure_device()) return nullptr;
    dss_fenc *f = new dss_fenc;
    hipGetDevice(&f->device);
    if (dss_fenc_setup(f->blocks, &f->d)) { dss_fenc_destroy(f); return nullptr; }
    return f;
}

// The argument checks of both forms; the total number of frames, or DSS_EINVAL.
static long long fenc_check(const dss_fenc *f, long long n, const long long *offsets, int n_trials)
{
    if (!f) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    if (n < 0) { dss_set_error("feature encoder: %lld samples", n); return DSS_EINVAL; }
    if (n_trials == 0) return 0;
    const long long total = dss_fenc_frame_offsets(offsets, n_trials, nullptr);
    if (total < 0) return total;
    if (offsets[n_trials] > n) {
        dss_set_error("feature encoder: the trial list ends at sample %lld, behind the audio's %lld", offsets[n_trials], n);
        return DSS_EINVAL;
    }
    return total;
}

// d_audio holds samples base .. of the caller's array.
static int fenc_run(dss_fenc *f, const short *d_audio, long long base, const long long *offsets, int n_trials, long long total,
                    float *d_out36, hipStream_t st)
{
    f->desc.host.resize((size_t)n_trials);
    f->tiles.host.clear();
    long long out = 0;
    for (int i = 0; i < n_trials; ++i) {
        DssFencTrial &t = f->desc.host[i];
        t.first = offsets[i] - base; t.n = offsets[i + 1] - offsets[i]; t.out = out; t.frames = (int)(t.n / FENC_FRAME); t.pad = 0;
        out += t.frames;
        for (int f0 = 0; f0 < t.frames; f0 += FENC_TILE_FRAMES) f->tiles.host.push_back(DssFencTile{i, f0});
    }
    if (f->tiles.host.size() > 0x7fffffffULL / FENC_TILE_FRAMES) { dss_set_error("feature encoder: too many frames for one launch"); return DSS_EINVAL; }
    int rc = f->d_scores.grow_headroom(f->blocks, (size_t)total * 2 * FENC_LAGS);
    if (!rc) rc = f->desc.upload(f->blocks, st);
    if (!rc) rc = f->tiles.upload(f->blocks, st);
    if (!rc) rc = dss_launch_fenc(f->d, d_audio, f->desc.dev, n_trials, f->tiles.dev, (int)f->tiles.host.size(), d_out36, f->d_scores, st,
                                  f->timing ? f->stamps : nullptr);
    if (rc) return rc;
    f->stamped = f->timing;
    f->last_subframes = 2 * total;
    f->last_stream = st;
    return DSS_OK;
}

extern "C" long long dss_fenc_features_trials_dev(dss_fenc *f, const short *d_audio, long long n, const long long *offsets, int n_trials,
                                                  float *d_out36, void *hip_stream)
{
    const long long total = fenc_check(f, n, offsets, n_trials);
    if (total < 0) return total;
    f->last_subframes = 0;
    if (total == 0) return 0;
    if (!d_audio || !d_out36) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(f->device));
    const int rc = fenc_run(f, d_audio, 0, offsets, n_trials, total, d_out36, (hipStream_t)hip_stream);
    return rc ? rc : total;
}

extern "C" long long dss_fenc_features_trials(dss_fenc *f, const short *audio, long long n, const long long *offsets, int n_trials,
                                              float *out36)
{
    const long long total = fenc_check(f, n, offsets, n_trials);
    if (total < 0) return total;
    f->last_subframes = 0;
    if (total == 0) return 0;
    if (!audio || !out36) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(f->device));
    const long long lo = offsets[0], hi = offsets[n_trials];             // only the samples the trials span cross the bus
    int rc = f->d_audio.grow_headroom(f->blocks, (size_t)(hi - lo));
    if (!rc) rc = f->d_out.grow_headroom(f->blocks, (size_t)total * FENC_OUT);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(f->d_audio, audio + lo, sizeof(short) * (size_t)(hi - lo), hipMemcpyHostToDevice));
    rc = fenc_run(f, f->d_audio, lo, offsets, n_trials, total, f->d_out, nullptr);
    if (!rc) rc = dss_fetch(out36, f->d_out.p, (size_t)total * FENC_OUT);
    return rc ? rc : total;
}

extern "C" long long dss_fenc_tap_scores(dss_fenc *f, double *out, long long n)
{
    if (!f) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    const long long have = f->last_subframes * FENC_LAGS;
    if (n != have) { dss_set_error("feature encoder: the last call left %lld scores (sub-frames x 256), not %lld", have, n); return DSS_EINVAL; }
    if (have == 0) return 0;
    if (!out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(f->device));
    DSS_HIP_CHECK(hipStreamSynchronize(f->last_stream));
    DSS_HIP_CHECK(hipMemcpy(out, f->d_scores, sizeof(double) * (size_t)have, hipMemcpyDeviceToHost));
    return f->last_subframes;
}

extern "C" int dss_fenc_enable_timing(dss_fenc *f, int on)
{
    if (!f) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(f->device));
    for (hipEvent_t &e : f->stamps)
        if (on && !e) DSS_HIP_CHECK(hipEventCreate(&e));
    f->timing = on != 0;
    f->stamped = false;
    return DSS_OK;
}

extern "C" double dss_fenc_kernel_ms(dss_fenc *f, int which)
{
    if (!f || which < 0 || which > 2) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    if (!f->stamped) { dss_set_error("feature encoder: no timed call (dss_fenc_enable_timing, then a call with frames)"); return DSS_EINVAL; }
    float ms = 0.f;
    DSS_HIP_CHECK(hipEventSynchronize(f->stamps[3]));
    DSS_HIP_CHECK(hipEventElapsedTime(&ms, f->stamps[which], f->stamps[which + 1]));
    return (double)ms;
}
