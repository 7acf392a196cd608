// csrc/dss_contam.cpp -- host side of Part 12 of include/dss_hip.h: the lagged audio-ECoG spectrogram correlation sums of the
// acoustic contamination analysis.
//
// Owns the tables (window, twiddles), the workspaces of a call (the audio spectrogram, the frame mask, the workgroups' partial
// sums) and the staging of the host-buffer form; the arithmetic runs in csrc/contamination.hip only.  Every check of a value is a
// handle-free host function (dss_contam_check_params, _check_window, _frames_for, _check_call, _result_size) that create and the
// two calls run before they touch a device, so each is testable without one; only the NULL checks of a call's own pointers need
// a handle to be told apart from a missing handle.  How a call's frames are cut into workgroups is decided in one place
// (contam_cut), which dss_contam_plan reports without a device.
#include <math.h>

#include <algorithm>
#include <vector>

#include "contamination.h"
#include "dss_host.h"

struct dss_contam {
    int device = 0;
    dss_contam_params p;
    DssContamDev v;
    DssDevBlocks blocks;
    double *d_win = nullptr, *d_tw = nullptr, *d_shift = nullptr;
    // per call (one call per handle in flight)
    DssDevTable<unsigned char> keep;
    DssDevArray<double> d_aud, d_partial;
    // staging of the host-buffer form
    DssDevArray<double> d_x, d_audio, d_out;
};

extern "C" int dss_contam_check_params(const dss_contam_params *p)
{
    if (!p) { dss_set_error("contamination: no parameters"); return DSS_EINVAL; }
    if (p->nperseg < 2) { dss_set_error("contamination: nperseg must be at least 2, not %d", p->nperseg); return DSS_EINVAL; }
    if (p->nperseg > 2048) { dss_set_error("contamination: nperseg up to 2048 supported, not %d", p->nperseg); return DSS_EINVAL; }
    if (p->hop < 1) { dss_set_error("contamination: the hop between frames must be at least 1, not %d", p->hop); return DSS_EINVAL; }
    if (p->n_bins < 1 || p->n_bins > CONTAM_MAX_BINS) {
        dss_set_error("contamination: the band keeps %d bins; 1 to %d supported", p->n_bins, CONTAM_MAX_BINS);
        return DSS_EINVAL;
    }
    if (p->bin_lo < 0 || p->bin_lo + p->n_bins > p->nperseg / 2 + 1) {
        dss_set_error("contamination: bins %d .. %d lie outside the %d bins of a %d-row window", p->bin_lo, p->bin_lo + p->n_bins - 1,
                      p->nperseg / 2 + 1, p->nperseg);
        return DSS_EINVAL;
    }
    if (p->max_lag < 0 || p->max_lag > 4096) { dss_set_error("contamination: a maximum lag of 0 to 4096 frames supported, not %d", p->max_lag); return DSS_EINVAL; }
    DssContamDev v;
    if (!dss_contam_shape(p->nperseg, p->hop, p->bin_lo, p->n_bins, p->max_lag, &v)) {
        dss_set_error("contamination: 32 frames of %d rows every %d rows do not fit the kernel's %d bytes of LDS", p->nperseg, p->hop,
                      SPEC_LDS_SOFT);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" long long dss_contam_frames_for(long long n_rows, int nperseg, int hop, int max_lag)
{
    if (nperseg < 2) { dss_set_error("contamination: nperseg must be at least 2, not %d", nperseg); return DSS_EINVAL; }
    if (hop < 1) { dss_set_error("contamination: the hop between frames must be at least 1, not %d", hop); return DSS_EINVAL; }
    if (max_lag < 0) { dss_set_error("contamination: a negative maximum lag (%d)", max_lag); return DSS_EINVAL; }
    if (n_rows < nperseg) { dss_set_error("a recording of %lld rows is shorter than one window (%d rows)", n_rows, nperseg); return DSS_EINVAL; }
    const long long W = (n_rows - nperseg) / hop + 1;
    if (W > 0x7fffffffLL - 2LL * max_lag - 64) {
        dss_set_error("contamination: %lld frames and lags up to %d exceed the 32-bit frame index", W, max_lag);
        return DSS_EINVAL;
    }
    return W;
}

extern "C" long long dss_contam_result_size(const dss_contam_params *p, int n_channels, long long offsets[7])
{
    if (dss_contam_check_params(p)) return DSS_EINVAL;
    if (n_channels < 1) { dss_set_error("contamination: %d channels", n_channels); return DSS_EINVAL; }
    if (n_channels > CONTAM_MAX_CHANNELS) {
        dss_set_error("contamination: %d channels are too many for one launch (up to %d)", n_channels, CONTAM_MAX_CHANNELS);
        return DSS_EINVAL;
    }
    DssContamDev v;
    dss_contam_shape(p->nperseg, p->hop, p->bin_lo, p->n_bins, p->max_lag, &v);
    long long off[8];
    dss_contam_layout(v, n_channels, off);
    if (offsets) std::copy(off, off + 7, offsets);
    return off[7];
}

extern "C" int dss_contam_check_window(const dss_contam_params *p, const double *window)
{
    if (dss_contam_check_params(p)) return DSS_EINVAL;
    if (!window) { dss_set_error("contamination: missing window"); return DSS_EINVAL; }
    double sq = 0.0;
    for (int k = 0; k < p->nperseg; ++k) {
        if (!isfinite(window[k])) { dss_set_error("contamination: the window holds a non-finite value"); return DSS_EINVAL; }
        sq += window[k] * window[k];
    }
    if (!(sq > 0.0)) { dss_set_error("contamination: the window is all zero"); return DSS_EINVAL; }
    return DSS_OK;
}

extern "C" long long dss_contam_check_call(const dss_contam_params *p, long long n_rows, int ld, int n_channels)
{
    if (dss_contam_check_params(p)) return DSS_EINVAL;
    if (n_channels < 1 || ld < n_channels) {
        dss_set_error("contamination: %d channels in rows of %d values", n_channels, ld);
        return DSS_EINVAL;
    }
    if (n_channels > CONTAM_MAX_CHANNELS) {
        dss_set_error("contamination: %d channels are too many for one launch (up to %d)", n_channels, CONTAM_MAX_CHANNELS);
        return DSS_EINVAL;
    }
    return dss_contam_frames_for(n_rows, p->nperseg, p->hop, p->max_lag);
}

// Chunks of whole tiles: about 512 workgroups in all, every chunk at least one tile, the last one perhaps shorter.
static void contam_cut(const DssContamDev &v, int W, int C, int *n_tiles, int *chunks, int *tiles_per_chunk)
{
    *n_tiles = (W + CONTAM_F - 1) / CONTAM_F;
    const long long per_chunk = (long long)C * v.Z;
    const int want = (int)std::max(1LL, std::min((long long)*n_tiles, (512 + per_chunk - 1) / per_chunk));
    *tiles_per_chunk = (*n_tiles + want - 1) / want;
    *chunks = (*n_tiles + *tiles_per_chunk - 1) / *tiles_per_chunk;
}

extern "C" int dss_contam_plan(const dss_contam_params *p, long long n_rows, int n_channels, int plan[6])
{
    const long long W = dss_contam_check_call(p, n_rows, n_channels, n_channels);
    if (W < 0) return DSS_EINVAL;
    if (!plan) { dss_set_error("contamination: nowhere to write the plan"); return DSS_EINVAL; }
    DssContamDev v;
    dss_contam_shape(p->nperseg, p->hop, p->bin_lo, p->n_bins, p->max_lag, &v);
    plan[0] = (int)W;
    contam_cut(v, (int)W, n_channels, &plan[1], &plan[2], &plan[3]);
    plan[4] = v.Z;
    plan[5] = v.lgn;
    return DSS_OK;
}

extern "C" void dss_contam_destroy(dss_contam *h) { dss_destroy_handle(h); }

static int contam_setup(dss_contam *h, const double *window)
{
    const dss_contam_params &p = h->p;
    dss_contam_shape(p.nperseg, p.hop, p.bin_lo, p.n_bins, p.max_lag, &h->v);
    std::vector<double> win((size_t)h->v.spec.K4, 0.0);
    std::copy(window, window + p.nperseg, win.begin());
    const std::vector<double> tw = dss_twiddles(p.nperseg);
    int rc = h->blocks.upload(win.data(), win.size(), &h->d_win);
    if (!rc) rc = h->blocks.upload(tw.data(), tw.size(), &h->d_tw);
    if (!rc) rc = h->blocks.alloc_bytes(CONTAM_PAD * sizeof(double), (void **)&h->d_shift);
    if (rc) return rc;
    h->v.spec.win = h->d_win; h->v.spec.tw = h->d_tw;
    return DSS_OK;
}

extern "C" dss_contam *dss_contam_create(const dss_contam_params *p, const double *window)
{
    if (dss_contam_check_window(p, window)) return nullptr;
    if (dss_ensure_device()) return nullptr;
    dss_contam *h = new dss_contam;
    h->p = *p;
    hipGetDevice(&h->device);
    if (contam_setup(h, window)) { dss_contam_destroy(h); return nullptr; }
    return h;
}

// The checks of both forms; the number of frames.
static long long contam_check_call(const dss_contam *h, long long n_rows, int ld, int C)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    return dss_contam_check_call(&h->p, n_rows, ld, C);
}

// The launches on device-resident signals.  keep_frames: W host bytes, or NULL for every frame.
static int contam_run(dss_contam *h, const double *d_x, int ld, int C, const double *d_audio, long long T, int W,
                      const unsigned char *keep_frames, double *d_out, hipStream_t st)
{
    const DssContamDev &v = h->v;
    h->keep.host.assign((size_t)W, 1);
    if (keep_frames)
        for (int t = 0; t < W; ++t) h->keep.host[t] = keep_frames[t] ? 1 : 0;
    int n_tiles, chunks, tiles_per_chunk;
    contam_cut(v, W, C, &n_tiles, &chunks, &tiles_per_chunk);
    int rc = h->d_aud.grow_headroom(h->blocks, (size_t)W * CONTAM_PAD);
    if (!rc) rc = h->d_partial.grow_headroom(h->blocks, (size_t)chunks * v.nlag * C * contam_record(v.B));
    if (!rc) rc = h->keep.upload(h->blocks, st);
    if (rc) return rc;
    return dss_launch_contam(v, d_x, ld, C, d_audio, T, W, h->keep.dev, h->d_aud, h->d_shift, h->d_partial, chunks, tiles_per_chunk, d_out, st);
}

extern "C" int dss_contam_moments_dev(dss_contam *h, const double *d_brain, long long n_rows, int ld, int C, const double *d_audio,
                                      const unsigned char *keep_frames, double *d_out, void *hip_stream)
{
    const long long W = contam_check_call(h, n_rows, ld, C);
    if (W < 0) return DSS_EINVAL;
    if (!d_brain || !d_audio || !d_out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return contam_run(h, d_brain, ld, C, d_audio, n_rows, (int)W, keep_frames, d_out, (hipStream_t)hip_stream);
}

extern "C" int dss_contam_moments(dss_contam *h, const double *brain, long long n_rows, int ld, int C, const double *audio,
                                  const unsigned char *keep_frames, double *out)
{
    const long long W = contam_check_call(h, n_rows, ld, C);
    if (W < 0) return DSS_EINVAL;
    if (!brain || !audio || !out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    long long off[8];
    dss_contam_layout(h->v, C, off);
    int rc = h->d_x.grow_headroom(h->blocks, (size_t)n_rows * ld + 1);
    if (!rc) rc = h->d_audio.grow_headroom(h->blocks, (size_t)n_rows);
    if (!rc) rc = h->d_out.grow_headroom(h->blocks, (size_t)off[7]);
    if (rc) return rc;
    // the last row ends behind its C channels: the caller's array may be a view that ends there
    DSS_HIP_CHECK(hipMemcpy(h->d_x, brain, sizeof(double) * ((size_t)(n_rows - 1) * ld + C), hipMemcpyHostToDevice));
    DSS_HIP_CHECK(hipMemcpy(h->d_audio, audio, sizeof(double) * (size_t)n_rows, hipMemcpyHostToDevice));
    rc = contam_run(h, h->d_x, ld, C, h->d_audio, n_rows, (int)W, keep_frames, h->d_out, nullptr);
    return rc ? rc : dss_fetch(out, h->d_out.p, (size_t)off[7]);
}
