// csrc/dss_spec.cpp -- host side of Part 11 of include/dss_hip.h: spectrograms over a trial list, the onset-locked mean and the
// mean spectrum.
//
// Owns the tables (window, twiddles, scaling), the descriptor and tile tables of a call and the staging of the host-buffer forms;
// the arithmetic runs in csrc/spectral.hip only.  Every check is a handle-free host function, so it is testable without a device.
#include <math.h>

#include <algorithm>
#include <vector>

#include "dss_host.h"
#include "spectral.h"

struct dss_spec {
    int device = 0;
    dss_spec_params p;
    DssSpecDev d;
    DssDevBlocks blocks;
    double *d_win = nullptr, *d_tw = nullptr;
    // per call (one call per handle in flight)
    DssDevTable<DssSpecTrial> desc;
    DssDevTable<DssSpecTile> tiles;
    DssDevArray<double> d_partial;                               // per-trial sums of the mean spectrum
    // staging of the host-buffer forms
    DssDevArray<double> d_x, d_out;
};

static int spec_frame_shape(int nperseg, int hop)
{
    if (nperseg < 2) { dss_set_error("spectrogram: nperseg must be at least 2, not %d", nperseg); return DSS_EINVAL; }
    if (hop < 1) { dss_set_error("spectrogram: the hop between frames must be at least 1 (noverlap < nperseg), not %d", hop); return DSS_EINVAL; }
    return DSS_OK;
}

extern "C" int dss_spec_check_params(const dss_spec_params *p)
{
    if (!p) { dss_set_error("spectrogram: no parameters"); return DSS_EINVAL; }
    if (spec_frame_shape(p->nperseg, p->hop)) return DSS_EINVAL;
    if (p->nfft < p->nperseg) { dss_set_error("spectrogram: nfft (%d) is smaller than nperseg (%d)", p->nfft, p->nperseg); return DSS_EINVAL; }
    if (p->nfft > 2048) { dss_set_error("spectrogram: nfft up to 2048 supported, not %d", p->nfft); return DSS_EINVAL; }
    if (p->mode != DSS_SPEC_PSD && p->mode != DSS_SPEC_MAGNITUDE) { dss_set_error("spectrogram: unknown mode %d", p->mode); return DSS_EINVAL; }
    if (p->detrend != 0 && p->detrend != 1) { dss_set_error("spectrogram: detrend must be 0 (none) or 1 (constant), not %d", p->detrend); return DSS_EINVAL; }
    if (!(p->fs > 0.0) || !isfinite(p->fs)) { dss_set_error("spectrogram: the sampling rate must be positive and finite"); return DSS_EINVAL; }
    return DSS_OK;
}

extern "C" long long dss_spec_trial_frames_for(long long n, int nperseg, int hop)
{
    if (spec_frame_shape(nperseg, hop)) return DSS_EINVAL;
    if (n < nperseg) { dss_set_error("a trial of %lld rows is shorter than one window (%d rows)", n, nperseg); return DSS_EINVAL; }
    return (n - nperseg) / hop + 1;
}

extern "C" long long dss_spec_check_trials(long long n_rows, int n_trials, const long long *first, const long long *length, int nperseg,
                                           int hop)
{
    if (spec_frame_shape(nperseg, hop)) return DSS_EINVAL;
    if (n_trials < 0 || n_rows < 0) { dss_set_error("bad trial list: negative count"); return DSS_EINVAL; }
    if (n_trials && (!first || !length)) { dss_set_error("bad trial list: missing array"); return DSS_EINVAL; }
    long long total = 0;
    for (int i = 0; i < n_trials; ++i) {
        if (first[i] < 0 || length[i] < 0) { dss_set_error("trial %d: negative first row or length", i); return DSS_EINVAL; }
        if (first[i] > n_rows || length[i] > n_rows - first[i]) {
            dss_set_error("trial %d (rows %lld .. %lld) lies outside the signals of %lld rows", i, first[i], first[i] + length[i], n_rows);
            return DSS_EINVAL;
        }
        if (length[i] < nperseg) { dss_set_error("trial %d: %lld rows are shorter than one window (%d rows)", i, length[i], nperseg); return DSS_EINVAL; }
        const long long W = (length[i] - nperseg) / hop + 1;
        if (W > 0x7fffffffLL) { dss_set_error("trial %d emits more than 2^31 - 1 frames", i); return DSS_EINVAL; }
        total += W;
    }
    return total;
}

extern "C" int dss_spec_check_locked(int n_trials, const long long *length, const int *onset, int pre, int post, int nperseg, int hop)
{
    if (spec_frame_shape(nperseg, hop)) return DSS_EINVAL;
    if (n_trials < 1) { dss_set_error("onset-locked mean: no trials"); return DSS_EINVAL; }
    if (!length || !onset) { dss_set_error("bad trial list: missing array"); return DSS_EINVAL; }
    if (pre < 0 || post < 0 || (long long)pre + post < 1 || (long long)pre + post > 0x7fffffffLL) {
        dss_set_error("onset-locked mean: %d frames before and %d after the onset", pre, post);
        return DSS_EINVAL;
    }
    for (int i = 0; i < n_trials; ++i) {
        if (length[i] < nperseg) { dss_set_error("trial %d: %lld rows are shorter than one window (%d rows)", i, length[i], nperseg); return DSS_EINVAL; }
        const long long W = (length[i] - nperseg) / hop + 1;
        if (onset[i] < 0 || (long long)onset[i] - pre < 0) {
            dss_set_error("trial %d: onset frame %d has fewer than %d frames before it", i, onset[i], pre);
            return DSS_EINVAL;
        }
        if ((long long)onset[i] + post > W) {
            dss_set_error("trial %d: onset frame %d plus %d frames runs past the trial's %lld frames", i, onset[i], post, W);
            return DSS_EINVAL;
        }
    }
    return pre + post;
}

extern "C" void dss_spec_destroy(dss_spec *h) { dss_destroy_handle(h); }

// The part of the device view that the parameters alone decide: what dss_spec_pick_geom reads.
static void spec_shape(const dss_spec_params &p, DssSpecDev *d)
{
    d->nperseg = p.nperseg; d->hop = p.hop; d->nfft = p.nfft; d->bins = p.nfft / 2 + 1; d->nblk = (d->bins + 15) / 16;
    d->K4 = (p.nperseg + 3) & ~3; d->sh = std::min(p.hop, d->K4);
    d->mode = p.mode; d->detrend = p.detrend; d->odd = p.nfft & 1;
}

extern "C" int dss_spec_geometry(const dss_spec_params *p, int n_channels, int kind, int out[5])
{
    if (dss_spec_check_params(p)) return DSS_EINVAL;
    if (n_channels < 1) { dss_set_error("spectrogram: %d channels", n_channels); return DSS_EINVAL; }
    if (kind != SPEC_KIND_TRIALS && kind != SPEC_KIND_LOCKED && kind != SPEC_KIND_MEAN) {
        dss_set_error("spectrogram: unknown kernel kind %d (0 trials, 1 onset-locked mean, 2 mean spectrum)", kind);
        return DSS_EINVAL;
    }
    if (!out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DssSpecDev d = {};
    spec_shape(*p, &d);
    DssSpecGeom g;
    if (!dss_spec_pick_geom(d, n_channels, kind, &g)) { dss_set_error("spectrogram: the frame shape does not fit the kernel"); return DSS_EINVAL; }
    out[0] = g.F; out[1] = g.CG; out[2] = g.NB; out[3] = d.nblk; out[4] = (int)g.lds_bytes;
    return DSS_OK;
}

static int spec_setup(dss_spec *h, const double *window)
{
    const dss_spec_params &p = h->p;
    const int K4 = (p.nperseg + 3) & ~3;
    std::vector<double> win((size_t)K4, 0.0);
    double sq = 0.0;
    for (int k = 0; k < p.nperseg; ++k) {
        if (!isfinite(window[k])) { dss_set_error("spectrogram: the window holds a non-finite value"); return DSS_EINVAL; }
        win[k] = window[k];
        sq += window[k] * window[k];
    }
    if (!(sq > 0.0)) { dss_set_error("spectrogram: the window is all zero"); return DSS_EINVAL; }
    const std::vector<double> tw = dss_twiddles(p.nfft);
    int rc = h->blocks.upload(win.data(), win.size(), &h->d_win);
    if (!rc) rc = h->blocks.upload(tw.data(), tw.size(), &h->d_tw);
    if (rc) return rc;
    DssSpecDev &d = h->d;
    spec_shape(p, &d);
    const double scale = 1.0 / (p.fs * sq);          // scipy: scale = 1.0 / (fs * (win * win).sum())
    d.scale = p.mode == DSS_SPEC_MAGNITUDE ? sqrt(scale) : scale;
    d.win = h->d_win; d.tw = h->d_tw;
    return DSS_OK;
}

extern "C" dss_spec *dss_spec_create(const dss_spec_params *p, const double *window)
{
    if (dss_spec_check_params(p)) return nullptr;
    if (!window) { dss_set_error("spectrogram: missing window"); return nullptr; }
    if (dss_ensure_device()) return nullptr;
    dss_spec *h = new dss_spec;
    h->p = *p;
    hipGetDevice(&h->device);
    if (spec_setup(h, window)) { dss_spec_destroy(h); return nullptr; }
    return h;
}

static int spec_check_layout(const dss_spec *h, int ld, int C)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    if (C < 1 || ld < C) { dss_set_error("spectrogram: %d channels in rows of %d values", C, ld); return DSS_EINVAL; }
    return DSS_OK;
}

// The three operations on device-resident signals; d_x holds rows row_base .. of the caller's array.
static long long spec_run_trials(dss_spec *h, const double *d_x, long long row_base, int ld, int C, int n_trials, const long long *first,
                                 const long long *length, double *d_out, hipStream_t st)
{
    const int N = h->p.nperseg, hop = h->p.hop;
    DssSpecGeom g;
    if (!dss_spec_pick_geom(h->d, C, SPEC_KIND_TRIALS, &g)) { dss_set_error("spectrogram: the frame shape does not fit the kernel"); return DSS_EINVAL; }
    // descriptor table, longest trial first: the long trials' tiles start first and the short ones fill the tail
    const std::vector<int> order = trials_longest_first(n_trials, length);
    const std::vector<long long> out_frame = trials_offsets(n_trials, [&](int i) { return (length[i] - N) / hop + 1; });
    std::vector<DssSpecTile> &tiles = h->tiles.host;
    h->desc.host.resize((size_t)n_trials);
    tiles.clear();
    for (int k = 0; k < n_trials; ++k) {
        const int i = order[k];
        DssSpecTrial &t = h->desc.host[k];
        t.first = first[i] - row_base; t.n = length[i]; t.out = out_frame[i]; t.W = (int)((length[i] - N) / hop + 1); t.frame0 = 0;
        for (long long f0 = 0; f0 < t.W; f0 += g.F) tiles.push_back(DssSpecTile{k, (int)f0});
    }
    if (tiles.size() > 0x7fffffffULL) { dss_set_error("spectrogram: too many tiles for one launch"); return DSS_EINVAL; }
    int rc = h->desc.upload(h->blocks, st);
    if (!rc) rc = h->tiles.upload(h->blocks, st);
    if (!rc) rc = dss_launch_spec_trials(h->d, g, d_x, ld, C, h->desc.dev, h->tiles.dev, (int)tiles.size(), d_out, st);
    return rc ? rc : out_frame[n_trials];
}

static int spec_run_locked(dss_spec *h, const double *d_x, long long row_base, int ld, int C, int n_trials, const long long *first,
                           const long long *length, const int *onset, int pre, int post, double *d_out, hipStream_t st)
{
    DssSpecGeom g;
    if (!dss_spec_pick_geom(h->d, C, SPEC_KIND_LOCKED, &g)) { dss_set_error("spectrogram: the frame shape does not fit the kernel"); return DSS_EINVAL; }
    h->desc.host.resize((size_t)n_trials);
    for (int i = 0; i < n_trials; ++i) {
        DssSpecTrial &t = h->desc.host[i];
        t.first = first[i] - row_base; t.n = length[i]; t.out = i; t.W = (int)((length[i] - h->p.nperseg) / h->p.hop + 1);
        t.frame0 = onset[i] - pre;
    }
    int rc = h->desc.upload(h->blocks, st);
    if (!rc) rc = dss_launch_spec_locked(h->d, g, d_x, ld, C, h->desc.dev, n_trials, pre + post, d_out, st);
    return rc ? rc : pre + post;
}

static int spec_run_mean(dss_spec *h, const double *d_x, long long row_base, int ld, int C, int n_trials, const long long *first,
                         const long long *length, long long total, double *d_out, hipStream_t st)
{
    DssSpecGeom g;
    if (!dss_spec_pick_geom(h->d, C, SPEC_KIND_MEAN, &g)) { dss_set_error("spectrogram: the frame shape does not fit the kernel"); return DSS_EINVAL; }
    // the grid takes the longest trial first; every trial's sum lands at its place in the caller's list
    const std::vector<int> order = trials_longest_first(n_trials, length);
    h->desc.host.resize((size_t)n_trials);
    for (int k = 0; k < n_trials; ++k) {
        const int i = order[k];
        DssSpecTrial &t = h->desc.host[k];
        t.first = first[i] - row_base; t.n = length[i]; t.out = i; t.W = (int)((length[i] - h->p.nperseg) / h->p.hop + 1); t.frame0 = 0;
    }
    int rc = h->desc.upload(h->blocks, st);
    if (!rc) rc = h->d_partial.grow_headroom(h->blocks, (size_t)n_trials * C * h->d.bins);
    if (!rc) rc = dss_launch_spec_mean(h->d, g, d_x, ld, C, h->desc.dev, n_trials, total, h->d_partial, d_out, st);
    return rc;
}

// Host-buffer forms: only the rows the trials span cross the bus, once, however the trials overlap; run(row_base) is the
// operation on the staged rows, into h->d_out, and its result the form's.
template <typename Run>
static long long spec_host_form(dss_spec *h, const double *x, int ld, int C, int n_trials, const long long *first, const long long *length,
                                double *out, size_t count, Run run)
{
    long long lo, hi;
    trials_hull(n_trials, first, length, nullptr, &lo, &hi);
    int rc = h->d_x.grow_headroom(h->blocks, (size_t)(hi - lo) * ld + 1);
    if (rc) return rc;
    // the last row ends behind its C channels: the caller's array may be a view that ends there
    if (hi > lo) DSS_HIP_CHECK(hipMemcpy(h->d_x, x + lo * ld, sizeof(double) * ((size_t)(hi - lo - 1) * ld + C), hipMemcpyHostToDevice));
    rc = h->d_out.grow_headroom(h->blocks, count);
    if (rc) return rc;
    const long long got = run(lo);
    if (got < 0) return got;
    rc = dss_fetch(out, h->d_out.p, count);
    return rc ? rc : got;
}

extern "C" long long dss_spec_trials_dev(dss_spec *h, const double *d_x, long long n_rows, int ld, int C, int n_trials,
                                         const long long *first, const long long *length, double *d_out, void *hip_stream)
{
    if (spec_check_layout(h, ld, C)) return DSS_EINVAL;
    const long long total = dss_spec_check_trials(n_rows, n_trials, first, length, h->p.nperseg, h->p.hop);
    if (total <= 0) return total;
    if (!d_x || !d_out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return spec_run_trials(h, d_x, 0, ld, C, n_trials, first, length, d_out, (hipStream_t)hip_stream);
}

extern "C" long long dss_spec_trials(dss_spec *h, const double *x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                                     const long long *length, double *out)
{
    if (spec_check_layout(h, ld, C)) return DSS_EINVAL;
    const long long total = dss_spec_check_trials(n_rows, n_trials, first, length, h->p.nperseg, h->p.hop);
    if (total <= 0) return total;
    if (!x || !out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return spec_host_form(h, x, ld, C, n_trials, first, length, out, (size_t)total * C * h->d.bins, [&](long long base) {
        return spec_run_trials(h, h->d_x, base, ld, C, n_trials, first, length, h->d_out, nullptr);
    });
}

extern "C" int dss_spec_locked_dev(dss_spec *h, const double *d_x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                                   const long long *length, const int *onset, int pre, int post, double *d_out, void *hip_stream)
{
    if (spec_check_layout(h, ld, C)) return DSS_EINVAL;
    if (dss_spec_check_trials(n_rows, n_trials, first, length, h->p.nperseg, h->p.hop) < 0) return DSS_EINVAL;
    const int J = dss_spec_check_locked(n_trials, length, onset, pre, post, h->p.nperseg, h->p.hop);
    if (J < 0) return J;
    if (!d_x || !d_out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return spec_run_locked(h, d_x, 0, ld, C, n_trials, first, length, onset, pre, post, d_out, (hipStream_t)hip_stream);
}

extern "C" int dss_spec_locked(dss_spec *h, const double *x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                               const long long *length, const int *onset, int pre, int post, double *out)
{
    if (spec_check_layout(h, ld, C)) return DSS_EINVAL;
    if (dss_spec_check_trials(n_rows, n_trials, first, length, h->p.nperseg, h->p.hop) < 0) return DSS_EINVAL;
    const int J = dss_spec_check_locked(n_trials, length, onset, pre, post, h->p.nperseg, h->p.hop);
    if (J < 0) return J;
    if (!x || !out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return (int)spec_host_form(h, x, ld, C, n_trials, first, length, out, (size_t)C * h->d.bins * J, [&](long long base) {
        return spec_run_locked(h, h->d_x, base, ld, C, n_trials, first, length, onset, pre, post, h->d_out, nullptr);
    });
}

extern "C" int dss_spec_mean_dev(dss_spec *h, const double *d_x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                                 const long long *length, double *d_out, void *hip_stream)
{
    if (spec_check_layout(h, ld, C)) return DSS_EINVAL;
    const long long total = dss_spec_check_trials(n_rows, n_trials, first, length, h->p.nperseg, h->p.hop);
    if (total < 0) return DSS_EINVAL;
    if (total == 0) { dss_set_error("mean spectrum: no trials"); return DSS_EINVAL; }
    if (!d_x || !d_out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return spec_run_mean(h, d_x, 0, ld, C, n_trials, first, length, total, d_out, (hipStream_t)hip_stream);
}

extern "C" int dss_spec_mean(dss_spec *h, const double *x, long long n_rows, int ld, int C, int n_trials, const long long *first,
                             const long long *length, double *out)
{
    if (spec_check_layout(h, ld, C)) return DSS_EINVAL;
    const long long total = dss_spec_check_trials(n_rows, n_trials, first, length, h->p.nperseg, h->p.hop);
    if (total < 0) return DSS_EINVAL;
    if (total == 0) { dss_set_error("mean spectrum: no trials"); return DSS_EINVAL; }
    if (!x || !out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return (int)spec_host_form(h, x, ld, C, n_trials, first, length, out, (size_t)C * h->d.bins, [&](long long base) {
        return spec_run_mean(h, h->d_x, base, ld, C, n_trials, first, length, total, h->d_out, nullptr);
    });
}
