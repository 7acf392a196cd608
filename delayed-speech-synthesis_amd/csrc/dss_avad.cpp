// csrc/dss_avad.cpp -- host side of Part 7 of include/dss_hip.h: acoustic voice-activity labels over a trial list.
//
// Owns the tables (window, twiddles, the mel matrix's nonzero runs), the descriptor and tile tables of a call and the
// staging of the host-buffer form; the arithmetic of steps 3-5 runs in csrc/acoustic_vad.hip only.  Every check and the
// threshold / vote of one trial are handle-free host functions, so they are testable without a device; so are the peak and
// the scaling of the prepared audio, which are avad_gain.h's functions, the ones the kernels call.
#include <math.h>

#include <algorithm>
#include <vector>

#include "acoustic_vad.h"
#include "avad_gain.h"
#include "dss_host.h"

struct dss_avad {
    int device = 0;
    dss_avad_params p;
    DssAvadDev d;
    DssDevBlocks blocks;
    double *d_win = nullptr, *d_tw = nullptr, *d_mel_w = nullptr;
    int *d_band_lo = nullptr, *d_band_off = nullptr;
    // per call (one call per handle in flight)
    DssDevTable<DssAvadTrialDesc> desc;
    DssDevTable<DssAvadTile> tiles;
    DssDevArray<double> d_le;                                     // log energies when the caller does not want them
    // staging of the host-buffer form
    DssDevArray<short> d_audio;
    DssDevArray<unsigned char> d_labels;
    DssDevArray<double> d_le_out, d_thr;
    // the prepared audio (dss_avad_set_gain, dss_avad_prepare_trials*)
    double *d_gain = nullptr;            bool gain_set = false;
    DssDevTable<DssAvadPeakTile> ptiles;
    DssDevTable<DssAvadTile> stiles;
    DssDevArray<int> d_peaks;
    DssDevArray<short> d_prep;
};

// One call's outputs and options, all optional but for what the entry point demands.
struct AvadCall {
    const unsigned char *silence = nullptr, *normalize = nullptr;
    unsigned char *d_labels = nullptr;
    double *d_le = nullptr, *d_thr = nullptr;
    short *d_prepared = nullptr;
    int *d_peaks = nullptr;
    long long n_avail = 0;               // samples behind audio_base that d_audio holds (the peak's cut is clamped there)
};

extern "C" int dss_avad_check_params(const dss_avad_params *p)
{
    if (!p) { dss_set_error("acoustic VAD: no parameters"); return DSS_EINVAL; }
    if (p->window < 4 || (p->window & 3)) { dss_set_error("acoustic VAD: the window must be a positive multiple of 4 samples, not %d", p->window); return DSS_EINVAL; }
    if (p->shift < 1 || p->shift > p->window) { dss_set_error("acoustic VAD: frame shift %d outside 1 .. window (%d)", p->shift, p->window); return DSS_EINVAL; }
    if (p->n_bins != p->window / 2 + 1) { dss_set_error("acoustic VAD: %d bins for a window of %d samples (expected %d)", p->n_bins, p->window, p->window / 2 + 1); return DSS_EINVAL; }
    if (p->n_bands < 1 || p->n_bands > AVAD_MAX_BANDS) { dss_set_error("acoustic VAD: 1 .. %d mel bands supported, not %d", AVAD_MAX_BANDS, p->n_bands); return DSS_EINVAL; }
    if (p->frames_context < 0) { dss_set_error("acoustic VAD: frames_context must not be negative"); return DSS_EINVAL; }
    if (!(p->energy_mean_scale >= 0.0)) { dss_set_error("acoustic VAD: energy_mean_scale must not be negative"); return DSS_EINVAL; }
    if (!(p->proportion_threshold > 0.0 && p->proportion_threshold < 1.0)) { dss_set_error("acoustic VAD: proportion_threshold must lie inside (0, 1)"); return DSS_EINVAL; }
    if (!isfinite(p->energy_threshold)) { dss_set_error("acoustic VAD: energy_threshold is not finite"); return DSS_EINVAL; }
    if (dss_avad_energy_lds_bytes(p->window, p->shift, p->n_bins, p->n_bands) > AVAD_LDS_LIMIT) {
        dss_set_error("acoustic VAD: a window of %d samples shifted by %d does not fit the energy kernel's tile", p->window, p->shift);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

extern "C" int dss_avad_trial_frames_for(int n, int window, int shift)
{
    if (window <= 0 || shift <= 0) { dss_set_error("acoustic VAD: bad frame shape"); return DSS_EINVAL; }
    if (n < window) { dss_set_error("a trial of %d samples is shorter than one window (%d samples)", n, window); return DSS_EINVAL; }
    return (n - window) / shift + 1;
}

// frames = false: the list of a call that wants the prepared audio only, where a trial may be shorter than one window
static int avad_check_list(long long n_audio, int n_trials, const long long *first, const int *len, const int *lead, int window,
                           int shift, bool frames)
{
    if (window <= 0 || shift <= 0) { dss_set_error("acoustic VAD: bad frame shape"); return DSS_EINVAL; }
    if (n_trials < 0 || n_audio < 0) { dss_set_error("bad trial list: negative count"); return DSS_EINVAL; }
    if (n_trials && (!first || !len || !lead)) { dss_set_error("bad trial list: missing array"); return DSS_EINVAL; }
    long long total = 0;
    for (int i = 0; i < n_trials; ++i) {
        if (first[i] < 0 || len[i] < 0) { dss_set_error("trial %d: negative first sample or length", i); return DSS_EINVAL; }
        if (lead[i] < 0 || lead[i] > len[i]) { dss_set_error("trial %d: %d leading zeros in a trial of %d samples", i, lead[i], len[i]); return DSS_EINVAL; }
        if (first[i] > n_audio || (long long)(len[i] - lead[i]) > n_audio - first[i]) {
            dss_set_error("trial %d (samples %lld .. %lld) lies outside the audio of %lld samples", i, first[i],
                          first[i] + (long long)(len[i] - lead[i]), n_audio);
            return DSS_EINVAL;
        }
        if (!frames) continue;
        if (len[i] < window) { dss_set_error("trial %d: %d samples are shorter than one window (%d samples)", i, len[i], window); return DSS_EINVAL; }
        total += (len[i] - window) / shift + 1;
        if (total > 0x7fffffffLL) { dss_set_error("trial list emits more than 2^31 - 1 frames"); return DSS_EINVAL; }
    }
    return (int)total;
}

extern "C" int dss_avad_check_trials(long long n_audio, int n_trials, const long long *first, const int *len, const int *lead,
                                     int window, int shift)
{
    return avad_check_list(n_audio, n_trials, first, len, lead, window, shift, true);
}

extern "C" int dss_avad_peak_tile(void) { return AVAD_PEAK_TILE; }

extern "C" int dss_avad_peak_host(const int16_t *x, long long n)
{
    if (n < 0 || (n && !x)) { dss_set_error("acoustic VAD peak: bad arguments"); return DSS_EINVAL; }
    int m = 0;
    for (long long i = 0; i < n; ++i) m = std::max(m, avad_abs16(x[i]));
    return m;
}

extern "C" int dss_avad_scale_host(const int16_t *x, long long n, double factor, int16_t *out)
{
    if (n < 0 || (n && (!x || !out))) { dss_set_error("acoustic VAD scale: bad arguments"); return DSS_EINVAL; }
    if (!isfinite(factor)) { dss_set_error("acoustic VAD scale: the factor is not finite"); return DSS_EINVAL; }
    for (long long i = 0; i < n; ++i) out[i] = avad_scale(x[i], factor);
    return DSS_OK;
}

// the sum of the device kernel (avad_vote_kernel): 256 strided running sums, then a halving tree
static double avad_ordered_sum(const double *x, int W)
{
    double part[256];
    for (int t = 0; t < 256; ++t) {
        double s = 0.0;
        for (int i = t; i < W; i += 256) s += x[i];
        part[t] = s;
    }
    for (int o = 128; o > 0; o >>= 1)
        for (int t = 0; t < o; ++t) part[t] += part[t + o];
    return part[0];
}

extern "C" int dss_avad_vote_host(const double *log_energy, int W, const dss_avad_params *p, unsigned char *labels, double *threshold)
{
    if (!log_energy || !labels || !p || W <= 0) { dss_set_error("acoustic VAD vote: bad arguments"); return DSS_EINVAL; }
    if (p->frames_context < 0 || !(p->energy_mean_scale >= 0.0) || !(p->proportion_threshold > 0.0 && p->proportion_threshold < 1.0)) {
        dss_set_error("acoustic VAD vote: bad parameters");
        return DSS_EINVAL;
    }
    double thr = p->energy_threshold;
    if (p->energy_mean_scale != 0.0) thr += p->energy_mean_scale * avad_ordered_sum(log_energy, W) / (double)W;
    if (threshold) *threshold = thr;
    for (int i = 0; i < W; ++i) {
        int num = 0, den = 0;
        for (long long t2 = (long long)i - p->frames_context; t2 < (long long)i + p->frames_context; ++t2) {
            if (t2 >= 0 && t2 < W) {
                ++den;
                if (log_energy[t2] > thr) ++num;
            }
        }
        labels[i] = (double)num >= (double)den * p->proportion_threshold ? 1 : 0;
    }
    return DSS_OK;
}

extern "C" void dss_avad_destroy(dss_avad *h) { dss_destroy_handle(h); }

static int avad_setup(dss_avad *h, const double *window_fn, const double *mel)
{
    const dss_avad_params &p = h->p;
    const int N = p.window;
    std::vector<double> win((size_t)N);
    const std::vector<double> tw = dss_twiddles(N);
    for (int j = 0; j < N; ++j) win[j] = window_fn[j] * (1.0 / 32768.0);          // exact: x / 2^15 * w == x * (w * 2^-15)
    // every band's column of the mel matrix as its run first nonzero .. last nonzero (a triangular filter: one run)
    std::vector<double> mel_w;
    std::vector<int> lo((size_t)p.n_bands), off((size_t)p.n_bands + 1);
    for (int b = 0; b < p.n_bands; ++b) {
        int a = -1, z = -1;
        for (int k = 0; k < p.n_bins; ++k) {
            const double w = mel[(size_t)k * p.n_bands + b];
            if (!isfinite(w)) { dss_set_error("acoustic VAD: the mel matrix holds a non-finite value"); return DSS_EINVAL; }
            if (w != 0.0) { if (a < 0) a = k; z = k; }
        }
        off[b] = (int)mel_w.size();
        lo[b] = a < 0 ? 0 : a;
        for (int k = a; a >= 0 && k <= z; ++k) mel_w.push_back(mel[(size_t)k * p.n_bands + b]);
    }
    off[p.n_bands] = (int)mel_w.size();
    if (mel_w.empty()) mel_w.push_back(0.0);
    int rc = h->blocks.upload(win.data(), win.size(), &h->d_win);
    if (!rc) rc = h->blocks.upload(tw.data(), tw.size(), &h->d_tw);
    if (!rc) rc = h->blocks.upload(mel_w.data(), mel_w.size(), &h->d_mel_w);
    if (!rc) rc = h->blocks.upload(lo.data(), lo.size(), &h->d_band_lo);
    if (!rc) rc = h->blocks.upload(off.data(), off.size(), &h->d_band_off);
    if (rc) return rc;
    DssAvadDev &d = h->d;
    d.N = N; d.shift = p.shift; d.bins = p.n_bins; d.bands = p.n_bands; d.context = p.frames_context;
    d.threshold = p.energy_threshold; d.mean_scale = p.energy_mean_scale; d.proportion = p.proportion_threshold;
    d.win = h->d_win; d.tw = h->d_tw; d.mel_w = h->d_mel_w; d.band_lo = h->d_band_lo; d.band_off = h->d_band_off;
    return DSS_OK;
}

extern "C" dss_avad *dss_avad_create(const dss_avad_params *p, const double *window_fn, const double *mel)
{
    if (dss_avad_check_params(p)) return nullptr;
    if (!window_fn || !mel) { dss_set_error("acoustic VAD: missing window or mel matrix"); return nullptr; }
    if (dss_ensure_device()) return nullptr;
    dss_avad *h = new dss_avad;
    h->p = *p;
    hipGetDevice(&h->device);
    if (avad_setup(h, window_fn, mel)) { dss_avad_destroy(h); return nullptr; }
    return h;
}

extern "C" int dss_avad_set_gain(dss_avad *h, const double *gain_by_peak, double post_gain)
{
    if (!gain_by_peak) { dss_set_error("acoustic VAD gain: bad arguments"); return DSS_EINVAL; }
    // the data is judged before the handle is looked at, so that the refusals need no device
    for (int k = 0; k < AVAD_GAIN_ENTRIES; ++k)
        if (!isfinite(gain_by_peak[k]) || gain_by_peak[k] < 0.0) {
            dss_set_error("acoustic VAD gain: the factor of peak %d is negative or not finite", k);
            return DSS_EINVAL;
        }
    if (!isfinite(post_gain) || post_gain < 0.0) { dss_set_error("acoustic VAD gain: the post gain is negative or not finite"); return DSS_EINVAL; }
    if (!h) { dss_set_error("acoustic VAD gain: no handle"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    DSS_HIP_CHECK(hipDeviceSynchronize());                            // a call still queued reads the table it was issued with
    if (!h->d_gain) {
        int rc = h->blocks.upload(gain_by_peak, (size_t)AVAD_GAIN_ENTRIES, &h->d_gain);
        if (rc) return rc;
    } else {
        DSS_HIP_CHECK(hipMemcpy(h->d_gain, gain_by_peak, sizeof(double) * AVAD_GAIN_ENTRIES, hipMemcpyHostToDevice));
    }
    h->d.gain = h->d_gain;
    h->d.post_gain = post_gain;
    h->gain_set = true;
    return DSS_OK;
}

// The trial list on device-resident audio.  d_audio holds samples audio_base .. audio_base + c.n_avail of the caller's array.
// Launches: peak (when a trial is normalised or the peaks are asked for), energy and vote (when labels are asked for), prepared
// audio (when asked for); nothing waits for the device in between.
static int avad_run(dss_avad *h, const short *d_audio, long long audio_base, int n_trials, const long long *first, const int *len,
                    const int *lead, const AvadCall &c, hipStream_t st)
{
    const int N = h->p.window, shift = h->p.shift;
    const bool want_frames = c.d_labels != nullptr;
    bool use_gain = false;
    for (int i = 0; c.normalize && i < n_trials; ++i) use_gain = use_gain || c.normalize[i];
    if (use_gain && !h->gain_set) { dss_set_error("acoustic VAD: trials to normalise but no gain table set (dss_avad_set_gain)"); return DSS_EINVAL; }
    const bool want_peaks = use_gain || c.d_peaks;
    // descriptor table, longest trial first: the long trials' tiles start first and the short ones fill the tail
    const std::vector<int> order = trials_longest_first(n_trials, len);
    const std::vector<long long> out_frame = trials_offsets(n_trials, [&](int i) { return want_frames ? (len[i] - N) / shift + 1 : 0; });
    const std::vector<long long> out_sample = trials_offsets(n_trials, [&](int i) { return len[i]; });
    const long long total = out_frame[n_trials];
    std::vector<DssAvadTile> &tiles = h->tiles.host, &stiles = h->stiles.host;
    std::vector<DssAvadPeakTile> &ptiles = h->ptiles.host;
    h->desc.host.resize((size_t)n_trials);
    tiles.clear(); ptiles.clear(); stiles.clear();
    for (int k = 0; k < n_trials; ++k) {
        const int i = order[k];
        DssAvadTrialDesc &t = h->desc.host[k];
        t.first = first[i] - audio_base; t.out_frame = out_frame[i]; t.out_sample = out_sample[i]; t.n = len[i]; t.lead = lead[i];
        t.W = want_frames ? (len[i] - N) / shift + 1 : 0; t.silence = c.silence && c.silence[i] ? 1 : 0; t.index = i;
        t.normalize = c.normalize && c.normalize[i] ? 1 : 0;
        for (int f0 = 0; f0 < t.W; f0 += AVAD_TILE_FRAMES) tiles.push_back(DssAvadTile{k, f0});
        if (want_peaks) {
            // the cut audio[first .. first + n), clamped where the audio ends: the last `lead` samples count although the shift drops them
            const long long cut = std::min((long long)len[i], c.n_avail - t.first);
            for (long long s0 = 0; s0 < cut; s0 += AVAD_PEAK_TILE)
                ptiles.push_back(DssAvadPeakTile{t.first + s0, (int)std::min((long long)AVAD_PEAK_TILE, cut - s0), i});
        }
        if (c.d_prepared)
            for (long long s0 = 0; s0 < t.n; s0 += AVAD_PEAK_TILE) stiles.push_back(DssAvadTile{k, (int)s0});
    }
    if (tiles.size() > 0x7fffffffULL || ptiles.size() > 0x7fffffffULL || stiles.size() > 0x7fffffffULL) {
        dss_set_error("acoustic VAD: too many tiles for one launch");
        return DSS_EINVAL;
    }
    double *d_le = c.d_le;
    int *d_peaks = c.d_peaks;
    int rc = DSS_OK;
    if (want_frames && !d_le) { rc = h->d_le.grow_headroom(h->blocks, (size_t)total); d_le = h->d_le; }
    if (!rc && want_peaks && !d_peaks) { rc = h->d_peaks.grow_headroom(h->blocks, (size_t)n_trials); d_peaks = h->d_peaks; }
    if (!rc) rc = h->desc.upload(h->blocks, st);
    if (!rc) rc = h->tiles.upload(h->blocks, st);
    if (rc) return rc;
    if (want_peaks) {
        DSS_HIP_CHECK(hipMemsetAsync(d_peaks, 0, sizeof(int) * (size_t)n_trials, st));
        rc = h->ptiles.upload(h->blocks, st);
        if (!rc) rc = dss_launch_avad_peak(d_audio, h->ptiles.dev, (int)ptiles.size(), d_peaks, st);
        if (rc) return rc;
    }
    if (want_frames) {
        rc = dss_launch_avad_energy(h->d, d_audio, h->desc.dev, h->tiles.dev, (int)tiles.size(), d_le, use_gain ? d_peaks : nullptr, st);
        if (!rc) rc = dss_launch_avad_vote(h->d, h->desc.dev, n_trials, d_le, c.d_labels, c.d_thr, st);
        if (rc) return rc;
    }
    if (c.d_prepared && !stiles.empty()) {
        rc = h->stiles.upload(h->blocks, st);
        if (!rc) rc = dss_launch_avad_prepare(h->d, d_audio, h->desc.dev, h->stiles.dev, (int)stiles.size(), d_peaks, c.d_prepared, st);
        if (rc) return rc;
    }
    return (int)total;
}

extern "C" int dss_avad_labels_trials_dev(dss_avad *h, const int16_t *d_audio, long long n_audio, int n_trials, const long long *first,
                                          const int *len, const int *lead, const unsigned char *silence, unsigned char *d_labels,
                                          double *d_log_energy, double *d_threshold, void *hip_stream)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    const int total = dss_avad_check_trials(n_audio, n_trials, first, len, lead, h->p.window, h->p.shift);
    if (total <= 0) return total;
    if (!d_audio || !d_labels) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    AvadCall c;
    c.silence = silence; c.d_labels = d_labels; c.d_le = d_log_energy; c.d_thr = d_threshold; c.n_avail = n_audio;
    return avad_run(h, d_audio, 0, n_trials, first, len, lead, c, (hipStream_t)hip_stream);
}

extern "C" int dss_avad_labels_trials(dss_avad *h, const int16_t *audio, long long n_audio, int n_trials, const long long *first,
                                      const int *len, const int *lead, const unsigned char *silence, unsigned char *labels,
                                      double *log_energy, double *threshold)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    const int total = dss_avad_check_trials(n_audio, n_trials, first, len, lead, h->p.window, h->p.shift);
    if (total <= 0) return total;
    if (!audio || !labels) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    // only the samples the trials span cross the bus, once, however the trials overlap
    long long lo, hi;
    trials_hull(n_trials, first, len, lead, &lo, &hi);
    int rc = h->d_audio.grow_headroom(h->blocks, (size_t)(hi - lo) + 1);
    if (!rc) rc = h->d_labels.grow_headroom(h->blocks, (size_t)total);
    if (!rc) rc = h->d_le_out.grow_headroom(h->blocks, (size_t)total);
    if (!rc) rc = h->d_thr.grow_headroom(h->blocks, (size_t)n_trials);
    if (rc) return rc;
    if (hi > lo) DSS_HIP_CHECK(hipMemcpy(h->d_audio, audio + lo, sizeof(short) * (size_t)(hi - lo), hipMemcpyHostToDevice));
    AvadCall c;
    c.silence = silence; c.d_labels = h->d_labels; c.d_le = h->d_le_out; c.d_thr = h->d_thr; c.n_avail = hi - lo;
    rc = avad_run(h, h->d_audio, lo, n_trials, first, len, lead, c, nullptr);
    if (rc < 0) return rc;
    DSS_HIP_CHECK(hipMemcpy(labels, h->d_labels, (size_t)total, hipMemcpyDeviceToHost));
    if (log_energy) DSS_HIP_CHECK(hipMemcpy(log_energy, h->d_le_out, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost));
    if (threshold) DSS_HIP_CHECK(hipMemcpy(threshold, h->d_thr, sizeof(double) * (size_t)n_trials, hipMemcpyDeviceToHost));
    return total;
}

// ---- the prepared audio: labels of normalised trials, and the int16 trials themselves ------------------------------------------
static int avad_prepare_check(dss_avad *h, long long n_audio, int n_trials, const long long *first, const int *len, const int *lead,
                              const void *labels, const void *log_energy, const void *threshold, const void *prepared, const void *peaks)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    if (!labels && (log_energy || threshold)) { dss_set_error("acoustic VAD: log energies and thresholds come with the labels only"); return DSS_EINVAL; }
    if (!labels && !prepared && !peaks) { dss_set_error("acoustic VAD: no output asked for"); return DSS_EINVAL; }
    return avad_check_list(n_audio, n_trials, first, len, lead, h->p.window, h->p.shift, labels != nullptr);
}

extern "C" int dss_avad_prepare_trials_dev(dss_avad *h, const int16_t *d_audio, long long n_audio, int n_trials, const long long *first,
                                           const int *len, const int *lead, const unsigned char *silence, const unsigned char *normalize,
                                           unsigned char *d_labels, double *d_log_energy, double *d_threshold, int16_t *d_prepared,
                                           int *d_peaks, void *hip_stream)
{
    const int total = avad_prepare_check(h, n_audio, n_trials, first, len, lead, d_labels, d_log_energy, d_threshold, d_prepared, d_peaks);
    if (total < 0 || n_trials == 0) return total;
    if (!d_audio) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    AvadCall c;
    c.silence = silence; c.normalize = normalize; c.d_labels = d_labels; c.d_le = d_log_energy; c.d_thr = d_threshold;
    c.d_prepared = d_prepared; c.d_peaks = d_peaks; c.n_avail = n_audio;
    return avad_run(h, d_audio, 0, n_trials, first, len, lead, c, (hipStream_t)hip_stream);
}

extern "C" int dss_avad_prepare_trials(dss_avad *h, const int16_t *audio, long long n_audio, int n_trials, const long long *first,
                                       const int *len, const int *lead, const unsigned char *silence, const unsigned char *normalize,
                                       unsigned char *labels, double *log_energy, double *threshold, int16_t *prepared, int *peaks)
{
    const int total = avad_prepare_check(h, n_audio, n_trials, first, len, lead, labels, log_energy, threshold, prepared, peaks);
    if (total < 0 || n_trials == 0) return total;
    if (!audio) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    // the whole cut of every trial crosses the bus (the peak is taken over the samples the shift drops too), clamped at the end
    long long lo, hi, samples = 0;
    trials_hull(n_trials, first, len, nullptr, &lo, &hi);
    hi = std::max(lo, std::min(hi, n_audio));
    for (int i = 0; i < n_trials; ++i) samples += len[i];
    int rc = h->d_audio.grow_headroom(h->blocks, (size_t)(hi - lo) + 1);
    if (!rc && labels) rc = h->d_labels.grow_headroom(h->blocks, (size_t)total);
    if (!rc && labels) rc = h->d_le_out.grow_headroom(h->blocks, (size_t)total);
    if (!rc && labels) rc = h->d_thr.grow_headroom(h->blocks, (size_t)n_trials);
    if (!rc && prepared) rc = h->d_prep.grow_headroom(h->blocks, (size_t)samples + 1);
    if (!rc && peaks) rc = h->d_peaks.grow_headroom(h->blocks, (size_t)n_trials);
    if (rc) return rc;
    if (hi > lo) DSS_HIP_CHECK(hipMemcpy(h->d_audio, audio + lo, sizeof(short) * (size_t)(hi - lo), hipMemcpyHostToDevice));
    AvadCall c;
    c.silence = silence; c.normalize = normalize; c.n_avail = hi - lo;
    if (labels) { c.d_labels = h->d_labels; c.d_le = h->d_le_out; c.d_thr = h->d_thr; }
    if (prepared) c.d_prepared = h->d_prep;
    if (peaks) c.d_peaks = h->d_peaks;
    rc = avad_run(h, h->d_audio, lo, n_trials, first, len, lead, c, nullptr);
    if (rc < 0) return rc;
    if (labels && total) DSS_HIP_CHECK(hipMemcpy(labels, h->d_labels, (size_t)total, hipMemcpyDeviceToHost));
    if (log_energy && total) DSS_HIP_CHECK(hipMemcpy(log_energy, h->d_le_out, sizeof(double) * (size_t)total, hipMemcpyDeviceToHost));
    if (threshold) DSS_HIP_CHECK(hipMemcpy(threshold, h->d_thr, sizeof(double) * (size_t)n_trials, hipMemcpyDeviceToHost));
    if (prepared && samples) DSS_HIP_CHECK(hipMemcpy(prepared, h->d_prep, sizeof(short) * (size_t)samples, hipMemcpyDeviceToHost));
    if (peaks) DSS_HIP_CHECK(hipMemcpy(peaks, h->d_peaks, sizeof(int) * (size_t)n_trials, hipMemcpyDeviceToHost));
    return total;
}
