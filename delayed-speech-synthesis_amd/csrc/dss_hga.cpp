// csrc/dss_hga.cpp -- host side of the high-gamma extractor of the C ABI (include/dss_hip.h; csrc/hga_kernels.hip): streaming,
// front end, bad-channel patches and trial lists.  The only numbers produced on the host are the final log() of
// dss_hga_log_power and of the host-buffer forms ("HGA log"), their patch and z-score.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dss_host.h"

// ------------------------------------------------------------------------------------------------------
// HGA
// ------------------------------------------------------------------------------------------------------
extern "C" int dss_hga_num_windows(int T, int sr, float window_length, float window_shift)
{
    // hga_optimized.pyx:36 -- float32 products, C floor()
    return (int)floor((T - window_length * sr) / (window_shift * sr)) + 1;
}

extern "C" int dss_hga_log_power(const double *data, int T, int C, int sr, float wl, float ws, double *out)
{
    if (!data || !out || T <= 0 || C <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    int rc = dss_ensure_device();
    if (rc) return rc;
    const int W = dss_hga_num_windows(T, sr, wl, ws);
    if (W <= 0) return DSS_OK;
    DssDevBlocks mem;
    double *d_in = nullptr, *d_out = nullptr;
    rc = mem.alloc_bytes(sizeof(double) * (size_t)T * C, (void **)&d_in);
    if (!rc) rc = mem.alloc_bytes(sizeof(double) * (size_t)W * C, (void **)&d_out);
    if (rc) { mem.free_all(); return rc; }
    DSS_HIP_CHECK(hipMemcpy(d_in, data, sizeof(double) * (size_t)T * C, hipMemcpyHostToDevice));
    rc = dss_launch_log_power(d_in, T, C, sr, wl, ws, W, d_out, 0, 0);
    if (!rc) {
        hipError_t e = hipMemcpy(out, d_out, sizeof(double) * (size_t)W * C, hipMemcpyDeviceToHost);
        if (e != hipSuccess) { dss_set_error("copy back failed: %s", hipGetErrorString(e)); rc = DSS_ENODEV; }
    }
    mem.free_all();
    if (rc) return rc;
    for (size_t k = 0; k < (size_t)W * C; ++k) out[k] = log(out[k]);       // pyx:46, host libm (DESIGN.md "HGA log")
    return DSS_OK;
}

// hga_optimized.pyx:72-74 (float32 products truncated to int): rows of a frame and rows between two frames
static void hga_window_rows(int fs, float window_length, float window_shift, int *frame_length, int *shift)
{
    *shift = (int)(window_shift * fs);
    *frame_length = (int)(window_length * fs);
}

/* What serves a window shape, without a device: out = {frame_length, shift, overlap, ring_rows, ring_bytes, fused}.  The ring is
 * dss_hga_ring's (csrc/dss_common.h), the one dss_launch_hga and dss_launch_hga_trials size their launches by: fused = 1 means
 * one launch per call (hga_fused_kernel) and a serviceable trial list, 0 the three-launch form and no trial list. */
extern "C" int dss_hga_plan(int fs, float window_length, float window_shift, int out[6])
{
    if (!out) { dss_set_error("nowhere to write the plan"); return DSS_EINVAL; }
    int fl, shift;
    hga_window_rows(fs, window_length, window_shift, &fl, &shift);
    if (fs <= 0 || fl <= 0 || shift <= 0 || shift > fl) { dss_set_error("bad window shape"); return DSS_EINVAL; }
    if (fl > (1 << 24)) { dss_set_error("a frame of %d rows is too long", fl); return DSS_EINVAL; }
    const DssHgaRing ring = dss_hga_ring(fl, fl - shift);
    out[0] = fl; out[1] = shift; out[2] = fl - shift; out[3] = ring.rows; out[4] = (int)ring.bytes; out[5] = ring.fused ? 1 : 0;
    return DSS_OK;
}

struct dss_hga {
    int device;
    DssHgaDev d;
    DssDevBlocks blocks;
    int first_frame = 1;
    // optional fused front end
    int c_raw = 0, n_grids = 0;
    int *d_src_col = nullptr, *d_grid_of = nullptr, *d_comp_cols = nullptr, *d_comp_off = nullptr;
    DssDevArray<double> d_pre, d_raw, d_wire;
    double *d_zi0[2] = {nullptr, nullptr};
    DssDevArray<double> d_in, d_out;
    double *d_zs[2] = {nullptr, nullptr};                  // z-score mean / std on the device ...
    std::vector<double> zs_host[2];                        // ... and on the host (host-buffer entry points); empty = no z-score
    std::vector<double> zs_dev[2];                         // the values the resident device copies hold (dss_hga_set_zscore)
    // trial lists (dss_hga_extract_trials*): bad-channel patches, the descriptor table and the host-buffer form's staging
    std::vector<int> patch_dst, patch_cols, patch_off;     // empty = no patch
    int *d_patch_dst = nullptr, *d_patch_cols = nullptr, *d_patch_off = nullptr;
    DssDevTable<DssHgaTrialDesc> desc;
    DssDevTable<long long> single_rows;                    // output frames of the trials that emit one frame
    DssDevArray<double> d_trec, d_tout;
};

static int hga_grow_rows(dss_hga *h, int need_rows)
{
    if (need_rows <= h->d.cap_rows) return DSS_OK;
    const int cap = need_rows + h->d.frame_length;
    double *nr = nullptr;
    int rc = h->blocks.alloc_bytes(sizeof(double) * (size_t)h->d.S * cap * h->d.C, (void **)&nr);
    if (rc) return rc;
    if (h->d.rows) {
        DSS_HIP_CHECK(hipMemcpy2D(nr, sizeof(double) * (size_t)cap * h->d.C, h->d.rows,
                                  sizeof(double) * (size_t)h->d.cap_rows * h->d.C,
                                  sizeof(double) * (size_t)h->d.overlap * h->d.C, h->d.S, hipMemcpyDeviceToDevice));
        h->blocks.release(h->d.rows);
    }
    h->d.rows = nr;
    h->d.cap_rows = cap;
    return DSS_OK;
}

extern "C" dss_hga *dss_hga_create(int n_streams, int n_channels, int fs, float window_length, float window_shift,
                                   int n_sections, const double *sos_hg, const double *sos_fh, const double *zi_hg,
                                   const double *zi_fh)
{
    if (n_streams <= 0 || n_channels <= 0 || n_sections <= 0 || n_sections > 8 || !sos_hg || !sos_fh || !zi_hg || !zi_fh) {
        dss_set_error("bad HGA arguments (1..8 second-order sections supported)");
        return nullptr;
    }
    if (dss_ensure_device()) return nullptr;
    dss_hga *h = new dss_hga;
    hipGetDevice(&h->device);
    DssHgaDev &d = h->d;
    memset(&d, 0, sizeof(d));
    d.S = n_streams; d.C = n_channels; d.fs = fs; d.nsec = n_sections; d.wl = window_length; d.ws = window_shift;
    int shift;
    hga_window_rows(fs, window_length, window_shift, &d.frame_length, &shift);
    d.overlap = d.frame_length - shift;
    for (int q = 0; q < n_sections; ++q)
        for (int k = 0; k < 6; ++k) { d.sos[0][q][k] = sos_hg[q * 6 + k]; d.sos[1][q][k] = sos_fh[q * 6 + k]; }
    int rc = h->blocks.alloc<double>((size_t)n_streams * 2 * 8 * 2 * n_channels, &d.zi);
    rc |= h->blocks.upload<double>(zi_hg, (size_t)n_sections * 2, &h->d_zi0[0]);
    rc |= h->blocks.upload<double>(zi_fh, (size_t)n_sections * 2, &h->d_zi0[1]);
    if (!rc) rc = hga_grow_rows(h, d.overlap + 4 * d.frame_length);
    if (!rc) rc = dss_launch_hga_reset(d, h->d_zi0[0], h->d_zi0[1], 0);
    if (!rc && hipDeviceSynchronize() != hipSuccess) rc = DSS_ENODEV;
    if (rc) { dss_set_error("HGA device setup failed"); dss_hga_destroy(h); return nullptr; }
    return h;
}

extern "C" void dss_hga_destroy(dss_hga *h)
{
    if (!h) return;
    hipSetDevice(h->device);
    h->blocks.free_all();
    delete h;
}

extern "C" int dss_hga_reset(dss_hga *h)
{
    if (!h) return DSS_EINVAL;
    DSS_HIP_CHECK(hipSetDevice(h->device));
    int rc = dss_launch_hga_reset(h->d, h->d_zi0[0], h->d_zi0[1], 0);
    if (rc) return rc;
    DSS_HIP_CHECK(hipStreamSynchronize(0));
    h->first_frame = 1;
    return DSS_OK;
}

// rows the frame buffer hands to the window stage for n new samples, and where the new rows start
static void hga_plan(const dss_hga *h, int n, int *row0, int *zero_rows, int *rows)
{
    const int fl = h->d.frame_length, ov = h->d.overlap;
    if (h->first_frame && n >= fl) { *row0 = 0; *zero_rows = 0; *rows = n; }                      // CASE 1, pyx:104-107
    else if (h->first_frame) { *row0 = fl - n; *zero_rows = fl - n; *rows = fl; }                  // CASE 2, pyx:111-122
    else { *row0 = ov; *zero_rows = 0; *rows = ov + n; }                                           // CASE 3, pyx:123-131
}

extern "C" int dss_hga_frames_for(const dss_hga *h, int n)
{
    if (!h || n <= 0) return 0;
    int row0, zr, rows;
    hga_plan(h, n, &row0, &zr, &rows);
    int W = dss_hga_num_windows(rows, h->d.fs, h->d.wl, h->d.ws);
    return W < 0 ? 0 : W;
}

// one call of the extractor on device-resident input: (S, n, C) rows
static int hga_run(dss_hga *h, const double *d_data, int n, double *d_out, int apply_log, hipStream_t s)
{
    int row0, zr, rows;
    hga_plan(h, n, &row0, &zr, &rows);
    int rc = hga_grow_rows(h, rows);
    if (rc) return rc;
    int W = dss_hga_num_windows(rows, h->d.fs, h->d.wl, h->d.ws);
    if (W < 0) W = 0;
    rc = dss_launch_hga(h->d, d_data, n, row0, zr, rows, W, d_out, apply_log, s);
    if (rc) return rc;
    h->first_frame = 0;
    return W;
}

extern "C" int dss_hga_extract_dev(dss_hga *h, const double *d_data, int n, double *d_out, int apply_log, void *hip_stream)
{
    if (!h || !d_data || !d_out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return hga_run(h, d_data, n, d_out, apply_log, (hipStream_t)hip_stream);
}

/* Optional z-score of the frames, (x - mean[c]) / std[c] (ZScoreNormalization, local/common.py:367-376; the last step of
 * the reference's feature chain, decode_online.py:88-97), inside the extractor's launch.  NULL clears it.  The
 * host-buffer entry points apply it on the host after their host-libm log (same two IEEE operations). */
extern "C" int dss_hga_set_zscore(dss_hga *h, const double *means, const double *stds)
{
    if (!h || (!means) != (!stds)) { dss_set_error("z-score needs both means and stds (or neither)"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    // The device copies stay resident: clearing only drops the pointers the kernels see, and setting the values that are
    // already there only restores them -- a caller that toggles the epilogue per call (SegmentPipeline's intermediates
    // tap) pays no hipFree / hipMalloc / copy, i.e. no device-wide synchronisation, in its hot path.
    h->d.zs_mean = h->d.zs_std = nullptr;
    h->zs_host[0].clear(); h->zs_host[1].clear();
    if (!means) return DSS_OK;
    const size_t C = (size_t)h->d.C;
    const bool same = h->d_zs[0] && h->d_zs[1] && h->zs_dev[0].size() == C && !memcmp(h->zs_dev[0].data(), means, C * sizeof(double)) &&
                      !memcmp(h->zs_dev[1].data(), stds, C * sizeof(double));
    if (!same) {
        for (int k = 0; k < 2; ++k) { h->blocks.release(h->d_zs[k]); h->d_zs[k] = nullptr; h->zs_dev[k].clear(); }
        if (h->blocks.upload<double>(means, C, &h->d_zs[0]) || h->blocks.upload<double>(stds, C, &h->d_zs[1])) return DSS_ENOMEM;
        h->zs_dev[0].assign(means, means + C);
        h->zs_dev[1].assign(stds, stds + C);
    }
    h->zs_host[0] = h->zs_dev[0];
    h->zs_host[1] = h->zs_dev[1];
    h->d.zs_mean = h->d_zs[0]; h->d.zs_std = h->d_zs[1];
    return DSS_OK;
}

/* Tests and A/B timing only: 0 = choose (default: hga_fused_kernel, three launches when its ring does not fit),
 * 1 = hga_fused_kernel, 2 = the three-launch form. */
extern "C" int dss_selftest_hga_force_path(dss_hga *h, int path)
{
    if (!h || path < 0 || path > 2) return DSS_EINVAL;
    h->d.force_path = path;
    return DSS_OK;
}

// host-side finish of the host-buffer entry points: glibc log (pyx:46; DESIGN.md "HGA log"), then the optional z-score
static void hga_host_finish(const dss_hga *h, double *out, size_t cnt)
{
    for (size_t k = 0; k < cnt; ++k) out[k] = log(out[k]);
    if (!h->zs_host[0].empty()) {
        const int C = h->d.C;
        for (size_t k = 0; k < cnt; ++k) out[k] = (out[k] - h->zs_host[0][k % C]) / h->zs_host[1][k % C];
    }
}

// the host-buffer entry points take the mean power from the device WITHOUT log and z-score (both are applied on the host)
struct HgaNoZs {
    dss_hga *h; const double *m, *sd;
    explicit HgaNoZs(dss_hga *hh) : h(hh), m(hh->d.zs_mean), sd(hh->d.zs_std) { h->d.zs_mean = h->d.zs_std = nullptr; }
    ~HgaNoZs() { h->d.zs_mean = m; h->d.zs_std = sd; }
};

extern "C" int dss_hga_extract(dss_hga *h, const double *data, int n, double *out)
{
    if (!h || !data || !out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    const size_t in_n = (size_t)h->d.S * n * h->d.C;
    const int Wmax = dss_hga_frames_for(h, n);
    const size_t out_n = (size_t)h->d.S * (Wmax > 0 ? Wmax : 1) * h->d.C;
    int rc = h->d_in.grow(h->blocks, in_n);
    if (!rc) rc = h->d_out.grow(h->blocks, out_n);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(h->d_in, data, in_n * sizeof(double), hipMemcpyHostToDevice));
    int W;
    { HgaNoZs guard(h); W = dss_hga_extract_dev(h, h->d_in, n, h->d_out, 0, nullptr); }
    if (W < 0) return W;
    if (W == 0) { DSS_HIP_CHECK(hipDeviceSynchronize()); return 0; }
    const size_t cnt = (size_t)h->d.S * W * h->d.C;
    DSS_HIP_CHECK(hipMemcpy(out, h->d_out, cnt * sizeof(double), hipMemcpyDeviceToHost));
    hga_host_finish(h, out, cnt);
    return W;
}


extern "C" int dss_hga_set_frontend(dss_hga *h, int c_raw, const int *src_col, const int *grid_of, int n_grids,
                                    const int *comp_cols, const int *comp_off)
{
    if (!h || c_raw <= 0 || !src_col || !grid_of || n_grids < 0 || n_grids > 4 || (n_grids && (!comp_cols || !comp_off))) {
        dss_set_error("bad front-end description (at most 4 grids)");
        return DSS_EINVAL;
    }
    const int C = h->d.C;
    for (int c = 0; c < C; ++c)
        if (src_col[c] < 0 || src_col[c] >= c_raw || grid_of[c] >= n_grids) { dss_set_error("front-end column %d out of range", c); return DSS_EINVAL; }
    const int n_comp = n_grids ? comp_off[n_grids] : 0;
    if (n_comp > 4 * c_raw) { dss_set_error("front end: %d reference columns for %d raw columns", n_comp, c_raw); return DSS_EINVAL; }
    for (int g = 0; g < n_grids; ++g)
        if (comp_off[g + 1] <= comp_off[g]) { dss_set_error("grid %d has no reference channels", g); return DSS_EINVAL; }
    for (int k = 0; k < n_comp; ++k)
        if (comp_cols[k] < 0 || comp_cols[k] >= c_raw) { dss_set_error("reference column out of range"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    int rc = h->blocks.upload<int>(src_col, C, &h->d_src_col);
    rc |= h->blocks.upload<int>(grid_of, C, &h->d_grid_of);
    static const int zero2[2] = {0, 0};
    rc |= h->blocks.upload<int>(n_comp ? comp_cols : zero2, n_comp ? n_comp : 1, &h->d_comp_cols);
    rc |= h->blocks.upload<int>(n_grids ? comp_off : zero2, n_grids + 1, &h->d_comp_off);
    if (rc) return DSS_ENOMEM;
    h->c_raw = c_raw; h->n_grids = n_grids;
    return DSS_OK;
}

extern "C" int dss_hga_extract_raw_dev(dss_hga *h, const double *d_raw, int n, double *d_out, int apply_log, void *hip_stream)
{
    if (!h || !h->c_raw) { dss_set_error("no front end configured (dss_hga_set_frontend)"); return DSS_EINVAL; }
    if (!d_raw || !d_out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    // two launches: the front end (HBM-bound), then the extractor (a one-launch form measured slower, profiles/r3_hga_experiment.md)
    const size_t need = (size_t)h->d.S * n * h->d.C;
    int rc = h->d_pre.grow(h->blocks, need);
    if (rc) return rc;
    rc = dss_launch_hga_frontend(d_raw, h->d_pre, h->d.S, n, h->c_raw, h->d.C, h->d_src_col, h->d_grid_of, h->n_grids,
                                     h->d_comp_cols, h->d_comp_off, (hipStream_t)hip_stream);
    if (rc) return rc;
    return dss_hga_extract_dev(h, h->d_pre, n, d_out, apply_log, hip_stream);
}

// Payloads in wire format (float32, [stream][channel][sample]: the body of the amplifier's packets) -> frames.  With a front end
// configured the payload carries its c_raw channels and goes through it, otherwise the extractor's own n_channels.
extern "C" int dss_hga_extract_wire_dev(dss_hga *h, const float *d_payload, int n, double *d_out, int apply_log, void *hip_stream)
{
    if (!h || !d_payload || !d_out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    const int c_in = h->c_raw ? h->c_raw : h->d.C;
    const size_t need = (size_t)h->d.S * n * c_in;
    int rc = h->d_wire.grow(h->blocks, need);
    if (rc) return rc;
    rc = dss_launch_hga_wire(d_payload, h->d_wire, h->d.S, c_in, n, (hipStream_t)hip_stream);
    if (rc) return rc;
    return h->c_raw ? dss_hga_extract_raw_dev(h, h->d_wire, n, d_out, apply_log, hip_stream)
                    : dss_hga_extract_dev(h, h->d_wire, n, d_out, apply_log, hip_stream);
}

extern "C" int dss_hga_extract_raw(dss_hga *h, const double *raw, int n, double *out)
{
    if (!h || !h->c_raw) { dss_set_error("no front end configured (dss_hga_set_frontend)"); return DSS_EINVAL; }
    if (!raw || !out || n <= 0) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    const size_t in_n = (size_t)h->d.S * n * h->c_raw;
    int rc = h->d_raw.grow(h->blocks, in_n);
    if (rc) return rc;
    const int Wmax = dss_hga_frames_for(h, n);
    const size_t out_n = (size_t)h->d.S * (Wmax > 0 ? Wmax : 1) * h->d.C;
    rc = h->d_out.grow(h->blocks, out_n);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(h->d_raw, raw, in_n * sizeof(double), hipMemcpyHostToDevice));
    int W;
    { HgaNoZs guard(h); W = dss_hga_extract_raw_dev(h, h->d_raw, n, h->d_out, 0, nullptr); }
    if (W < 0) return W;
    if (W == 0) { DSS_HIP_CHECK(hipDeviceSynchronize()); return 0; }
    const size_t cnt = (size_t)h->d.S * W * h->d.C;
    DSS_HIP_CHECK(hipMemcpy(out, h->d_out, cnt * sizeof(double), hipMemcpyDeviceToHost));
    hga_host_finish(h, out, cnt);
    return W;
}

// ---- trial lists: a session's trials in one call (baseline_offline.py:45-60, prepare_corpus.py:42-52,179-199) -------------
// Frames a FRESH extractor emits for one chunk of `len` rows: CASE 1 (pyx:104-107) from len rows, CASE 2 (pyx:111-122) one
// zero-padded frame; a chunk no longer than the frame shift is what the reference's frame buffer must not be given (pyx:57).
extern "C" int dss_hga_trial_frames_for(int fs, float wl, float ws, int len)
{
    int shift, fl;
    hga_window_rows(fs, wl, ws, &fl, &shift);
    if (fs <= 0 || fl <= 0 || shift <= 0 || shift > fl) { dss_set_error("bad window shape"); return DSS_EINVAL; }
    if (len <= shift) { dss_set_error("a trial of %d rows is not longer than the frame shift (%d rows)", len, shift); return DSS_EINVAL; }
    const int W = dss_hga_num_windows(len >= fl ? len : fl, fs, wl, ws);
    return W < 0 ? 0 : W;
}

extern "C" int dss_hga_trial_frames(const dss_hga *h, int len)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    return dss_hga_trial_frames_for(h->d.fs, h->d.wl, h->d.ws, len);
}

// every trial inside the recording and long enough; returns the frames of the whole list
extern "C" int dss_hga_check_trials(int fs, float wl, float ws, long long T_rec, int n_trials, const long long *start, const int *len)
{
    if (n_trials < 0 || T_rec < 0 || (n_trials && (!start || !len))) { dss_set_error("bad trial list"); return DSS_EINVAL; }
    long long total = 0;
    for (int i = 0; i < n_trials; ++i) {
        if (start[i] < 0 || len[i] < 0 || start[i] + (long long)len[i] > T_rec) {
            dss_set_error("trial %d (rows %lld .. %lld) lies outside the recording of %lld rows", i, start[i], start[i] + (long long)len[i], T_rec);
            return DSS_EINVAL;
        }
        const int W = dss_hga_trial_frames_for(fs, wl, ws, len[i]);
        if (W < 0) { dss_set_error("trial %d: %d rows are not longer than the frame shift", i, len[i]); return DSS_EINVAL; }
        total += W;
        if (total > 0x7fffffffLL) { dss_set_error("trial list emits more than 2^31 frames"); return DSS_EINVAL; }
    }
    return (int)total;
}

extern "C" int dss_hga_check_patches(int C, int n_patches, const int *dst_col, const int *nb_cols, const int *nb_off)
{
    if (C <= 0 || n_patches < 0 || (n_patches && (!dst_col || !nb_cols || !nb_off))) { dss_set_error("bad patch list"); return DSS_EINVAL; }
    if (n_patches && nb_off[0] != 0) { dss_set_error("patch offsets must start at 0"); return DSS_EINVAL; }
    std::vector<char> is_dst((size_t)C, 0);
    for (int k = 0; k < n_patches; ++k) {
        if (dst_col[k] < 0 || dst_col[k] >= C) { dss_set_error("patch %d: column %d outside 0..%d", k, dst_col[k], C - 1); return DSS_EINVAL; }
        if (is_dst[dst_col[k]]) { dss_set_error("column %d is patched twice", dst_col[k]); return DSS_EINVAL; }
        is_dst[dst_col[k]] = 1;
        if (nb_off[k + 1] <= nb_off[k] || nb_off[k + 1] - nb_off[k] >= 128) { dss_set_error("patch %d: 1..127 neighbours supported", k); return DSS_EINVAL; }
    }
    for (int j = 0; j < (n_patches ? nb_off[n_patches] : 0); ++j) {
        if (nb_cols[j] < 0 || nb_cols[j] >= C) { dss_set_error("neighbour column %d outside 0..%d", nb_cols[j], C - 1); return DSS_EINVAL; }
        if (is_dst[nb_cols[j]]) { dss_set_error("neighbour column %d is itself patched", nb_cols[j]); return DSS_EINVAL; }
    }
    return DSS_OK;
}

// BadChannelCorrection.__call__ (local/common.py:286-291) in place on ONE call's frames (N, C), by numpy's own summation
// order for np.mean(data[:, neighbours], axis=1): with N >= 2 the fancy-indexed copy is Fortran-ordered and is added one
// column at a time (the sequential sum in list order, for 8 neighbours too); with N == 1 it is one contiguous row, which
// numpy's pairwise kernel sums as eight running sums over blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the
// remainder in order (fewer than 8: sequential).  Neighbours are never patched columns (dss_hga_check_patches).
static double hga_row_mean(const double *fr, const int *cols, int n, bool single)
{
    double sum;
    if (!single || n < 8) {
        sum = fr[cols[0]];
        for (int j = 1; j < n; ++j) sum += fr[cols[j]];
    } else {
        double r[8];
        for (int u = 0; u < 8; ++u) r[u] = fr[cols[u]];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int u = 0; u < 8; ++u) r[u] += fr[cols[i + u]];
        sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) sum += fr[cols[i]];
    }
    return sum / (double)n;
}

extern "C" int dss_hga_apply_patches(double *frames, long long N, int C, int n_patches, const int *dst_col, const int *nb_cols,
                                     const int *nb_off)
{
    if (N < 0 || (N && !frames)) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    const int rc = dss_hga_check_patches(C, n_patches, dst_col, nb_cols, nb_off);
    if (rc) return rc;
    for (long long i = 0; i < N; ++i) {
        double *fr = frames + (size_t)i * C;
        for (int k = 0; k < n_patches; ++k)
            fr[dst_col[k]] = hga_row_mean(fr, nb_cols + nb_off[k], nb_off[k + 1] - nb_off[k], N == 1);
    }
    return DSS_OK;
}

// numpy's pairwise_sum over a contiguous run of n elements (element i: a[i], or with sq (a[i] - m) * (a[i] - m)): sequential
// below 8 elements; up to 128 eight running sums over blocks of eight, ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the remainder
// in order; longer runs are halved (the left half a multiple of 8) and the halves' sums added
static double hga_pairwise_sum(const double *a, long long n, double m, bool sq)
{
    auto at = [&](long long i) { const double d = a[i] - m; return sq ? d * d : a[i]; };
    if (n < 8) {
        double r = at(0);
        for (long long i = 1; i < n; ++i) r += at(i);
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int u = 0; u < 8; ++u) r[u] = at(u);
        long long i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int u = 0; u < 8; ++u) r[u] += at(i + u);
        double sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) sum += at(i);
        return sum;
    }
    long long n2 = n / 2;
    n2 -= n2 % 8;
    const double left = hga_pairwise_sum(a, n2, m, sq);
    return left + hga_pairwise_sum(a + n2, n - n2, m, sq);
}

// np.vstack([np.mean(x, axis=0), np.std(x, axis=0)]) of a C-contiguous (N, C) array, in numpy's order: rows are added one
// after the other (row 0, += row 1, ...), / N; std from d = x - mean, d * d summed the same way, / N, sqrt.  ONE column is one
// contiguous run, which numpy sums with its pairwise kernel instead (hga_pairwise_sum), the squares too.
extern "C" int dss_hga_column_stats(const double *frames, long long N, int C, double *out)
{
    if (!frames || !out || N <= 0 || C <= 0) { dss_set_error("column statistics need at least one frame"); return DSS_EINVAL; }
    double *mean = out, *sd = out + C;
    if (C == 1) {
        mean[0] = hga_pairwise_sum(frames, N, 0.0, false) / (double)N;
        sd[0] = sqrt(hga_pairwise_sum(frames, N, mean[0], true) / (double)N);
        return DSS_OK;
    }
    for (int c = 0; c < C; ++c) mean[c] = frames[c];
    for (long long i = 1; i < N; ++i)
        for (int c = 0; c < C; ++c) mean[c] += frames[(size_t)i * C + c];
    for (int c = 0; c < C; ++c) mean[c] = mean[c] / (double)N;
    for (int c = 0; c < C; ++c) { const double d = frames[c] - mean[c]; sd[c] = d * d; }
    for (long long i = 1; i < N; ++i)
        for (int c = 0; c < C; ++c) { const double d = frames[(size_t)i * C + c] - mean[c]; sd[c] += d * d; }
    for (int c = 0; c < C; ++c) sd[c] = sqrt(sd[c] / (double)N);
    return DSS_OK;
}

extern "C" int dss_hga_column_stats_dev(const double *d_frames, long long N, int C, double *d_out, void *hip_stream)
{
    if (!d_frames || !d_out || N <= 0 || C <= 0) { dss_set_error("column statistics need at least one frame"); return DSS_EINVAL; }
    int rc = dss_ensure_device();
    if (rc) return rc;
    return dss_launch_hga_colstats(d_frames, (long)N, C, d_out, (hipStream_t)hip_stream);
}

extern "C" int dss_hga_set_patches(dss_hga *h, int n_patches, const int *dst_col, const int *nb_cols, const int *nb_off)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    if (!dst_col || n_patches == 0) n_patches = 0;
    int rc = dss_hga_check_patches(h->d.C, n_patches, dst_col, nb_cols, nb_off);
    if (rc) return rc;
    DSS_HIP_CHECK(hipSetDevice(h->device));
    int **dev[3] = {&h->d_patch_dst, &h->d_patch_cols, &h->d_patch_off};
    for (int k = 0; k < 3; ++k) { h->blocks.release(*dev[k]); *dev[k] = nullptr; }
    h->patch_dst.clear(); h->patch_cols.clear(); h->patch_off.clear();
    if (!n_patches) return DSS_OK;
    h->patch_dst.assign(dst_col, dst_col + n_patches);
    h->patch_off.assign(nb_off, nb_off + n_patches + 1);
    h->patch_cols.assign(nb_cols, nb_cols + nb_off[n_patches]);
    rc = h->blocks.upload<int>(h->patch_dst.data(), h->patch_dst.size(), &h->d_patch_dst);
    rc |= h->blocks.upload<int>(h->patch_cols.data(), h->patch_cols.size(), &h->d_patch_cols);
    rc |= h->blocks.upload<int>(h->patch_off.data(), h->patch_off.size(), &h->d_patch_off);
    if (rc) { h->patch_dst.clear(); h->patch_cols.clear(); h->patch_off.clear(); return DSS_ENOMEM; }
    return DSS_OK;
}

// The trial list on device-resident rows.  d_rows holds recording rows row_base .. (c_in columns); `finish` = log, patch and
// z-score on the device (the device-resident entry point) or none of them (the host-buffer one finishes on the host).
static int hga_trials_run(dss_hga *h, const double *d_rows, long long row_base, int n_trials, const long long *start, const int *len,
                          double *d_out, int apply_log, bool finish, hipStream_t st)
{
    const DssHgaDev &d = h->d;
    long long lo, hi;
    trials_hull(n_trials, start, len, nullptr, &lo, &hi);
    const double *d_data = d_rows;
    long long data_base = row_base;             // recording row that d_data's row 0 holds
    if (h->c_raw) {
        // the front end runs once over the rows the trials span (they overlap and cover most of a recording), not per trial
        const long long span = hi - lo;
        if (span > 0x7fffffffLL / (h->c_raw > d.C ? h->c_raw : d.C)) { dss_set_error("trial list spans too many rows for one front-end launch"); return DSS_EINVAL; }
        int rc = h->d_pre.grow(h->blocks, (size_t)span * d.C);
        if (rc) return rc;
        rc = dss_launch_hga_frontend(d_rows + (size_t)(lo - row_base) * h->c_raw, h->d_pre, 1, (int)span, h->c_raw, d.C, h->d_src_col,
                                     h->d_grid_of, h->n_grids, h->d_comp_cols, h->d_comp_off, st);
        if (rc) return rc;
        d_data = h->d_pre;
        data_base = lo;
    }
    // descriptor table, longest trial first: the long trials' blocks start first and the short ones fill the tail
    const std::vector<int> order = trials_longest_first(n_trials, len);
    const std::vector<long long> out_row = trials_offsets(n_trials, [&](int i) { return dss_hga_trial_frames_for(d.fs, d.wl, d.ws, len[i]); });
    const long long total = out_row[n_trials];
    h->desc.host.resize((size_t)n_trials);
    for (int k = 0; k < n_trials; ++k) {
        const int i = order[k];
        DssHgaTrialDesc &t = h->desc.host[k];
        t.in_row = start[i] - data_base; t.out_row = out_row[i]; t.n = len[i];
        t.W = dss_hga_trial_frames_for(d.fs, d.wl, d.ws, len[i]);
        t.zero_rows = len[i] >= d.frame_length ? 0 : d.frame_length - len[i];
        t.pad = 0;
    }
    int rc = h->desc.upload_exact(h->blocks, st);
    if (rc) return rc;
    const bool patched = finish && !h->patch_dst.empty();
    const bool zs = finish && d.zs_mean;
    // the patch stands between the log and the z-score (prepare_corpus.py:166-170), so with patches the z-score leaves the
    // trial kernel's epilogue and follows the patch kernel
    rc = dss_launch_hga_trials(d, d_data, h->desc.dev, n_trials, h->d_zi0[0], h->d_zi0[1], d_out, finish ? apply_log : 0,
                                   zs && !patched, st);
    if (rc) return rc;
    if (patched) {
        // the reference patches trial by trial, and numpy sums the neighbours of a ONE-frame call differently (hga_patch_kernel)
        h->single_rows.host.clear();
        for (int i = 0; i < n_trials; ++i)
            if (dss_hga_trial_frames_for(d.fs, d.wl, d.ws, len[i]) == 1) h->single_rows.host.push_back(out_row[i]);
        rc = h->single_rows.upload_exact(h->blocks, st);
        if (rc) return rc;
        rc = dss_launch_hga_patch(d_out, (long)total, d.C, (int)h->patch_dst.size(), h->d_patch_dst, h->d_patch_cols, h->d_patch_off,
                                  h->single_rows.dev, (long)h->single_rows.host.size(), zs ? d.zs_mean : nullptr, zs ? d.zs_std : nullptr, st);
    }
    return rc ? rc : (int)total;
}

extern "C" int dss_hga_extract_trials_dev(dss_hga *h, const double *d_rec, long long T_rec, int n_trials, const long long *start,
                                          const int *len, double *d_out, int apply_log, void *hip_stream)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    const int total = dss_hga_check_trials(h->d.fs, h->d.wl, h->d.ws, T_rec, n_trials, start, len);
    if (total <= 0) return total;
    if (!d_rec || !d_out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    return hga_trials_run(h, d_rec, 0, n_trials, start, len, d_out, apply_log, true, (hipStream_t)hip_stream);
}

extern "C" int dss_hga_extract_trials(dss_hga *h, const double *rec, long long T_rec, int n_trials, const long long *start,
                                      const int *len, double *out)
{
    if (!h) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    const int total = dss_hga_check_trials(h->d.fs, h->d.wl, h->d.ws, T_rec, n_trials, start, len);
    if (total <= 0) return total;
    if (!rec || !out) { dss_set_error("bad arguments"); return DSS_EINVAL; }
    DSS_HIP_CHECK(hipSetDevice(h->device));
    const int c_in = h->c_raw ? h->c_raw : h->d.C;
    long long lo, hi;
    trials_hull(n_trials, start, len, nullptr, &lo, &hi);
    // only the rows the trials span cross the bus, once, however the trials overlap
    int rc = h->d_trec.grow(h->blocks, (size_t)(hi - lo) * c_in);
    if (!rc) rc = h->d_tout.grow(h->blocks, (size_t)total * h->d.C);
    if (rc) return rc;
    DSS_HIP_CHECK(hipMemcpy(h->d_trec, rec + (size_t)lo * c_in, sizeof(double) * (size_t)(hi - lo) * c_in, hipMemcpyHostToDevice));
    rc = hga_trials_run(h, h->d_trec, lo, n_trials, start, len, h->d_tout, 0, false, nullptr);
    if (rc < 0) return rc;
    const size_t cnt = (size_t)total * h->d.C;
    DSS_HIP_CHECK(hipMemcpy(out, h->d_tout, cnt * sizeof(double), hipMemcpyDeviceToHost));
    // host libm log (pyx:46; DESIGN.md "HGA log"), BadChannelCorrection, ZScoreNormalization: the reference's order
    for (size_t k = 0; k < cnt; ++k) out[k] = log(out[k]);
    if (!h->patch_dst.empty()) {
        size_t row = 0;                         // trial by trial, as the reference's post-transform sees the frames
        for (int i = 0; i < n_trials; ++i) {
            const int W = dss_hga_trial_frames_for(h->d.fs, h->d.wl, h->d.ws, len[i]);
            dss_hga_apply_patches(out + row * h->d.C, W, h->d.C, (int)h->patch_dst.size(), h->patch_dst.data(), h->patch_cols.data(),
                                  h->patch_off.data());
            row += (size_t)W;
        }
    }
    if (!h->zs_host[0].empty()) {
        const int C = h->d.C;
        for (size_t k = 0; k < cnt; ++k) out[k] = (out[k] - h->zs_host[0][k % C]) / h->zs_host[1][k % C];
    }
    return total;
}
