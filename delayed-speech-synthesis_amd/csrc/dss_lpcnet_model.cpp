// csrc/dss_lpcnet_model.cpp -- the LPCNet model of the C ABI (include/dss_hip.h): blob -> host model -> device copy.
//
// The only numbers produced on the host are constant tables that xiph/LPCNet itself builds at run time with libm
// (lpcnet_init()'s sampling_logit_table, common.h's ulaw2lin over its 256 integer inputs, freq.c's dct table); all
// arithmetic of the path runs in the HIP kernels (lpcnet_frame.hip, lpcnet_sample.hip).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <mutex>
#include <vector>

#include "dss_host.h"

// ------------------------------------------------------------------------------------------------------
// model: blob -> device
// ------------------------------------------------------------------------------------------------------
struct HostModel {
    std::vector<char> blob;
    dss_blob_header h;
    double bytes_per_sample = 0;
    int refs = 0;                      // decoder batches created from this model (guarded by g_model_mu)
    // per-device uploads
    std::vector<DssModelDev> dev;      // index = device id
    std::vector<char> dev_ready;
    std::vector<DssDevBlocks> dev_blocks;   // everything upload_model() allocated there
};

static std::mutex g_model_mu;
static HostModel *g_model = nullptr;

// free a model's device memory and the host copy (caller holds g_model_mu; refs must be 0)
static void free_model(HostModel *hm)
{
    int cur = -1;
    hipGetDevice(&cur);
    for (size_t dv = 0; dv < hm->dev_blocks.size(); ++dv)
        if (!hm->dev_blocks[dv].blocks.empty()) { hipSetDevice((int)dv); hm->dev_blocks[dv].free_all(); }
    if (cur >= 0) hipSetDevice(cur);
    delete hm;
}

static float host_ulaw2lin(float u)           // xiph common.h
{
    float s;
    float scale_1 = 32768.f / 255.f;
    u = u - 128.f;
    s = (u < 0) ? -1.f : 1.f;
    u = fabsf(u);
    return s * scale_1 * (exp(u / 128. * 5.5451774445f) - 1);
}

// The activation table and, DSS_TANSIG_Y floats behind it, the 1 - y*y that vec.h tanh_approx forms from the entry it
// reads: two separately rounded fp32 operations.  The square goes through a volatile float, so that no compiler setting
// (contraction, excess precision) can fuse it into the subtraction or keep it wider than fp32.
static void dss_tansig_tables(float *t)
{
    for (int i = 0; i < 201; ++i) {
        t[i] = (float)(floor(tanh(.04 * i) * 1e6 + .5) / 1e6);                                       // tansig_table.h
        volatile float yy = t[i] * t[i];
        t[DSS_TANSIG_Y + i] = 1.f - yy;
    }
}

struct BlobView {
    const float *embed_pitch, *conv1_w, *conv1_b, *conv2_w, *conv2_b, *dense1_w, *dense1_b, *dense2_w, *dense2_b;
    const float *gru_a_dense_w, *gru_a_dense_b, *gru_b_dense_w, *gru_b_dense_b, *embed_sig, *embed_pred, *embed_exc;
    const float *gru_a_rbias, *gru_a_diag;
    const int32_t *gru_a_idx;
    const float *gru_a_w, *gru_b_bias, *gru_b_w_in, *gru_b_w_rec, *fc_bias, *fc_w, *fc_factor;
};

static int view_blob(const std::vector<char> &blob, const dss_blob_header &h, BlobView &v)
{
    const float *p = (const float *)(blob.data() + sizeof(dss_blob_header));
    const int fin = h.nb_features + h.embed_pitch_dim, NA3 = 3 * h.gru_a, NB3 = 3 * h.gru_b;
#define TAKE(f, c) do { v.f = p; p += (size_t)(c); } while (0)
    TAKE(embed_pitch, (size_t)h.pitch_max * h.embed_pitch_dim);
    TAKE(conv1_w, (size_t)3 * fin * h.conv1_out);          TAKE(conv1_b, h.conv1_out);
    TAKE(conv2_w, (size_t)3 * h.conv1_out * h.conv2_out);  TAKE(conv2_b, h.conv2_out);
    TAKE(dense1_w, (size_t)h.conv2_out * h.dense1_out);    TAKE(dense1_b, h.dense1_out);
    TAKE(dense2_w, (size_t)h.dense1_out * h.dense2_out);   TAKE(dense2_b, h.dense2_out);
    TAKE(gru_a_dense_w, (size_t)h.dense2_out * NA3);       TAKE(gru_a_dense_b, NA3);
    TAKE(gru_b_dense_w, (size_t)h.dense2_out * NB3);       TAKE(gru_b_dense_b, NB3);
    TAKE(embed_sig, (size_t)256 * NA3); TAKE(embed_pred, (size_t)256 * NA3); TAKE(embed_exc, (size_t)256 * NA3);
    TAKE(gru_a_rbias, NA3); TAKE(gru_a_diag, NA3);
    v.gru_a_idx = (const int32_t *)p; p += h.sparse_idx_len;
    TAKE(gru_a_w, (size_t)h.sparse_nblocks * 32);
    TAKE(gru_b_bias, 2 * NB3); TAKE(gru_b_w_in, (size_t)h.gru_a * NB3); TAKE(gru_b_w_rec, (size_t)h.gru_b * NB3);
    TAKE(fc_bias, 2 * h.dual_fc_out); TAKE(fc_w, (size_t)h.dual_fc_out * 2 * h.gru_b); TAKE(fc_factor, 2 * h.dual_fc_out);
#undef TAKE
    if ((size_t)((const char *)p - blob.data()) != blob.size()) {
        dss_set_error("weight blob length %zu does not match its header", blob.size());
        return DSS_EINVAL;
    }
    return DSS_OK;
}

static int check_header(const dss_blob_header &h)
{
    if (memcmp(h.magic, DSS_BLOB_MAGIC, 8) != 0 || h.version != 1) { dss_set_error("not a DSSLPCN1 v1 blob"); return DSS_EINVAL; }
    // the kernels are specialised for the published LPCNet dimensions
    if (h.nb_features != 20 || h.nb_bands != 18 || h.embed_pitch_dim != 64 || h.pitch_max != 256 || h.conv1_out != 128 ||
        h.conv2_out != 128 || h.dense1_out != 128 || h.dense2_out != 128 || h.gru_a != DSS_GRU_A || h.gru_b != DSS_GRU_B ||
        h.dual_fc_out != DSS_FC_OUT || h.lpc_order != DSS_LPC_ORDER) {
        dss_set_error("blob dimensions differ from the LPCNet architecture this build is specialised for "
                      "(features 20, conv/dense 128, GRU A 384, GRU B 16, dual FC 256)");
        return DSS_EINVAL;
    }
    if (h.gru_a_order != DSS_GRUA_INPUT_FIRST && h.gru_a_order != DSS_GRUA_RECUR_FIRST) {
        dss_set_error("blob header: gru_a_order %d is neither 0 (input first) nor 1 (recurrent first)", h.gru_a_order);
        return DSS_EINVAL;
    }
    return DSS_OK;
}

// parse + validate a blob into a new HostModel (no lock, no device work)
static int parse_blob(const void *blob, size_t len, HostModel **out)
{
    if (!blob || len < sizeof(dss_blob_header)) { dss_set_error("blob too short"); return DSS_EINVAL; }
    HostModel *hm = new HostModel;
    memcpy(&hm->h, blob, sizeof(hm->h));
    int rc = check_header(hm->h);
    if (rc) { delete hm; return rc; }
    hm->blob.assign((const char *)blob, (const char *)blob + len);
    BlobView v;
    rc = view_blob(hm->blob, hm->h, v);
    if (rc) { delete hm; return rc; }
    // validate the sparse index (host-side shape check before any kernel trusts it)
    {
        const int groups = 3 * hm->h.gru_a / 8;
        long pos = 0, blocks = 0;
        for (int g = 0; g < groups; ++g) {
            if (pos >= hm->h.sparse_idx_len) { dss_set_error("sparse idx truncated"); delete hm; return DSS_EINVAL; }
            int cnt = v.gru_a_idx[pos++];
            if (cnt < 0 || pos + cnt > hm->h.sparse_idx_len) { dss_set_error("sparse idx corrupt"); delete hm; return DSS_EINVAL; }
            for (int j = 0; j < cnt; ++j) {
                int p = v.gru_a_idx[pos++];
                if (p < 0 || p + 4 > hm->h.gru_a || (p & 3)) { dss_set_error("sparse idx position %d invalid", p); delete hm; return DSS_EINVAL; }
            }
            blocks += cnt;
        }
        if (pos != hm->h.sparse_idx_len || blocks != hm->h.sparse_nblocks) { dss_set_error("sparse idx/blocks mismatch"); delete hm; return DSS_EINVAL; }
    }
    const int na = hm->h.gru_a, nb = hm->h.gru_b;
    const double floats = 3.0 * (3 * na) + (double)hm->h.sparse_nblocks * 32 + 3 * na + 3.0 * nb * (na + nb) + 2.0 * nb * 8 + 16;
    hm->bytes_per_sample = 4.0 * floats + 2.0 + 80.0 / 160.0;
    *out = hm;
    return DSS_OK;
}

// caller holds g_model_mu
static int load_blob_locked(const void *blob, size_t len)
{
    HostModel *hm = nullptr;
    int rc = parse_blob(blob, len, &hm);
    if (rc) return rc;
    // an earlier model stays alive exactly as long as decoder batches created from it exist (they hold its device
    // pointers); with none left it is freed here, otherwise when its last batch is destroyed
    if (g_model && g_model->refs == 0) free_model(g_model);
    g_model = hm;
    return DSS_OK;
}

extern "C" int dss_lpcnet_load_model(const void *blob, size_t len)
{
    HostModel *hm = nullptr;
    int rc = parse_blob(blob, len, &hm);                    // the slow part outside the lock
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_model_mu);
    if (g_model && g_model->refs == 0) free_model(g_model);
    g_model = hm;
    return DSS_OK;
}

static int read_file(const char *path, std::vector<char> &buf)
{
    FILE *f = fopen(path, "rb");
    if (!f) { dss_set_error("cannot open %s", path); return DSS_EINVAL; }
    fseek(f, 0, SEEK_END);
    long n = ftell(f);
    fseek(f, 0, SEEK_SET);
    buf.resize((size_t)(n > 0 ? n : 0));
    size_t got = n > 0 ? fread(buf.data(), 1, (size_t)n, f) : 0;
    fclose(f);
    if (n < 0 || got != (size_t)n) { dss_set_error("short read on %s", path); return DSS_EINVAL; }
    return DSS_OK;
}

extern "C" int dss_lpcnet_load_model_file(const char *path)
{
    std::vector<char> buf;
    int rc = read_file(path, buf);
    if (rc) return rc;
    return dss_lpcnet_load_model(buf.data(), buf.size());
}

extern "C" double dss_lpcnet_bytes_per_sample(void)
{
    std::lock_guard<std::mutex> lk(g_model_mu);
    return g_model ? g_model->bytes_per_sample : 0.0;
}

// ---- CU-resident layout of the sample-rate kernel (lpcnet_sample.hip): pure host work, no device calls -----------
struct FastLayout {
    int fast_ok = 0, zmax = 0, hmax = 0, zr_cap = 10, ext = 0, ext_tab = 0, hfloats = 0;
    std::vector<int> unit_of, unit_h, wave_nh, grp_hoff, wave_nzr, wave_nzt;
    std::vector<float> zr_w, hblk;
    std::vector<unsigned> zr_col, h_col;
};

static void build_fast_layout(const BlobView &v, int NA, FastLayout &F)
{
    const int G = NA / 8;                       // 48 row groups per gate
    std::vector<int> cnt(3 * G), start(3 * G), blk0(3 * G);
    long pos = 0, blk = 0;
    for (int g = 0; g < 3 * G; ++g) {
        cnt[g] = v.gru_a_idx[pos]; start[g] = (int)pos + 1; blk0[g] = (int)blk;
        pos += 1 + cnt[g]; blk += cnt[g];
    }
    int fast_ok = (NA == 384 && G == 48);
    int zmax = 0, hmax = 0;
    for (int g = 0; g < G; ++g) {
        zmax = std::max(zmax, std::max(cnt[g], cnt[G + g]));
        hmax = std::max(hmax, cnt[2 * G + g]);
    }
    if (hmax > DSS_HCX + DSS_HX) fast_ok = 0;
    // Two independent lane assignments, both "8 row groups per wave":
    //  * h-gate chains (LDS resident): groups sorted by h block count, so each wave's loop length (its
    //    largest group) is close to what all its groups need;
    //  * z/r chains (register resident): groups sorted by max(z, r) block count.  The 16 heaviest groups go to
    //    waves 4 and 5, whose code path carries no dual-FC weights and therefore has room for zr_cap register
    //    slots per gate; waves 0..3 run the 8-slot instantiation.  Blocks beyond a wave's register slots (models
    //    with skewed sparsity) stay in idx order behind them as "tail" records in LDS.
    // Both the h chain and the z/r block products run between barriers B and C, under the GRU B relay; waves 4
    // and 5 also run the speculation there, so they get the lightest h chains, and among waves 0..3 the heavier
    // z/r groups go with the lighter h chains.
    // The per-unit pre-activation of the h gate travels from its h lane to its z/r lane through LDS.
    std::vector<int> order_h(G), order_zr(G);
    for (int g = 0; g < G; ++g) order_h[g] = order_zr[g] = g;
    std::stable_sort(order_h.begin(), order_h.end(), [&](int a, int b2) { return cnt[2 * G + a] > cnt[2 * G + b2]; });
    std::stable_sort(order_zr.begin(), order_zr.end(), [&](int a, int b2) {
        return std::max(cnt[a], cnt[G + a]) > std::max(cnt[b2], cnt[G + b2]);
    });
    // Register slots per gate on waves 4, 5.  A model that fits the register slots as it is runs the 10-slot
    // instantiation (no spills) or, with 11 or 12 blocks in some group, the 12-slot one (22 spilled registers, ~4 %
    // slower).  Any other model runs the 10-slot layout with tails: measured faster than 12 slots + tails
    // (tools/model_fit.py), the spills cost more than the two extra tail blocks.
    const int zr17 = std::max(cnt[order_zr[16]], cnt[G + order_zr[16]]);      // heaviest group that lands on waves 0..3
    const bool plain = zmax <= DSS_ZRC && zr17 <= 8 && hmax <= DSS_HC;
    const int zr_cap = (plain && zmax > 10) ? DSS_ZRC : 10;
    int rank_wave_h[6] = {0, 1, 3, 2, 5, 4};
    static const int rank_wave_zr[6] = {4, 5, 2, 3, 1, 0};
    if (const char *e = getenv("DSS_RANK_WAVE_H")) {        // development switch (A/B timing of the h-chain assignment): a permutation of 0..5
        int p[6], seen = 0;
        if (sscanf(e, "%d,%d,%d,%d,%d,%d", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5]) == 6) {
            for (int k = 0; k < 6; ++k) if (p[k] >= 0 && p[k] < 6) seen |= 1 << p[k];
            if (seen == 63) for (int k = 0; k < 6; ++k) rank_wave_h[k] = p[k];
        }
    }
    std::vector<int> grp_h(G, 0), grp_zr(G, 0);
    std::vector<int> &unit_of = F.unit_of, &unit_h = F.unit_h, &wave_nh = F.wave_nh, &grp_hoff = F.grp_hoff, &wave_nzr = F.wave_nzr, &wave_nzt = F.wave_nzt;
    unit_of.assign(NA, 0); unit_h.assign(NA, 0); wave_nh.assign(8, 0); grp_hoff.assign(G, 0); wave_nzr.assign(8, 0); wave_nzt.assign(8, 0);
    int hfloats = 0, ext = 0;
    for (int rk = 0; rk < 6 && fast_ok; ++rk) {
        int nh = 0, nzr = 0;
        for (int q = 0; q < 8; ++q) {
            grp_h[rank_wave_h[rk] * 8 + q] = order_h[rk * 8 + q];
            grp_zr[rank_wave_zr[rk] * 8 + q] = order_zr[rk * 8 + q];
            nh = std::max(nh, cnt[2 * G + order_h[rk * 8 + q]]);
            nzr = std::max(nzr, std::max(cnt[order_zr[rk * 8 + q]], cnt[G + order_zr[rk * 8 + q]]));
        }
        const int cap = rank_wave_zr[rk] < 4 ? 8 : zr_cap;
        wave_nh[rank_wave_h[rk]] = (nh + 1) & ~1;       // the kernel tests for the end of a list every 2 slots
        wave_nzr[rank_wave_zr[rk]] = std::min((nzr + 1) & ~1, cap);
        wave_nzt[rank_wave_zr[rk]] = std::max(0, nzr - cap);
        if (nzr - cap > DSS_ZR_TAIL) fast_ok = 0;
        if (nzr > cap || nh > DSS_HC) ext = 1;
    }
    // The h-gate image: every row group's own records back to back (128 bytes = [8 rows][4 inputs] per block), no
    // padding to the wave's longest list.  A wave still runs wave_nh slots on all its lanes: a lane whose group is
    // shorter reads on into the next group's records and multiplies them by "column 96", four zeros behind the
    // state vector, so the extra terms are +-0.  One spare record goes between two groups of a wave whenever
    // they would otherwise start an even number of records apart: 8-lane groups that start 32 banks apart keep
    // the wave's ds_read_b128 of its block records conflict-free.
    int hend = 0;
    for (int wv = 0; wv < 6 && fast_ok; ++wv)
        for (int q = 0; q < 8; ++q) {
            if (q && (((hfloats - grp_hoff[wv * 8 + q - 1]) / 32) & 1) == 0) hfloats += 32;
            grp_hoff[wv * 8 + q] = hfloats;
            hfloats += cnt[2 * G + grp_h[wv * 8 + q]] * 32;
            hend = std::max(hend, grp_hoff[wv * 8 + q] + (wave_nh[wv] + 4) * 32);      // + 4: the kernel fetches two chunks of two slots ahead
        }
    hfloats = std::max(hfloats, hend);                  // the last groups' over-reads stay inside the image
    // Extended paths (models with skewed sparsity only): behind the h records, the z and r tail lists of every
    // group of the z/r assignment (same over-read convention), then a table
    //   int   tail_off[48][2]                float offset of the group's z list and of its r list
    //   uint8 tail_col[48][2][DSS_ZR_TAIL]   block column of every tail slot (96 = unused)
    //   uint8 hx_col[48][DSS_HX]             block column of h slots DSS_HCX.. of the group of the h assignment
    const int ext_tab_floats = (G * 2 * 4 + G * 2 * DSS_ZR_TAIL + G * DSS_HX) / 4 + 4;     // + 16 B: the kernel reads columns one trip ahead
    std::vector<int> tail_off(G * 2, 0);
    int ext_tab = 0;
    if (fast_ok && ext) {
        int tend = hfloats;
        for (int wv = 0; wv < 6; ++wv)
            for (int q = 0; q < 8; ++q)
                for (int gate = 0; gate < 2; ++gate) {
                    const int cap = wv < 4 ? 8 : zr_cap, n = cnt[gate * G + grp_zr[wv * 8 + q]];
                    tail_off[(wv * 8 + q) * 2 + gate] = hfloats;
                    tend = std::max(tend, hfloats + wave_nzt[wv] * 32);
                    hfloats += std::max(0, n - cap) * 32;
                }
        hfloats = std::max(hfloats, tend);
        ext_tab = hfloats;
        hfloats += ext_tab_floats;
    }
    if ((size_t)hfloats * sizeof(float) > DSS_HBLK_BYTES) fast_ok = 0;
    std::vector<float> &zr_w = F.zr_w, &hblk = F.hblk;
    std::vector<unsigned> &zr_col = F.zr_col, &h_col = F.h_col;
    zr_w.assign((size_t)2 * DSS_ZRC * 4 * NA, 0.f); hblk.assign((size_t)std::max(hfloats, 4), 0.f);
    zr_col.assign((size_t)(2 * DSS_ZRC / 4) * NA, 0u); h_col.assign((size_t)(DSS_HCX / 4) * NA, 0u);
    if (fast_ok)
        for (int tid = 0; tid < NA; ++tid) {
            const int wv = tid / 64, l = tid & 63, q = l / 8, r = l & 7;
            {
                const int grp = grp_zr[wv * 8 + q];
                unit_of[tid] = grp * 8 + r;
                const int cap = wv < 4 ? 8 : zr_cap;
                for (int gate = 0; gate < 2; ++gate) {
                    const int g = gate * G + grp;
                    for (int sl = 0; sl < std::min(cnt[g], cap); ++sl) {
                        const int s2 = gate * DSS_ZRC + sl;
                        const float *wb = v.gru_a_w + (size_t)(blk0[g] + sl) * 32;
                        for (int k = 0; k < 4; ++k) zr_w[((size_t)s2 * 4 + k) * NA + tid] = wb[k * 8 + r];
                        zr_col[(size_t)(s2 >> 2) * NA + tid] |= (unsigned)(v.gru_a_idx[start[g] + sl] / 4) << (8 * (s2 & 3));
                    }
                    for (int sl = cap; sl < cnt[g]; ++sl) {              // tail: LDS records, columns in the table
                        const float *wb = v.gru_a_w + (size_t)(blk0[g] + sl) * 32;
                        float *rec = hblk.data() + tail_off[(wv * 8 + q) * 2 + gate] + (size_t)(sl - cap) * 32 + r * 4;
                        for (int k = 0; k < 4; ++k) rec[k] = wb[k * 8 + r];
                    }
                }
            }
            {
                const int grp = grp_h[wv * 8 + q], g = 2 * G + grp;
                unit_h[tid] = grp * 8 + r;
                for (int sl = 0; sl < cnt[g]; ++sl) {
                    const float *wb = v.gru_a_w + (size_t)(blk0[g] + sl) * 32;
                    float *rec = hblk.data() + grp_hoff[wv * 8 + q] + (size_t)sl * 32 + r * 4;
                    for (int k = 0; k < 4; ++k) rec[k] = wb[k * 8 + r];
                    if (sl < DSS_HCX) h_col[(size_t)(sl >> 2) * NA + tid] |= (unsigned)(v.gru_a_idx[start[g] + sl] / 4) << (8 * (sl & 3));
                }
                for (int sl = cnt[g]; sl < DSS_HCX; ++sl) h_col[(size_t)(sl >> 2) * NA + tid] |= 96u << (8 * (sl & 3));
            }
        }
    if (fast_ok && ext) {
        int *toff = reinterpret_cast<int *>(hblk.data() + ext_tab);
        unsigned char *tcol = reinterpret_cast<unsigned char *>(toff + G * 2);
        unsigned char *hxc = tcol + (size_t)G * 2 * DSS_ZR_TAIL;
        memset(tcol, 96, (size_t)G * 2 * DSS_ZR_TAIL + (size_t)G * DSS_HX);
        for (int wv = 0; wv < 6; ++wv)
            for (int q = 0; q < 8; ++q) {
                const int cap = wv < 4 ? 8 : zr_cap;
                for (int gate = 0; gate < 2; ++gate) {
                    const int g = gate * G + grp_zr[wv * 8 + q];
                    toff[(wv * 8 + q) * 2 + gate] = tail_off[(wv * 8 + q) * 2 + gate];
                    for (int sl = cap; sl < cnt[g]; ++sl)
                        tcol[((size_t)(wv * 8 + q) * 2 + gate) * DSS_ZR_TAIL + (sl - cap)] = (unsigned char)(v.gru_a_idx[start[g] + sl] / 4);
                }
                const int gh = 2 * G + grp_h[wv * 8 + q];
                for (int sl = DSS_HCX; sl < cnt[gh]; ++sl)
                    hxc[(size_t)(wv * 8 + q) * DSS_HX + (sl - DSS_HCX)] = (unsigned char)(v.gru_a_idx[start[gh] + sl] / 4);
            }
    }
    F.fast_ok = fast_ok; F.zmax = zmax; F.hmax = hmax; F.zr_cap = zr_cap; F.ext = fast_ok ? ext : 0; F.ext_tab = ext_tab; F.hfloats = hfloats;
}

static int upload_model(HostModel *hm, int device, DssModelDev &m)
{
    DssDevBlocks &mem = hm->dev_blocks[device];
    BlobView v;
    int rc = view_blob(hm->blob, hm->h, v);
    if (rc) return rc;
    const dss_blob_header &h = hm->h;
    memset(&m, 0, sizeof(m));
    m.h = h;
    const int fin = h.nb_features + h.embed_pitch_dim, NA = h.gru_a, NA3 = 3 * NA, NB3 = 3 * h.gru_b;
#define UP(field, src, count) do { float *d; rc = mem.upload<float>(src, (size_t)(count), &d); if (rc) return rc; m.field = d; } while (0)
    UP(embed_pitch, v.embed_pitch, (size_t)h.pitch_max * h.embed_pitch_dim);
    UP(conv1_w, v.conv1_w, (size_t)3 * fin * 128);   UP(conv1_b, v.conv1_b, 128);
    UP(conv2_w, v.conv2_w, (size_t)3 * 128 * 128);   UP(conv2_b, v.conv2_b, 128);
    UP(dense1_w, v.dense1_w, 128 * 128);             UP(dense1_b, v.dense1_b, 128);
    UP(dense2_w, v.dense2_w, 128 * 128);             UP(dense2_b, v.dense2_b, 128);
    UP(gru_a_dense_w, v.gru_a_dense_w, (size_t)128 * NA3);  UP(gru_a_dense_b, v.gru_a_dense_b, NA3);
    UP(gru_b_dense_w, v.gru_b_dense_w, (size_t)128 * NB3);  UP(gru_b_dense_b, v.gru_b_dense_b, NB3);
    UP(embed_sig, v.embed_sig, (size_t)256 * NA3);
    UP(embed_pred, v.embed_pred, (size_t)256 * NA3);
    UP(embed_exc, v.embed_exc, (size_t)256 * NA3);
    UP(gru_a_rbias, v.gru_a_rbias, NA3);
    UP(gru_a_diag, v.gru_a_diag, NA3);
    UP(gru_b_bias, v.gru_b_bias, 2 * NB3);
    UP(gru_b_w_in, v.gru_b_w_in, (size_t)NA * NB3);
    UP(gru_b_w_rec, v.gru_b_w_rec, (size_t)h.gru_b * NB3);
    UP(fc_bias, v.fc_bias, 2 * h.dual_fc_out);
    UP(fc_w, v.fc_w, (size_t)h.dual_fc_out * 2 * h.gru_b);
    UP(fc_factor, v.fc_factor, 2 * h.dual_fc_out);

    // ---- sparse GRU A: per gate, per unit, a padded list of (pos, 4 weights) slots in idx order ----------
    {
        const int groups_per_gate = NA / 8;
        std::vector<int> grp_start(3 * groups_per_gate), grp_cnt(3 * groups_per_gate), grp_blk(3 * groups_per_gate);
        long pos = 0, blk = 0;
        for (int g = 0; g < 3 * groups_per_gate; ++g) {
            grp_cnt[g] = v.gru_a_idx[pos];
            grp_start[g] = (int)pos + 1;
            grp_blk[g] = (int)blk;
            pos += 1 + grp_cnt[g];
            blk += grp_cnt[g];
        }
        int zr_slots = 0;
        for (int g = 0; g < 2 * groups_per_gate; ++g) zr_slots = std::max(zr_slots, grp_cnt[g]);
        for (int gate = 0; gate < 3; ++gate) {
            int slots = 0;
            for (int g = 0; g < groups_per_gate; ++g) slots = std::max(slots, grp_cnt[gate * groups_per_gate + g]);
            // the generic kernel keeps 16 blocks in flight, unconditionally: z and r lists share one length (multiple of 8),
            // the h list is a multiple of 16; the padding is zero blocks at input 0
            slots = gate < 2 ? ((std::max(zr_slots, 1) + 7) & ~7) : ((std::max(slots, 1) + 15) & ~15);
            std::vector<int> pos4((size_t)slots * NA, 0);
            std::vector<float> w((size_t)slots * 4 * NA, 0.f);
            for (int unit = 0; unit < NA; ++unit) {
                const int g = gate * groups_per_gate + unit / 8, r = unit & 7;
                for (int sl = 0; sl < grp_cnt[g]; ++sl) {
                    pos4[(size_t)sl * NA + unit] = v.gru_a_idx[grp_start[g] + sl] * 4;
                    const float *wb = v.gru_a_w + (size_t)(grp_blk[g] + sl) * 32;
                    for (int k = 0; k < 4; ++k) w[((size_t)sl * 4 + k) * NA + unit] = wb[k * 8 + r];
                }
            }
            int *dpos; float *dw;
            rc = mem.upload<int>(pos4.data(), pos4.size(), &dpos); if (rc) return rc;
            rc = mem.upload<float>(w.data(), w.size(), &dw); if (rc) return rc;
            m.gate[gate].slots = slots; m.gate[gate].pos4 = dpos; m.gate[gate].w = dw;
        }
    }
    // ---- CU-resident layout of the sample-rate kernel (lpcnet_sample.hip) ---------------------------------
    {
        FastLayout F;
        build_fast_layout(v, NA, F);
        m.fast_ok = F.fast_ok; m.nzr_max = (F.zmax + 1) & ~1; m.zr_cap = F.zr_cap; m.hmax = F.hmax;
        m.ext = F.ext; m.ext_tab = F.ext_tab; m.hblk_floats = F.hfloats;
        int *di; float *df; unsigned *du;
        rc = mem.upload<int>(F.unit_of.data(), F.unit_of.size(), &di); if (rc) return rc; m.unit_of = di;
        {   // embedding rows permuted into lane order, the three gates of a lane's unit side by side
            const float *tabs[3] = {v.embed_sig, v.embed_pred, v.embed_exc};
            std::vector<float> perm((size_t)256 * NA * 3);
            for (int t = 0; t < 3; ++t) {
                for (int idx = 0; idx < 256; ++idx)
                    for (int tid = 0; tid < NA; ++tid)
                        for (int g = 0; g < 3; ++g)
                            perm[((size_t)idx * NA + tid) * 3 + g] = tabs[t][(size_t)idx * 3 * NA + (size_t)g * NA + F.unit_of[tid]];
                rc = mem.upload<float>(perm.data(), perm.size(), &df); if (rc) return rc; m.embed_lane[t] = df;
            }
        }
        rc = mem.upload<int>(F.unit_h.data(), F.unit_h.size(), &di); if (rc) return rc; m.unit_h = di;
        rc = mem.upload<int>(F.wave_nh.data(), F.wave_nh.size(), &di); if (rc) return rc; m.wave_nh = di;
        rc = mem.upload<int>(F.grp_hoff.data(), F.grp_hoff.size(), &di); if (rc) return rc; m.grp_hoff = di;
        rc = mem.upload<int>(F.wave_nzr.data(), F.wave_nzr.size(), &di); if (rc) return rc; m.wave_nzr = di;
        rc = mem.upload<int>(F.wave_nzt.data(), F.wave_nzt.size(), &di); if (rc) return rc; m.wave_nzt = di;
        rc = mem.upload<float>(F.zr_w.data(), F.zr_w.size(), &df); if (rc) return rc; m.zr_w = df;
        rc = mem.upload<unsigned>(F.zr_col.data(), F.zr_col.size(), &du); if (rc) return rc; m.zr_col = du;
        rc = mem.upload<unsigned>(F.h_col.data(), F.h_col.size(), &du); if (rc) return rc; m.h_col = du;
        rc = mem.upload<float>(F.hblk.data(), F.hblk.size(), &df); if (rc) return rc; m.hblk = df;
        // GRU B input weights for the two relay waves, j-major with lane = row: [384][64]
        std::vector<float> gbl((size_t)NA * 64, 0.f);
        for (int j = 0; j < NA; ++j)
            for (int row = 0; row < NB3; ++row) gbl[(size_t)j * 64 + row] = v.gru_b_w_in[(size_t)j * NB3 + row];
        rc = mem.upload<float>(gbl.data(), gbl.size(), &df); if (rc) return rc; m.gb_w_lane = df;
        // ... and four inputs of a lane side by side, for the pair kernel's relay waves, which stream them from L2
        std::vector<float> gbq((size_t)NA * 64, 0.f);
        for (int j = 0; j < NA; ++j)
            for (int row = 0; row < NB3; ++row) gbq[((size_t)(j / 4) * 64 + row) * 4 + (j & 3)] = v.gru_b_w_in[(size_t)j * NB3 + row];
        rc = mem.upload<float>(gbq.data(), gbq.size(), &df); if (rc) return rc; m.gb_w_quad = df;
        // dual-FC weights for the pair kernel, whose dual-FC waves load their node's 32 weights every sample instead of
        // holding them in registers: [k 8][node 256][4] = (layer 0, layer 1) weights of inputs 2k and 2k+1, so that load k
        // of a wave reads 1 KB of consecutive bytes
        std::vector<float> fcp((size_t)DSS_FC_OUT * DSS_GRU_B * 2, 0.f);
        for (int node = 0; node < DSS_FC_OUT; ++node)
            for (int j = 0; j < DSS_GRU_B; ++j) {
                const size_t o = ((size_t)(j / 2) * DSS_FC_OUT + node) * 4 + (j & 1) * 2;
                fcp[o + 0] = v.fc_w[(size_t)node * 2 * DSS_GRU_B + j];
                fcp[o + 1] = v.fc_w[(size_t)node * 2 * DSS_GRU_B + DSS_GRU_B + j];
            }
        rc = mem.upload<float>(fcp.data(), fcp.size(), &df); if (rc) return rc; m.fc_w_pair = df;
    }
    // ---- derived tables (host libm, exactly as xiph builds them at run time) ---------------------------
    {
        float tansig[DSS_TANSIG_Y + 201] = {0}, logit[256], u2l[256], dct[18 * 18], costab[320], ia[160], ib[160];
        int iband[160];
        double lagw[17];
        dss_tansig_tables(tansig);
        for (int i = 0; i < 256; ++i) {                                                              // lpcnet_init()
            float prob = .025 + .95 * i / 255.;
            logit[i] = -log((1 - prob) / prob);
            u2l[i] = host_ulaw2lin((float)i);
        }
        for (int i = 0; i < 18; ++i)                                                                  // freq.c check_init()
            for (int j = 0; j < 18; ++j) {
                dct[i * 18 + j] = cos((i + .5) * j * M_PI / 18);
                if (j == 0) dct[i * 18 + j] *= sqrt(.5);
            }
        for (int i = 0; i < 320; ++i) costab[i] = (float)cos(2. * M_PI * i / 320);
        static const int eband5ms[18] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 14, 16, 20, 24, 28, 34, 40};
        for (int i = 0; i < 17; ++i) {                                                                // interp_band_gain()
            const int band_size = (eband5ms[i + 1] - eband5ms[i]) * 4;
            for (int j = 0; j < band_size; ++j) {
                const float frac = (float)j / band_size;
                ia[eband5ms[i] * 4 + j] = 1 - frac;
                ib[eband5ms[i] * 4 + j] = frac;
                iband[eband5ms[i] * 4 + j] = i;
            }
        }
        for (int i = 0; i < 17; ++i) lagw[i] = (1 - 6e-5 * i * i);
        float *d; int *di; double *dd;
        rc = mem.upload<float>(tansig, DSS_TANSIG_Y + 201, &d); if (rc) return rc; m.tansig = d;
        rc = mem.upload<float>(logit, 256, &d); if (rc) return rc; m.logit_table = d;
        rc = mem.upload<float>(u2l, 256, &d); if (rc) return rc; m.ulaw2lin = d;
        rc = mem.upload<float>(dct, 324, &d); if (rc) return rc; m.dct_table = d;
        rc = mem.upload<float>(costab, 320, &d); if (rc) return rc; m.cos_table = d;
        {
            std::vector<float> ckl((size_t)160 * 17);
            for (int k = 0; k < 160; ++k)
                for (int lag = 0; lag < 17; ++lag) ckl[(size_t)k * 17 + lag] = costab[(k * lag) % 320];
            rc = mem.upload<float>(ckl.data(), ckl.size(), &d); if (rc) return rc; m.cos_kl = d;
        }
        rc = mem.upload<float>(ia, 160, &d); if (rc) return rc; m.interp_a = d;
        rc = mem.upload<float>(ib, 160, &d); if (rc) return rc; m.interp_b = d;
        rc = mem.upload<int>(iband, 160, &di); if (rc) return rc; m.interp_band = di;
        rc = mem.upload<double>(lagw, 17, &dd); if (rc) return rc; m.lag_window = dd;
    }
#undef UP
    return DSS_OK;
}

// Returns the current model and its copy on the calling thread's device.  With acquire set, the model's reference count
// is taken while g_model_mu is still held, so a concurrent dss_lpcnet_load_model() cannot free it in between; the caller
// then owns one reference (release_model()).
int get_model(HostModel **out_hm, const DssModelDev **out, bool acquire)
{
    int rc = dss_ensure_device();
    if (rc) return rc;
    int dev = 0;
    DSS_HIP_CHECK(hipGetDevice(&dev));
    std::unique_lock<std::mutex> lk(g_model_mu);
    if (!g_model) {
        const char *path = getenv("DSS_LPCNET_WEIGHTS");
        if (!path) { dss_set_error("no LPCNet weights: call dss_lpcnet_load_model() or set DSS_LPCNET_WEIGHTS"); return DSS_ENOMODEL; }
        std::vector<char> buf;
        rc = read_file(path, buf);
        if (rc) return rc;
        rc = load_blob_locked(buf.data(), buf.size());
        if (rc) return rc;
    }
    HostModel *hm = g_model;
    const int ndev = dss_device_count();
    if ((int)hm->dev.size() < ndev) { hm->dev.resize(ndev); hm->dev_ready.resize(ndev, 0); hm->dev_blocks.resize(ndev); }
    if (!hm->dev_ready[dev]) {
        rc = upload_model(hm, dev, hm->dev[dev]);
        if (rc) return rc;
        hm->dev_ready[dev] = 1;
    }
    if (acquire) hm->refs++;
    *out_hm = hm;
    *out = &hm->dev[dev];
    return DSS_OK;
}

void release_model(HostModel *hm)
{
    std::lock_guard<std::mutex> lk(g_model_mu);
    if (hm && --hm->refs == 0 && hm != g_model) free_model(hm);     // a superseded model dies with its last user
}

extern "C" int dss_lpcnet_model_info(int *fast_path, int *zr_slots_max, int *h_slots_max, int *h_lds_bytes, int *gru_a_order)
{
    HostModel *hm; const DssModelDev *m;
    int rc = get_model(&hm, &m, true);
    if (rc) return rc;
    int hmax = 0;
    // recomputed from the blob (the device struct keeps only what the kernels need)
    {
        BlobView v;
        if (view_blob(hm->blob, hm->h, v)) { release_model(hm); return DSS_EINVAL; }
        const int G = hm->h.gru_a / 8;
        long pos = 0;
        for (int g = 0; g < 3 * G; ++g) { const int c = v.gru_a_idx[pos]; if (g >= 2 * G) hmax = std::max(hmax, c); pos += 1 + c; }
    }
    if (fast_path) *fast_path = m->fast_ok ? (m->ext ? 2 : 1) : 0;
    if (zr_slots_max) *zr_slots_max = m->nzr_max;
    if (h_slots_max) *h_slots_max = hmax;
    if (h_lds_bytes) *h_lds_bytes = m->hblk_floats * 4;
    if (gru_a_order) *gru_a_order = hm->h.gru_a_order;
    release_model(hm);
    return DSS_OK;
}

// Host-only: the activation table pair exactly as load_model uploads it, out[0..201) = y, out[DSS_TANSIG_Y .. +201) = 1 - y*y
// (tests/test_cpu_tansig_pairs.py compares the second half with numpy's two fp32 operations).
extern "C" int dss_selftest_tansig_table(float *out, int n)
{
    if (!out || n != DSS_TANSIG_Y + 201) { dss_set_error("dss_selftest_tansig_table: out must hold %d floats", DSS_TANSIG_Y + 201); return DSS_EINVAL; }
    memset(out, 0, sizeof(float) * (size_t)n);
    dss_tansig_tables(out);
    return DSS_OK;
}

extern "C" int dss_selftest_tansig(int which, unsigned start_bits, unsigned long long n, unsigned long long *res)
{
    if (!res || which < 0 || which > 2 || n == 0 || n > (1ull << 32)) { dss_set_error("dss_selftest_tansig: bad arguments"); return DSS_EINVAL; }
    int rc = dss_ensure_device();
    if (rc) return rc;
    float tab[DSS_TANSIG_Y + 201] = {0};
    dss_tansig_tables(tab);
    const unsigned long long init[2] = {0, ~0ull};
    DssDevBlocks mem;
    float *dtab = nullptr;
    unsigned long long *dres = nullptr;
    rc = mem.upload<float>(tab, DSS_TANSIG_Y + 201, &dtab) | mem.upload<unsigned long long>(init, 2, &dres);
    if (!rc) rc = dss_launch_tansig_selftest(dtab, which, start_bits, n, dres, 0);
    if (!rc && hipMemcpy(res, dres, sizeof(init), hipMemcpyDeviceToHost) != hipSuccess) rc = DSS_ENODEV;
    mem.free_all();
    return rc;
}

// Host-only check of build_fast_layout(): walks every lane's z, r and h lists through the arrays exactly as the kernel
// indexes them (register slots, tail records, long-list columns, over-reads) and compares the blocks it would multiply, in
// order, with the row's blocks in the blob.  Needs no GPU (tests/test_cpu_layout.py).
extern "C" int dss_selftest_fast_layout(const void *blob, size_t len, int *info)
{
    if (!blob || !info || len < sizeof(dss_blob_header)) { dss_set_error("dss_selftest_fast_layout: bad arguments"); return DSS_EINVAL; }
    dss_blob_header h;
    memcpy(&h, blob, sizeof(h));
    int rc = check_header(h);
    if (rc) return rc;
    std::vector<char> copy((const char *)blob, (const char *)blob + len);
    BlobView v;
    rc = view_blob(copy, h, v);
    if (rc) return rc;
    const int NA = h.gru_a, G = NA / 8;
    FastLayout F;
    build_fast_layout(v, NA, F);
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[0] = F.fast_ok ? (F.ext ? 2 : 1) : 0;
    info[1] = F.zmax; info[2] = F.hmax; info[3] = F.hfloats * 4; info[4] = F.zr_cap;
    if (!F.fast_ok) return DSS_OK;
    std::vector<int> cnt(3 * G), start(3 * G), blk0(3 * G);
    long pos = 0, blk = 0;
    for (int g = 0; g < 3 * G; ++g) { cnt[g] = v.gru_a_idx[pos]; start[g] = (int)pos + 1; blk0[g] = (int)blk; pos += 1 + cnt[g]; blk += cnt[g]; }
    int mismatches = 0, oob = 0, tails = 0;
    const int rec_end = F.ext ? F.ext_tab : F.hfloats;                 // records may be read up to here
    const int *toff = reinterpret_cast<const int *>(F.hblk.data() + F.ext_tab);
    const unsigned char *tcol = reinterpret_cast<const unsigned char *>(toff + G * 2);
    const unsigned char *hxc = tcol + (size_t)G * 2 * DSS_ZR_TAIL;
    std::vector<int> seen_zr(NA, 0), seen_h(NA, 0);
    struct Blk { int col; float w[4]; };
    auto compare = [&](const std::vector<Blk> &got, int g, int r) {
        // drop the terms that are +-0 by construction: zero column, or an all-zero padded register slot
        std::vector<Blk> eff;
        for (const Blk &b : got) {
            if (b.col == 96) continue;
            if (b.w[0] == 0.f && b.w[1] == 0.f && b.w[2] == 0.f && b.w[3] == 0.f) continue;
            eff.push_back(b);
        }
        if ((int)eff.size() != cnt[g]) { ++mismatches; return; }
        for (int sl = 0; sl < cnt[g]; ++sl) {
            const float *wb = v.gru_a_w + (size_t)(blk0[g] + sl) * 32;
            if (eff[sl].col != v.gru_a_idx[start[g] + sl] / 4) { ++mismatches; return; }
            for (int k = 0; k < 4; ++k) if (eff[sl].w[k] != wb[k * 8 + r]) { ++mismatches; return; }
        }
    };
    for (int tid = 0; tid < NA; ++tid) {
        const int wave = tid / 64, lane = tid & 63, grp2 = tid >> 3;
        {   // z and r lists of unit_of[tid]
            const int unit = F.unit_of[tid];
            if (unit < 0 || unit >= NA) { ++mismatches; continue; }
            ++seen_zr[unit];
            const int zreg = wave < 4 ? 8 : F.zr_cap, nzr = F.wave_nzr[wave], nzt = F.ext ? F.wave_nzt[wave] : 0;
            if (nzr > zreg || (!F.ext && F.wave_nzt[wave])) ++mismatches;
            for (int gate = 0; gate < 2; ++gate) {
                std::vector<Blk> got;
                for (int sl = 0; sl < nzr; ++sl) {
                    const int s2 = gate * DSS_ZRC + sl;
                    Blk b;
                    b.col = (F.zr_col[(size_t)(s2 >> 2) * NA + tid] >> (8 * (s2 & 3))) & 0xFF;
                    for (int k = 0; k < 4; ++k) b.w[k] = F.zr_w[((size_t)s2 * 4 + k) * NA + tid];
                    got.push_back(b);
                }
                for (int sl = 0; sl < nzt; ++sl) {
                    const int off = toff[grp2 * 2 + gate] + sl * 32 + (lane & 7) * 4;
                    if (off < 0 || off + 4 > rec_end) { ++oob; continue; }
                    Blk b;
                    b.col = tcol[((size_t)grp2 * 2 + gate) * DSS_ZR_TAIL + sl];
                    for (int k = 0; k < 4; ++k) b.w[k] = F.hblk[off + k];
                    if (b.col != 96) ++tails;
                    got.push_back(b);
                }
                compare(got, gate * G + unit / 8, unit & 7);
            }
        }
        {   // h list of unit_h[tid]
            const int unit = F.unit_h[tid];
            if (unit < 0 || unit >= NA) { ++mismatches; continue; }
            ++seen_h[unit];
            const int nh = F.wave_nh[wave], hreg = F.ext ? DSS_HCX : DSS_HC;
            if (!F.ext && nh > DSS_HC) ++mismatches;
            std::vector<Blk> got;
            for (int sl = 0; sl < nh; ++sl) {
                const int off = F.grp_hoff[grp2] + sl * 32 + (lane & 7) * 4;
                if (off < 0 || off + 4 > rec_end) { ++oob; continue; }
                Blk b;
                b.col = sl < hreg ? (int)((F.h_col[(size_t)(sl >> 2) * NA + tid] >> (8 * (sl & 3))) & 0xFF)
                                  : (int)hxc[(size_t)grp2 * DSS_HX + (sl - DSS_HCX)];
                for (int k = 0; k < 4; ++k) b.w[k] = F.hblk[off + k];
                got.push_back(b);
            }
            compare(got, 2 * G + unit / 8, unit & 7);
            // the kernel fetches two chunks of two slots ahead of the one it sums: those reads stay inside the image
            if (F.grp_hoff[grp2] + (nh + 4) * 32 > F.hfloats) ++oob;
        }
    }
    for (int u = 0; u < NA; ++u) if (seen_zr[u] != 1 || seen_h[u] != 1) ++mismatches;
    if ((size_t)F.hfloats * sizeof(float) > DSS_HBLK_BYTES) ++mismatches;
    info[5] = tails / 8;             // every tail block is seen by the 8 lanes of its row group
    info[6] = mismatches; info[7] = oob;
    return DSS_OK;
}
