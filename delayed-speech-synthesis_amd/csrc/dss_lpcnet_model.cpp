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
#include "lpc_tables.h"

struct BlobView {
    const float *embed_pitch, *conv1_w, *conv1_b, *conv2_w, *conv2_b, *dense1_w, *dense1_b, *dense2_w, *dense2_b;
    const float *gru_a_dense_w, *gru_a_dense_b, *gru_b_dense_w, *gru_b_dense_b, *embed_sig, *embed_pred, *embed_exc;
    const float *gru_a_rbias, *gru_a_diag;
    const int32_t *gru_a_idx;
    const float *gru_a_w, *gru_b_bias, *gru_b_w_in, *gru_b_w_rec, *fc_bias, *fc_w, *fc_factor;
};

// GRU A's sparse index, parsed once (parse_sparse): row group g = gate * G + group (3 gates x G = 48 groups of 8 rows) has cnt[g]
// 8x4 blocks, its block columns stand at idx[start[g] ..] and its first block record is blk0[g].
struct SparseGroups {
    int NA = 0, G = 0;                     // GRU A units, row groups per gate
    std::vector<int> cnt, start, blk0;     // [3 * G]
    int zmax = 0, hmax = 0;                // longest z or r list, longest h list
    const int32_t *idx = nullptr;          // the blob's own lists (the blob outlives this struct's users)
    const float *w = nullptr;

    int pos(int g, int sl) const { return idx[start[g] + sl]; }        // first input of block sl of group g
    int col(int g, int sl) const { return pos(g, sl) / 4; }            // ... as a block column
    // row r of block sl of group g, a record of [4 inputs][8 rows]: its four weights to dst[0], dst[stride], ...
    void block_row(int g, int sl, int r, float *dst, size_t stride = 1) const { for (int k = 0; k < 4; ++k) dst[k * stride] = w[(size_t)(blk0[g] + sl) * 32 + k * 8 + r]; }
};

// ---- model: blob -> device -------------------------------------------------------------------------------------------
struct HostModel {
    std::vector<char> blob;
    dss_blob_header h;
    BlobView v;                        // into blob
    SparseGroups groups;
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

// The one walk over GRU A's sparse index, and its validation (host-side shape check before any kernel trusts it).
static int parse_sparse(const BlobView &v, const dss_blob_header &h, SparseGroups &S)
{
    S.NA = h.gru_a; S.G = h.gru_a / 8; S.idx = v.gru_a_idx; S.w = v.gru_a_w; S.zmax = S.hmax = 0;
    S.cnt.assign(3 * S.G, 0); S.start.assign(3 * S.G, 0); S.blk0.assign(3 * S.G, 0);
    long pos = 0, blocks = 0;
    for (int g = 0; g < 3 * S.G; ++g) {
        if (pos >= h.sparse_idx_len) { dss_set_error("sparse idx truncated"); return DSS_EINVAL; }
        const int cnt = v.gru_a_idx[pos++];
        if (cnt < 0 || pos + cnt > h.sparse_idx_len) { dss_set_error("sparse idx corrupt"); return DSS_EINVAL; }
        S.cnt[g] = cnt; S.start[g] = (int)pos; S.blk0[g] = (int)blocks;
        for (int j = 0; j < cnt; ++j) {
            const int p = v.gru_a_idx[pos++];
            if (p < 0 || p + 4 > h.gru_a || (p & 3)) { dss_set_error("sparse idx position %d invalid", p); return DSS_EINVAL; }
        }
        blocks += cnt;
        int &longest = g < 2 * S.G ? S.zmax : S.hmax;
        longest = std::max(longest, cnt);
    }
    if (pos != h.sparse_idx_len || blocks != h.sparse_nblocks) { dss_set_error("sparse idx/blocks mismatch"); return DSS_EINVAL; }
    return DSS_OK;
}

// header, view and sparse groups of a blob held in `bytes` (which v and S point into)
static int parse_views(const std::vector<char> &bytes, dss_blob_header &h, BlobView &v, SparseGroups &S)
{
    if (bytes.size() < sizeof(dss_blob_header)) { dss_set_error("blob too short"); return DSS_EINVAL; }
    memcpy(&h, bytes.data(), sizeof(h));
    int rc = check_header(h);
    if (!rc) rc = view_blob(bytes, h, v);
    if (!rc) rc = parse_sparse(v, h, S);
    return rc;
}

// parse + validate a blob into a new HostModel (no lock, no device work)
static int parse_blob(const void *blob, size_t len, HostModel **out)
{
    if (!blob) { dss_set_error("blob too short"); return DSS_EINVAL; }
    HostModel *hm = new HostModel;
    hm->blob.assign((const char *)blob, (const char *)blob + len);
    const int rc = parse_views(hm->blob, hm->h, hm->v, hm->groups);
    if (rc) { delete hm; return rc; }
    const int na = hm->h.gru_a, nb = hm->h.gru_b;
    const double floats = 3.0 * (3 * na) + (double)hm->h.sparse_nblocks * 32 + 3 * na + 3.0 * nb * (na + nb) + 2.0 * nb * 8 + 16;
    hm->bytes_per_sample = 4.0 * floats + 2.0 + 80.0 / 160.0;
    *out = hm;
    return DSS_OK;
}

// makes a parsed model the current one (caller holds g_model_mu)
static void install_locked(HostModel *hm)
{
    // an earlier model stays alive exactly as long as decoder batches created from it exist (they hold its device
    // pointers); with none left it is freed here, otherwise when its last batch is destroyed
    if (g_model && g_model->refs == 0) free_model(g_model);
    g_model = hm;
}

extern "C" int dss_lpcnet_load_model(const void *blob, size_t len)
{
    HostModel *hm = nullptr;
    int rc = parse_blob(blob, len, &hm);                    // the slow part outside the lock
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_model_mu);
    install_locked(hm);
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

// ---- the generic kernel's lists (lpcnet_sample_generic.hip) -----------------------------------------------------------
// per gate, per unit, a padded list of (pos, 4 weights) slots in idx order
struct GenericGate { int slots; std::vector<int> pos4; std::vector<float> w; };      // pos4 [slots][NA], w [slots][4][NA]

static GenericGate build_generic_gate(const SparseGroups &S, int gate)
{
    const int NA = S.NA;
    GenericGate L;
    // the generic kernel keeps 16 blocks in flight, unconditionally: z and r lists share one length (multiple of 8),
    // the h list is a multiple of 16; the padding is zero blocks at input 0
    L.slots = gate < 2 ? ((std::max(S.zmax, 1) + 7) & ~7) : ((std::max(S.hmax, 1) + 15) & ~15);
    L.pos4.assign((size_t)L.slots * NA, 0); L.w.assign((size_t)L.slots * 4 * NA, 0.f);
    for (int unit = 0; unit < NA; ++unit) {
        const int g = gate * S.G + unit / 8, r = unit & 7;
        for (int sl = 0; sl < S.cnt[g]; ++sl) {
            L.pos4[(size_t)sl * NA + unit] = S.pos(g, sl) * 4;
            S.block_row(g, sl, r, &L.w[(size_t)sl * 4 * NA + unit], NA);
        }
    }
    return L;
}

// ---- CU-resident layout of the sample-rate kernel (lpcnet_sample.hip): pure host work, no device calls -----------
struct FastLayout {
    int fast_ok = 0, zmax = 0, hmax = 0, zr_cap = 10, ext = 0, ext_tab = 0, hfloats = 0;
    std::vector<int> grp_h, grp_zr;      // [48] row group whose h chain / whose z and r chains run at a place (see each_place)
    std::vector<int> tail_off;           // [48][2] float offset of the place's z and r tail records inside hblk
    std::vector<int> unit_of, unit_h, wave_nh, grp_hoff, wave_nzr, wave_nzt;
    std::vector<float> zr_w, hblk;
    std::vector<unsigned> zr_col, h_col;

    // register slots per gate of a wave: waves 0..3 hold the dual-FC weights and run the 8-slot instantiation
    int zr_regs(int wave) const { return wave < 4 ? 8 : zr_cap; }
};

// The 48 places of the GRU A waves: wave 0..5 x q 0..7, place = wave * 8 + q = thread id / 8; its lanes are threads place * 8 + row.
template <typename Fn>
static void each_place(Fn f) { for (int wv = 0; wv < 6; ++wv) for (int q = 0; q < 8; ++q) f(wv, q, wv * 8 + q); }

// Which wave runs the k-th heaviest eight h chains.  DSS_RANK_WAVE_H is a development switch (A/B timing of the h-chain
// assignment): a permutation of 0..5.
static void rank_wave_h_order(int rank_wave_h[6])
{
    int p[6] = {0, 1, 3, 2, 5, 4}, seen = 0;
    memcpy(rank_wave_h, p, sizeof(p));
    const char *e = getenv("DSS_RANK_WAVE_H");
    if (!e || sscanf(e, "%d,%d,%d,%d,%d,%d", &p[0], &p[1], &p[2], &p[3], &p[4], &p[5]) != 6) return;
    for (int k = 0; k < 6; ++k) if (p[k] >= 0 && p[k] < 6) seen |= 1 << p[k];
    if (seen == 63) memcpy(rank_wave_h, p, sizeof(p));
}

// Stage 1, assignment: which row group runs where, the register capacity, every wave's slot counts, fast_ok / ext.
static void layout_assign(const SparseGroups &S, FastLayout &F)
{
    const int G = S.G;
    const std::vector<int> &cnt = S.cnt;
    F.zmax = S.zmax; F.hmax = S.hmax; F.ext = 0;
    F.fast_ok = (S.NA == 384 && G == 48) && S.hmax <= DSS_HCX + DSS_HX;
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
    auto zr_of = [&](int grp) { return std::max(cnt[grp], cnt[G + grp]); };
    std::vector<int> order_h(G), order_zr(G);
    for (int g = 0; g < G; ++g) order_h[g] = order_zr[g] = g;
    std::stable_sort(order_h.begin(), order_h.end(), [&](int a, int b2) { return cnt[2 * G + a] > cnt[2 * G + b2]; });
    std::stable_sort(order_zr.begin(), order_zr.end(), [&](int a, int b2) { return zr_of(a) > zr_of(b2); });
    // Register slots per gate on waves 4, 5.  A model that fits the register slots as it is runs the 10-slot
    // instantiation (no spills) or, with 11 or 12 blocks in some group, the 12-slot one (22 spilled registers, ~4 %
    // slower).  Any other model runs the 10-slot layout with tails: measured faster than 12 slots + tails
    // (tools/model_fit.py), the spills cost more than the two extra tail blocks.
    const int zr17 = zr_of(order_zr[16]);                  // heaviest group that lands on waves 0..3
    const bool plain = S.zmax <= DSS_ZRC && zr17 <= 8 && S.hmax <= DSS_HC;
    F.zr_cap = (plain && S.zmax > 10) ? DSS_ZRC : 10;
    static const int rank_wave_zr[6] = {4, 5, 2, 3, 1, 0};
    int rank_wave_h[6]; rank_wave_h_order(rank_wave_h);
    F.grp_h.assign(G, 0); F.grp_zr.assign(G, 0); F.wave_nh.assign(8, 0); F.wave_nzr.assign(8, 0); F.wave_nzt.assign(8, 0);
    for (int rk = 0; rk < 6 && F.fast_ok; ++rk) {
        const int wh = rank_wave_h[rk], wz = rank_wave_zr[rk], cap = F.zr_regs(wz);
        int nh = 0, nzr = 0;
        for (int q = 0; q < 8; ++q) {
            F.grp_h[wh * 8 + q] = order_h[rk * 8 + q];
            F.grp_zr[wz * 8 + q] = order_zr[rk * 8 + q];
            nh = std::max(nh, cnt[2 * G + order_h[rk * 8 + q]]);
            nzr = std::max(nzr, zr_of(order_zr[rk * 8 + q]));
        }
        F.wave_nh[wh] = (nh + 1) & ~1;                  // the kernel tests for the end of a list every 2 slots
        F.wave_nzr[wz] = std::min((nzr + 1) & ~1, cap);
        F.wave_nzt[wz] = std::max(0, nzr - cap);
        if (nzr - cap > DSS_ZR_TAIL) F.fast_ok = 0;
        if (nzr > cap || nh > DSS_HC) F.ext = 1;
    }
}

// Stage 2, offsets of the LDS image: every place's h records, then (extended paths) its tail records and the table.
static void layout_offsets(const SparseGroups &S, FastLayout &F)
{
    const int G = S.G;
    F.grp_hoff.assign(G, 0); F.tail_off.assign(G * 2, 0); F.hfloats = F.ext_tab = 0;
    if (!F.fast_ok) return;
    // The h-gate image: every row group's own records back to back (128 bytes = [8 rows][4 inputs] per block), no
    // padding to the wave's longest list.  A wave still runs wave_nh slots on all its lanes: a lane whose group is
    // shorter reads on into the next group's records and multiplies them by "column 96", four zeros behind the
    // state vector, so the extra terms are +-0.  One spare record goes between two groups of a wave whenever
    // they would otherwise start an even number of records apart: 8-lane groups that start 32 banks apart keep
    // the wave's ds_read_b128 of its block records conflict-free.
    int hfloats = 0, hend = 0;
    each_place([&](int wv, int q, int place) {
        if (q && (((hfloats - F.grp_hoff[place - 1]) / 32) & 1) == 0) hfloats += 32;
        F.grp_hoff[place] = hfloats;
        hfloats += S.cnt[2 * G + F.grp_h[place]] * 32;
        hend = std::max(hend, F.grp_hoff[place] + (F.wave_nh[wv] + 4) * 32);      // + 4: the kernel fetches two chunks of two slots ahead
    });
    hfloats = std::max(hfloats, hend);                  // the last groups' over-reads stay inside the image
    // Extended paths (models with skewed sparsity only): behind the h records, the z and r tail lists of every
    // group of the z/r assignment (same over-read convention), then a table
    //   int   tail_off[48][2]                float offset of the group's z list and of its r list
    //   uint8 tail_col[48][2][DSS_ZR_TAIL]   block column of every tail slot (96 = unused)
    //   uint8 hx_col[48][DSS_HX]             block column of h slots DSS_HCX.. of the group of the h assignment
    if (F.ext) {
        int tend = hfloats;
        each_place([&](int wv, int, int place) {
            for (int gate = 0; gate < 2; ++gate) {
                F.tail_off[place * 2 + gate] = hfloats;
                tend = std::max(tend, hfloats + F.wave_nzt[wv] * 32);
                hfloats += std::max(0, S.cnt[gate * G + F.grp_zr[place]] - F.zr_regs(wv)) * 32;
            }
        });
        F.ext_tab = std::max(hfloats, tend);
        hfloats = F.ext_tab + (G * 2 * 4 + G * 2 * DSS_ZR_TAIL + G * DSS_HX) / 4 + 4;      // + 16 B: the kernel reads columns one trip ahead
    }
    F.hfloats = hfloats;
    if ((size_t)hfloats * sizeof(float) > DSS_HBLK_BYTES) F.fast_ok = 0;
}

// Stage 3, fill: per lane its units, the z/r register slots (weights, columns), and its row of the tail and h records.
static void layout_fill(const SparseGroups &S, FastLayout &F)
{
    const int NA = S.NA, G = S.G;
    F.unit_of.assign(NA, 0); F.unit_h.assign(NA, 0);
    F.zr_w.assign((size_t)2 * DSS_ZRC * 4 * NA, 0.f); F.hblk.assign((size_t)std::max(F.hfloats, 4), 0.f);
    F.zr_col.assign((size_t)(2 * DSS_ZRC / 4) * NA, 0u); F.h_col.assign((size_t)(DSS_HCX / 4) * NA, 0u);
    if (!F.fast_ok) return;
    each_place([&](int wv, int, int place) {
        const int cap = F.zr_regs(wv), gh = 2 * G + F.grp_h[place];
        for (int r = 0; r < 8; ++r) {
            const int tid = place * 8 + r;
            F.unit_of[tid] = F.grp_zr[place] * 8 + r; F.unit_h[tid] = F.grp_h[place] * 8 + r;
            for (int gate = 0; gate < 2; ++gate) {
                const int g = gate * G + F.grp_zr[place];
                for (int sl = 0; sl < std::min(S.cnt[g], cap); ++sl) {
                    const int s2 = gate * DSS_ZRC + sl;
                    S.block_row(g, sl, r, &F.zr_w[(size_t)s2 * 4 * NA + tid], NA);
                    F.zr_col[(size_t)(s2 >> 2) * NA + tid] |= (unsigned)S.col(g, sl) << (8 * (s2 & 3));
                }
                for (int sl = cap; sl < S.cnt[g]; ++sl)                    // tail: LDS records, columns in the table
                    S.block_row(g, sl, r, &F.hblk[F.tail_off[place * 2 + gate] + (size_t)(sl - cap) * 32 + r * 4]);
            }
            for (int sl = 0; sl < S.cnt[gh]; ++sl) {
                S.block_row(gh, sl, r, &F.hblk[F.grp_hoff[place] + (size_t)sl * 32 + r * 4]);
                if (sl < DSS_HCX) F.h_col[(size_t)(sl >> 2) * NA + tid] |= (unsigned)S.col(gh, sl) << (8 * (sl & 3));
            }
            for (int sl = S.cnt[gh]; sl < DSS_HCX; ++sl) F.h_col[(size_t)(sl >> 2) * NA + tid] |= 96u << (8 * (sl & 3));
        }
    });
}

struct ExtTable {        // the table of the extended paths inside hblk (layout_offsets describes it)
    int *toff; unsigned char *tcol, *hxc;
    ExtTable(float *at, int G) : toff(reinterpret_cast<int *>(at)), tcol(reinterpret_cast<unsigned char *>(toff + G * 2)), hxc(tcol + (size_t)G * 2 * DSS_ZR_TAIL) {}
};

// Stage 4, the table of the extended paths: tail offsets, tail columns, columns of the long h lists.
static void layout_ext_table(const SparseGroups &S, FastLayout &F)
{
    const int G = S.G;
    if (!F.fast_ok || !F.ext) return;
    const ExtTable T(F.hblk.data() + F.ext_tab, G);
    memset(T.tcol, 96, (size_t)G * 2 * DSS_ZR_TAIL + (size_t)G * DSS_HX);
    each_place([&](int wv, int, int place) {
        const int cap = F.zr_regs(wv), gh = 2 * G + F.grp_h[place];
        for (int gate = 0; gate < 2; ++gate) {
            const int g = gate * G + F.grp_zr[place];
            T.toff[place * 2 + gate] = F.tail_off[place * 2 + gate];
            for (int sl = cap; sl < S.cnt[g]; ++sl)
                T.tcol[((size_t)place * 2 + gate) * DSS_ZR_TAIL + (sl - cap)] = (unsigned char)S.col(g, sl);
        }
        for (int sl = DSS_HCX; sl < S.cnt[gh]; ++sl) T.hxc[(size_t)place * DSS_HX + (sl - DSS_HCX)] = (unsigned char)S.col(gh, sl);
    });
}

static void build_fast_layout(const SparseGroups &S, FastLayout &F)
{
    layout_assign(S, F); layout_offsets(S, F); layout_fill(S, F); layout_ext_table(S, F);
    if (!F.fast_ok) F.ext = 0;
}

// an embedding table's rows permuted into lane order, the three gates of a lane's unit side by side: [256][NA lanes][3]
static std::vector<float> build_embed_lane(const float *tab, const std::vector<int> &unit_of, int NA)
{
    std::vector<float> perm((size_t)256 * NA * 3);
    for (int idx = 0; idx < 256; ++idx)
        for (int tid = 0; tid < NA; ++tid)
            for (int g = 0; g < 3; ++g) perm[((size_t)idx * NA + tid) * 3 + g] = tab[(size_t)idx * 3 * NA + (size_t)g * NA + unit_of[tid]];
    return perm;
}

// GRU B input weights for the two relay waves, j-major with lane = row: [384][64]; with quad set, four inputs of a lane side by
// side, [384 / 4][64][4], for the pair kernel's relay waves, which stream them from L2
static std::vector<float> build_gb_w(const BlobView &v, int NA, int NB3, bool quad)
{
    std::vector<float> gb((size_t)NA * 64, 0.f);
    for (int j = 0; j < NA; ++j)
        for (int row = 0; row < NB3; ++row)
            gb[quad ? ((size_t)(j / 4) * 64 + row) * 4 + (j & 3) : (size_t)j * 64 + row] = v.gru_b_w_in[(size_t)j * NB3 + row];
    return gb;
}

// dual-FC weights for the pair kernel, whose dual-FC waves load their node's 32 weights every sample instead of
// holding them in registers: [k 8][node 256][4] = (layer 0, layer 1) weights of inputs 2k and 2k+1, so that load k
// of a wave reads 1 KB of consecutive bytes
static std::vector<float> build_fc_w_pair(const BlobView &v)
{
    std::vector<float> fcp((size_t)DSS_FC_OUT * DSS_GRU_B * 2, 0.f);
    for (int node = 0; node < DSS_FC_OUT; ++node)
        for (int j = 0; j < DSS_GRU_B; ++j) {
            const size_t o = ((size_t)(j / 2) * DSS_FC_OUT + node) * 4 + (j & 1) * 2;
            fcp[o + 0] = v.fc_w[(size_t)node * 2 * DSS_GRU_B + j];
            fcp[o + 1] = v.fc_w[(size_t)node * 2 * DSS_GRU_B + DSS_GRU_B + j];
        }
    return fcp;
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

// derived tables (host libm, exactly as xiph builds them at run time); those of lpc_from_cepstrum are LpcTables (lpc_tables.h)
struct LibmTables : LpcTables {
    float tansig[DSS_TANSIG_Y + 201] = {0}, logit[256], u2l[256];
    LibmTables()
    {
        dss_tansig_tables(tansig);
        for (int i = 0; i < 256; ++i) {                                                              // lpcnet_init()
            float prob = .025 + .95 * i / 255.;
            logit[i] = -log((1 - prob) / prob);
            u2l[i] = host_ulaw2lin((float)i);
        }
    }
};

// ---- upload -------------------------------------------------------------------------------------------------------------
// Puts one array after the other on the device (DssDevBlocks::upload: 16 spare bytes behind each) and its pointer into the
// DssModelDev field; after the first failure it does nothing more, and rc keeps that failure.
struct Uploader {
    DssDevBlocks &mem;
    int rc = DSS_OK;
    template <typename T> void operator()(const T *&field, const T *host, size_t count)
    {
        T *d = nullptr;
        if (!rc) rc = mem.upload<T>(host, count, &d);
        if (!rc) field = d;
    }
    template <typename T> void operator()(const T *&field, const std::vector<T> &host) { (*this)(field, host.data(), host.size()); }
};

static int upload_model(HostModel *hm, int device, DssModelDev &m)
{
    const BlobView &v = hm->v; const SparseGroups &S = hm->groups; const dss_blob_header &h = hm->h;
    const int fin = h.nb_features + h.embed_pitch_dim, NA = h.gru_a, NA3 = 3 * NA, NB3 = 3 * h.gru_b;
    Uploader up{hm->dev_blocks[device]};
    memset(&m, 0, sizeof(m));
    m.h = h;
    // ---- the blob's own arrays ------------------------------------------------------------------------------
    up(m.embed_pitch, v.embed_pitch, (size_t)h.pitch_max * h.embed_pitch_dim);
    up(m.conv1_w, v.conv1_w, (size_t)3 * fin * 128);   up(m.conv1_b, v.conv1_b, 128);
    up(m.conv2_w, v.conv2_w, (size_t)3 * 128 * 128);   up(m.conv2_b, v.conv2_b, 128);
    up(m.dense1_w, v.dense1_w, 128 * 128);             up(m.dense1_b, v.dense1_b, 128);
    up(m.dense2_w, v.dense2_w, 128 * 128);             up(m.dense2_b, v.dense2_b, 128);
    up(m.gru_a_dense_w, v.gru_a_dense_w, (size_t)128 * NA3);  up(m.gru_a_dense_b, v.gru_a_dense_b, NA3);
    up(m.gru_b_dense_w, v.gru_b_dense_w, (size_t)128 * NB3);  up(m.gru_b_dense_b, v.gru_b_dense_b, NB3);
    up(m.embed_sig, v.embed_sig, (size_t)256 * NA3); up(m.embed_pred, v.embed_pred, (size_t)256 * NA3); up(m.embed_exc, v.embed_exc, (size_t)256 * NA3);
    up(m.gru_a_rbias, v.gru_a_rbias, NA3);           up(m.gru_a_diag, v.gru_a_diag, NA3);
    up(m.gru_b_bias, v.gru_b_bias, 2 * NB3); up(m.gru_b_w_in, v.gru_b_w_in, (size_t)NA * NB3); up(m.gru_b_w_rec, v.gru_b_w_rec, (size_t)h.gru_b * NB3);
    up(m.fc_bias, v.fc_bias, 2 * h.dual_fc_out); up(m.fc_w, v.fc_w, (size_t)h.dual_fc_out * 2 * h.gru_b); up(m.fc_factor, v.fc_factor, 2 * h.dual_fc_out);
    // ---- sparse GRU A as the generic kernel reads it -------------------------------------------------------
    for (int gate = 0; gate < 3; ++gate) {
        const GenericGate L = build_generic_gate(S, gate);
        m.gate[gate].slots = L.slots;
        up(m.gate[gate].pos4, L.pos4); up(m.gate[gate].w, L.w);
    }
    // ---- CU-resident layout of the sample-rate kernel (lpcnet_sample.hip) ---------------------------------
    FastLayout F;
    build_fast_layout(S, F);
    m.fast_ok = F.fast_ok; m.nzr_max = (F.zmax + 1) & ~1; m.zr_cap = F.zr_cap; m.hmax = F.hmax;
    m.ext = F.ext; m.ext_tab = F.ext_tab; m.hblk_floats = F.hfloats;
    up(m.unit_of, F.unit_of);
    const float *tabs[3] = {v.embed_sig, v.embed_pred, v.embed_exc};
    for (int t = 0; t < 3; ++t) up(m.embed_lane[t], build_embed_lane(tabs[t], F.unit_of, NA));
    up(m.unit_h, F.unit_h);     up(m.wave_nh, F.wave_nh);   up(m.grp_hoff, F.grp_hoff);
    up(m.wave_nzr, F.wave_nzr); up(m.wave_nzt, F.wave_nzt);
    up(m.zr_w, F.zr_w);         up(m.zr_col, F.zr_col);     up(m.h_col, F.h_col);       up(m.hblk, F.hblk);
    up(m.gb_w_lane, build_gb_w(v, NA, NB3, false)); up(m.gb_w_quad, build_gb_w(v, NA, NB3, true)); up(m.fc_w_pair, build_fc_w_pair(v));
    // ---- derived tables -----------------------------------------------------------------------------------------
    const LibmTables T;
    up(m.tansig, T.tansig, DSS_TANSIG_Y + 201); up(m.logit_table, T.logit, 256); up(m.ulaw2lin, T.u2l, 256);
    up(m.dct_table, T.dct, 324);        up(m.cos_table, T.costab, 320);     up(m.cos_kl, T.cos_kl);
    up(m.interp_a, T.ia, 160);          up(m.interp_b, T.ib, 160);          up(m.interp_band, T.iband, 160);   up(m.lag_window, T.lagw, 17);
    return up.rc;
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
        HostModel *loaded = nullptr;
        rc = read_file(path, buf);
        if (!rc) rc = parse_blob(buf.data(), buf.size(), &loaded);
        if (rc) return rc;
        install_locked(loaded);
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
    if (fast_path) *fast_path = m->fast_ok ? (m->ext ? 2 : 1) : 0;
    if (zr_slots_max) *zr_slots_max = m->nzr_max;
    if (h_slots_max) *h_slots_max = hm->groups.hmax;
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
// order, with the row's blocks in the blob, as parse_sparse() found them.  Needs no GPU (tests/test_cpu_layout.py).
extern "C" int dss_selftest_fast_layout(const void *blob, size_t len, int *info)
{
    if (!blob || !info || len < sizeof(dss_blob_header)) { dss_set_error("dss_selftest_fast_layout: bad arguments"); return DSS_EINVAL; }
    const std::vector<char> copy((const char *)blob, (const char *)blob + len);
    dss_blob_header h; BlobView v; SparseGroups S;
    const int rc = parse_views(copy, h, v, S);
    if (rc) return rc;
    const int NA = S.NA, G = S.G;
    FastLayout F;
    build_fast_layout(S, F);
    for (int k = 0; k < 8; ++k) info[k] = 0;
    info[0] = F.fast_ok ? (F.ext ? 2 : 1) : 0;
    info[1] = F.zmax; info[2] = F.hmax; info[3] = F.hfloats * 4; info[4] = F.zr_cap;
    if (!F.fast_ok) return DSS_OK;
    int mismatches = 0, oob = 0, tails = 0;
    const int rec_end = F.ext ? F.ext_tab : F.hfloats;                 // records may be read up to here
    const ExtTable T(F.hblk.data() + F.ext_tab, G);
    std::vector<int> seen_zr(NA, 0), seen_h(NA, 0);
    struct Blk { int col; float w[4]; };
    auto lds_blk = [&](int off, int col) { Blk b; b.col = col; memcpy(b.w, &F.hblk[off], sizeof(b.w)); return b; };      // a lane's row of a record
    auto compare = [&](const std::vector<Blk> &got, int g, int r) {
        // drop the terms that are +-0 by construction: zero column, or an all-zero padded register slot
        std::vector<Blk> eff;
        for (const Blk &b : got)
            if (b.col != 96 && !(b.w[0] == 0.f && b.w[1] == 0.f && b.w[2] == 0.f && b.w[3] == 0.f)) eff.push_back(b);
        if ((int)eff.size() != S.cnt[g]) { ++mismatches; return; }
        for (int sl = 0; sl < S.cnt[g]; ++sl) {
            float want[4];
            S.block_row(g, sl, r, want);
            if (eff[sl].col != S.col(g, sl)) { ++mismatches; return; }
            for (int k = 0; k < 4; ++k) if (eff[sl].w[k] != want[k]) { ++mismatches; return; }
        }
    };
    for (int tid = 0; tid < NA; ++tid) {
        const int wave = tid / 64, lane = tid & 63, grp2 = tid >> 3;
        {   // z and r lists of unit_of[tid]
            const int unit = F.unit_of[tid];
            if (unit < 0 || unit >= NA) { ++mismatches; continue; }
            ++seen_zr[unit];
            const int nzr = F.wave_nzr[wave], nzt = F.ext ? F.wave_nzt[wave] : 0;
            if (nzr > F.zr_regs(wave) || (!F.ext && F.wave_nzt[wave])) ++mismatches;
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
                    const int off = T.toff[grp2 * 2 + gate] + sl * 32 + (lane & 7) * 4;
                    if (off < 0 || off + 4 > rec_end) { ++oob; continue; }
                    got.push_back(lds_blk(off, T.tcol[((size_t)grp2 * 2 + gate) * DSS_ZR_TAIL + sl]));
                    if (got.back().col != 96) ++tails;
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
                got.push_back(lds_blk(off, sl < hreg ? (int)((F.h_col[(size_t)(sl >> 2) * NA + tid] >> (8 * (sl & 3))) & 0xFF) : (int)T.hxc[(size_t)grp2 * DSS_HX + (sl - DSS_HCX)]));
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
