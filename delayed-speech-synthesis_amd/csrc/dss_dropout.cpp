// csrc/dss_dropout.cpp -- host side of Part 14 of include/dss_hip.h: the dropout masks of the trainers from a counter-based
// generator.  A mask is a pure function of its entry, so this part owns nothing: no handle, no device memory, no table ring (the
// entries travel as kernel arguments).  dss_dropout_masks_host is the same definition on the CPU, element by element, for hosts
// without a device and for the tests.
#include <math.h>

#include "dropout.h"
#include "dss_host.h"

static inline long long entry_elements(const dss_dropout_entry &e) { return (long long)e.rows * (long long)e.width; }

extern "C" int dss_dropout_check(int n_entries, const dss_dropout_entry *e)
{
    if (n_entries < 1 || n_entries > DSS_DROPOUT_MAX_ENTRIES) {
        dss_set_error("dropout masks: %d entries: must be 1 .. %d (more masks: more calls)", n_entries, DSS_DROPOUT_MAX_ENTRIES);
        return DSS_EINVAL;
    }
    if (!e) { dss_set_error("dropout masks: null entry table"); return DSS_EINVAL; }
    int live = 0;
    for (int i = 0; i < n_entries; ++i) {
        if (e[i].rows < 0 || e[i].width < 0) {
            dss_set_error("dropout masks: entry %d: a mask of %d x %d (negative size)", i, e[i].rows, e[i].width);
            return DSS_EINVAL;
        }
        if (!entry_elements(e[i])) continue;                // rows == 0 (or width == 0): left alone, nothing else of it is looked at
        if (entry_elements(e[i]) >= (1ll << 31)) {
            dss_set_error("dropout masks: entry %d: %d x %d elements: must be fewer than 2^31", i, e[i].rows, e[i].width);
            return DSS_EINVAL;
        }
        if (!e[i].d_mask || ((uintptr_t)e[i].d_mask & 3u)) {
            dss_set_error("dropout masks: entry %d: the mask pointer is null or not 4-byte aligned", i);
            return DSS_EINVAL;
        }
        if (!(e[i].p > 0.0f && e[i].p < 1.0f)) {
            dss_set_error("dropout masks: entry %d: p = %g: must be inside (0, 1) (p = 0 is no mask at all)", i, (double)e[i].p);
            return DSS_EINVAL;
        }
        if (!(e[i].scale > 0.0f) || isinf(e[i].scale)) {
            dss_set_error("dropout masks: entry %d: scale = %g: must be the finite 1 / (1 - p)", i, (double)e[i].scale);
            return DSS_EINVAL;
        }
        ++live;
    }
    if (!live) { dss_set_error("dropout masks: every entry is empty: nothing to fill"); return DSS_EINVAL; }
    return DSS_OK;
}

extern "C" int dss_dropout_masks_dev(const dss_dropout_entry *entries, int n_entries, void *hip_stream)
{
    int rc = dss_dropout_check(n_entries, entries);
    if (rc) return rc;
    if (dss_ensure_device()) return DSS_ENODEV;
    DssDropoutTable tab;
    memset(&tab, 0, sizeof(tab));
    unsigned max_blocks = 0;
    for (int i = 0; i < n_entries; ++i) {
        if (!entry_elements(entries[i])) continue;          // stays zeroed: its workgroups return at once
        tab.e[i] = entries[i];
        max_blocks = std::max(max_blocks, (unsigned)((entry_elements(entries[i]) + 3) / 4));
    }
    return dss_launch_dropout_masks(tab, n_entries, max_blocks, (hipStream_t)hip_stream);
}

extern "C" int dss_dropout_masks_host(const dss_dropout_entry *entries, int n_entries)
{
    int rc = dss_dropout_check(n_entries, entries);
    if (rc) return rc;
    for (int i = 0; i < n_entries; ++i) {
        const dss_dropout_entry &e = entries[i];
        const long long n = entry_elements(e);
        for (long long first = 0; first < n; first += 4) {
            float v[4];
            dss_dropout_block(e, (uint64_t)(first >> 2), v);
            for (int j = 0; j < 4 && first + j < n; ++j) e.d_mask[first + j] = v[j];
        }
    }
    return DSS_OK;
}

extern "C" int dss_selftest_philox(const unsigned *counter, const unsigned *key, unsigned *out)
{
    if (!counter || !key || !out) { dss_set_error("dss_selftest_philox: null argument"); return DSS_EINVAL; }
    uint32_t c[4] = {counter[0], counter[1], counter[2], counter[3]};
    dss_philox4x32_10(c, key[0], key[1]);
    for (int j = 0; j < 4; ++j) out[j] = c[j];
    return DSS_OK;
}
