// csrc/dss_host.cpp -- what dss_host.h declares and no single operator owns: the owner of device memory, trial lists, twiddles.
#include <math.h>

#include <algorithm>

#include "dss_host.h"
#include "lstm_blocks.h"

void dss_pack_rows(float *packed, int H4, int k0, const float *w, int n)
{
    for (int r = 0; r < H4; ++r)
        for (int k = 0; k < n; ++k) packed[lstm_packed_index(k0 + k, r, H4)] = w[(size_t)r * n + k];
}

int DssDevBlocks::alloc_bytes(size_t bytes, void **p)
{
    void *d = nullptr;
    DSS_HIP_CHECK(hipMalloc(&d, bytes));
    blocks.push_back(d);
    *p = d;
    return DSS_OK;
}

void DssDevBlocks::release(const void *p)
{
    auto it = std::find(blocks.begin(), blocks.end(), p);
    if (!p || it == blocks.end()) return;
    blocks.erase(it);
    hipFree(const_cast<void *>(p));
}

void DssDevBlocks::free_all()
{
    for (void *p : blocks) hipFree(p);
    blocks.clear();
}

extern "C" int dss_trials_check(long long N, int n_trials, const long long *first, const int *len, long long *total)
{
    if (!first || !len || !total) { dss_set_error("trial list: null argument"); return DSS_EINVAL; }
    if (n_trials < 0 || N < 0) { dss_set_error("trial list: negative count"); return DSS_EINVAL; }
    long long sum = 0;
    for (int i = 0; i < n_trials; ++i) {
        if (len[i] < 1) { dss_set_error("trial %d: %d frames (at least 1)", i, len[i]); return DSS_EINVAL; }
        if (first[i] < 0) { dss_set_error("trial %d: first row %lld is negative", i, first[i]); return DSS_EINVAL; }
        if (first[i] > N - len[i]) {
            dss_set_error("trial %d: rows %lld .. %lld end behind the %lld rows of the array", i, first[i], first[i] + len[i], N);
            return DSS_EINVAL;
        }
        sum += len[i];
    }
    *total = sum;
    return DSS_OK;
}

std::vector<double> dss_twiddles(int n)
{
    std::vector<double> tw((size_t)2 * n);
    for (int j = 0; j < n; ++j) {
        const double a = 2.0 * M_PI * (double)j / (double)n;
        tw[2 * j] = cos(a);
        tw[2 * j + 1] = sin(a);
    }
    return tw;
}
