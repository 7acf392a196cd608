// csrc/dropout.hip -- the dropout masks of the trainers drawn on the device (Part 14 of include/dss_hip.h): a stateless,
// counter-based generator.  One launch fills the masks of up to 64 entries; the entry is blockIdx.y and its descriptor comes with
// the kernel arguments, so there is no table in memory to keep alive behind a queued launch.  A thread owns one Philox block,
// that is four consecutive elements: twenty 32 x 32 -> 64 bit products for 16 bytes stored.
#include "dropout.h"

typedef float floatx4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(DSS_DROPOUT_THREADS) void dropout_masks_kernel(const DssDropoutTable tab)
{
    const dss_dropout_entry &e = tab.e[blockIdx.y];
    const unsigned n = (unsigned)e.rows * (unsigned)e.width;            // < 2^31 (dss_dropout_check); 0: the entry is left alone
    const unsigned b = blockIdx.x * DSS_DROPOUT_THREADS + threadIdx.x;
    if (b >= (n + 3u) / 4u) return;
    float v[4];
    dss_dropout_block(e, b, v);
    const unsigned first = 4u * b;
    float *dst = e.d_mask + first;
    if (first + 4u <= n && ((uintptr_t)dst & 15u) == 0) {
        const floatx4 q = {v[0], v[1], v[2], v[3]};                      // a native vector: one 16-byte store that stays one
        *reinterpret_cast<floatx4 *>(dst) = q;
    } else {                                                             // a mask that starts 1 .. 3 floats off, or its last block
        for (unsigned j = 0; j < 4u; ++j)
            if (first + j < n) dst[j] = v[j];
    }
}

int dss_launch_dropout_masks(const DssDropoutTable &tab, int n_entries, unsigned max_blocks, hipStream_t s)
{
    if (n_entries < 1 || n_entries > DSS_DROPOUT_MAX_ENTRIES || max_blocks < 1) {
        dss_set_error("dropout mask kernel: %d entries / %u blocks out of range", n_entries, max_blocks);
        return DSS_EINVAL;
    }
    const dim3 grid((max_blocks + DSS_DROPOUT_THREADS - 1) / DSS_DROPOUT_THREADS, n_entries);
    hipLaunchKernelGGL(dropout_masks_kernel, grid, dim3(DSS_DROPOUT_THREADS), 0, s, tab);
    DSS_HIP_CHECK(hipGetLastError());
    return DSS_OK;
}
