// csrc/dropout.h -- the dropout-mask generator of Part 14 of include/dss_hip.h, the part that the kernel (dropout.hip) and the
// library's scalar restatement (dss_dropout.cpp) share word for word: the Philox4x32-10 block and the word -> multiplier rule.
#pragma once

#include "dss_common.h"

#define DSS_DROPOUT_MAX_ENTRIES 64
#define DSS_DROPOUT_THREADS 256   // Philox blocks (of four elements) per workgroup

// the entries of one launch, handed to the kernel by value (64 x 40 bytes); entry blockIdx.y is the workgroup's
struct DssDropoutTable { dss_dropout_entry e[DSS_DROPOUT_MAX_ENTRIES]; };

// Philox4x32-10 (Salmon et al., SC'11): c and k in, the block in c.  Every round maps (c0, c1, c2, c3) to
// (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)), then the key moves on.
__host__ __device__ static inline void dss_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// block b of an entry's mask: its elements 4b .. 4b + 3 as multipliers
__host__ __device__ static inline void dss_dropout_block(const dss_dropout_entry &e, uint64_t b, float out[4])
{
    uint32_t c[4] = {(uint32_t)b, (uint32_t)(b >> 32), (uint32_t)e.draw, (uint32_t)(e.draw >> 32)};
    dss_philox4x32_10(c, (uint32_t)e.seed, (uint32_t)(e.seed >> 32));
    for (int j = 0; j < 4; ++j) {
        const float u = (float)(c[j] >> 8) * 5.9604644775390625e-08f;        // 24 bits x 2^-24: exact
        out[j] = u >= e.p ? e.scale : 0.0f;
    }
}

int dss_launch_dropout_masks(const DssDropoutTable &tab, int n_entries, unsigned max_blocks, hipStream_t s);
