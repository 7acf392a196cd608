// csrc/dss_global_ptr.h -- a pointer read from a descriptor or from a trial table, as a pointer to global memory (the trainers'
// kernels: dec_train.hip, vad_train.hip).
#pragma once

#include <hip/hip_runtime.h>

// The compiler knows that a kernel argument's pointer members point to global memory; of a pointer it loaded from a device table
// (the group kernels, which step several trainers in one launch) it does not, and would address it through the flat aperture:
// those loads also count as LDS traffic in the waits of the serial chains.  Changes no value and costs no instruction.
template <typename P>
__device__ __forceinline__ P *dss_gp(P *p)
{
    typedef __attribute__((address_space(1))) P *G;
    return (P *)(G)(unsigned long long)p;
}

// A global pointer whose value is the same in every lane of the wave (a row of a stash: base + step * row length), said so.  The
// compiler then keeps it in scalar registers and addresses row[lane] as scalar base + 32-bit lane offset; left to itself it
// reassociates base + step * n + lane into (base + lane) + step * n and hoists one 64-bit per-lane address per array out of the
// time loop, which is what the serial kernels' VGPR count is made of.  Changes no value.
template <typename P>
__device__ __forceinline__ P *dss_uniform(P *p)
{
    const unsigned long long v = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
    return dss_gp((P *)(((unsigned long long)hi << 32) | lo));
}

// An entry of a device table that nothing writes while the kernel runs (the host wrote it, in stream order, before the launch), as
// constant memory: what kernel arguments are.  Its loads are scalar loads wherever they stand, also behind the kernel's own
// stores to global memory, which would otherwise turn a later read of the entry into a vector load.
template <typename P>
__device__ __forceinline__ const P *dss_cp(const P *p)
{
    typedef const __attribute__((address_space(4))) P *K;
    return (const P *)(K)(unsigned long long)p;
}
