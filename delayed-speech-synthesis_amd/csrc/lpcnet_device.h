// csrc/lpcnet_device.h -- device-side scalar helpers of the LPCNet kernels.
//
// Each helper restates one inline function of xiph/LPCNet (src/vec.h generic path, src/common.h) in the
// exact operation order and precision of the C source: float where the C is float, double where C's
// usual arithmetic conversions promote to double.  The library is built with -ffp-contract=off so no
// product/sum pair is fused.  Tables (tansig, ulaw2lin, sampling logits) are computed by the host's
// libm when a model is loaded and passed in; the device never evaluates exp/log/tanh on this path.
// Two helpers also exist in a shorter instruction sequence that returns the same bits for every fp32 input, each proven
// by a sweep over all 2^32 bit patterns: lin2ulaw (dss_lin2ulaw) and the table activations (dss_sigmoid_short*,
// dss_tanh_times*: 1 - y*y read from a host-built table, the floor and the lower clamp dropped for a non-negative
// argument, the sigmoid's pre-scale as one product, its sign, 1/2 and offset as one fused operation, the tanh's sign
// folded into the factor of its consumer).  Why each step is exact stands in front of the helpers below.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// vec.h tanh_approx (201-entry table form).  `tab` may live in LDS or global memory.
__device__ __forceinline__ float dss_tanh_approx(const float *tab, float x)
{
    float sign = 1.f;
    if (x < 0) { x = -x; sign = -1.f; }
    int i = (int)floorf(.5f + 25 * x);
    i = i < 0 ? 0 : i;
    i = i > 200 ? 200 : i;
    x -= .04f * i;
    const float y = tab[i];
    const float dy = 1 - y * y;
    const float r = y + x * dy * (1 - y * x);
    return sign * r;
}

// Two independent evaluations with both table reads issued before either is consumed (same arithmetic per
// element as dss_tanh_approx; only the instruction interleaving differs).
__device__ __forceinline__ void dss_tanh_approx2(const float *tab, float x1, float x2, float &o1, float &o2)
{
    float s1 = 1.f, s2 = 1.f;
    if (x1 < 0) { x1 = -x1; s1 = -1.f; }
    if (x2 < 0) { x2 = -x2; s2 = -1.f; }
    int i1 = (int)floorf(.5f + 25 * x1);
    int i2 = (int)floorf(.5f + 25 * x2);
    i1 = i1 < 0 ? 0 : i1; i1 = i1 > 200 ? 200 : i1;
    i2 = i2 < 0 ? 0 : i2; i2 = i2 > 200 ? 200 : i2;
    const float y1 = tab[i1];
    const float y2 = tab[i2];
    x1 -= .04f * i1;
    x2 -= .04f * i2;
    const float d1 = 1 - y1 * y1, d2 = 1 - y2 * y2;
    const float r1 = y1 + x1 * d1 * (1 - y1 * x1);
    const float r2 = y2 + x2 * d2 * (1 - y2 * x2);
    o1 = s1 * r1;
    o2 = s2 * r2;
}

__device__ __forceinline__ void dss_sigmoid_approx2(const float *tab, float x1, float x2, float &o1, float &o2)
{
    float t1, t2;
    dss_tanh_approx2(tab, .5f * x1, .5f * x2, t1, t2);
    o1 = .5f + .5f * t1;
    o2 = .5f + .5f * t2;
}

__device__ __forceinline__ float dss_sigmoid_approx(const float *tab, float x)
{
    return .5f + .5f * dss_tanh_approx(tab, .5f * x);
}

// ---- short forms of the two table activations, for the CU-resident sample kernel (lpcnet_sample.hip) ----------------
// Every activation there stands on the sample's serial path, so these take out the instructions whose result does not
// depend on the run-time value in any way the result needs.  Each step returns the bits of the form above for every fp32
// input (tools/verify/tansig_exhaustive.c visits all 2^32 patterns on the host, dss_selftest_tansig on the device):
//   * dy = 1 - y*y depends on the table entry alone: the host forms it once, as two separately rounded fp32 operations,
//     when it builds the table (dss_lpcnet_model.cpp: m.tansig[DSS_TANSIG_Y + i]).  Both reads take the same index
//     register and an immediate offset, so they go out back to back, and x*dy and y*x start together.  (The kernel keeps
//     the two tables more than 255 words apart on purpose: nearer, the compiler joins them into one ds_read2_b32, whose
//     base then costs a further dependent v_add in front of the read.)
//   * the argument is >= 0 once the sign is taken off, so the conversion's truncation IS the floor, and the lower clamp
//     is dead.  The upper clamp is taken in fp32 ahead of the conversion (min(t, 200) and then truncation give
//     min(floor(t), 200)); it also keeps the conversion in range.  A NaN picks entry 200 instead of 0 and stays a NaN.
//   * sigmoid: 25*(.5f*x) == 12.5f*x.  Halving is exact until it reaches the last subnormal bits, and there both
//     products are far below .5 and select entry 0.  The halved x is still what the correction term uses, off the path
//     to the LDS address.
//   * sigmoid: .5f + .5f*(s*r) == fma(s*.5f, r, .5f), s = +-1.  (s*.5f)*r is an exact scaling of r, so the fused form
//     rounds the same sum once; where the scaling would lose a subnormal bit, both sums round to .5f.  +-.5f is known
//     before the read returns.
//   * tanh: the caller folds the sign into the factor the result is multiplied by: a*(s*r) == (s*a)*r, because
//     round-to-nearest is symmetric in the sign (also into the subnormal range) and s*r, s*a are exact.  The sign test
//     is the form's own `x < 0` (a -0 or a NaN counts as positive), never the sign bit: (-a)*0 would be -0.
// `tab` is the y table, `dtab` the table of 1 - y*y.  The "2" forms evaluate two independent arguments with all four table
// reads issued before any is consumed (left to itself the compiler finishes the first look-up before it starts the second).
__device__ __forceinline__ float dss_tansig_core(const float *tab, const float *dtab, float t, float ax)
{
    const int i = (int)__builtin_fminf(.5f + t, 200.f);
    const float y = tab[i], dy = dtab[i];
    const float x = ax - .04f * i;
    return y + x * dy * (1 - y * x);
}

__device__ __forceinline__ void dss_tansig_core2(const float *tab, const float *dtab, float t1, float t2, float ax1, float ax2,
                                                 float &r1, float &r2)
{
    const int i1 = (int)__builtin_fminf(.5f + t1, 200.f);
    const int i2 = (int)__builtin_fminf(.5f + t2, 200.f);
    const float y1 = tab[i1], d1 = dtab[i1];
    const float y2 = tab[i2], d2 = dtab[i2];
    const float x1 = ax1 - .04f * i1;
    const float x2 = ax2 - .04f * i2;
    r1 = y1 + x1 * d1 * (1 - y1 * x1);
    r2 = y2 + x2 * d2 * (1 - y2 * x2);
}

// a * dss_tanh_approx(tab, x)
__device__ __forceinline__ float dss_tanh_times(const float *tab, const float *dtab, float a, float x)
{
    const float ax = __builtin_fabsf(x);
    const float sa = x < 0 ? -a : a;
    return sa * dss_tansig_core(tab, dtab, 25 * ax, ax);
}

__device__ __forceinline__ void dss_tanh_times2(const float *tab, const float *dtab, float a1, float x1, float a2, float x2,
                                                float &o1, float &o2)
{
    const float ax1 = __builtin_fabsf(x1), ax2 = __builtin_fabsf(x2);
    const float sa1 = x1 < 0 ? -a1 : a1, sa2 = x2 < 0 ? -a2 : a2;
    float r1, r2;
    dss_tansig_core2(tab, dtab, 25 * ax1, 25 * ax2, ax1, ax2, r1, r2);
    o1 = sa1 * r1;
    o2 = sa2 * r2;
}

__device__ __forceinline__ float dss_sigmoid_short(const float *tab, const float *dtab, float x)
{
    const float ax = __builtin_fabsf(x);
    const float sh = x < 0 ? -.5f : .5f;
    return __builtin_fmaf(sh, dss_tansig_core(tab, dtab, 12.5f * ax, .5f * ax), .5f);
}

__device__ __forceinline__ void dss_sigmoid_short2(const float *tab, const float *dtab, float x1, float x2, float &o1, float &o2)
{
    const float ax1 = __builtin_fabsf(x1), ax2 = __builtin_fabsf(x2);
    const float sh1 = x1 < 0 ? -.5f : .5f, sh2 = x2 < 0 ? -.5f : .5f;
    float r1, r2;
    dss_tansig_core2(tab, dtab, 12.5f * ax1, 12.5f * ax2, .5f * ax1, .5f * ax2, r1, r2);
    o1 = __builtin_fmaf(sh1, r1, .5f);
    o2 = __builtin_fmaf(sh2, r2, .5f);
}

// common.h log2_approx / lin2ulaw
__device__ __forceinline__ float dss_log2_approx(float x)
{
    int in = __float_as_int(x);
    const int integer = (in >> 23) - 127;
    in -= integer << 23;
    float frac = __int_as_float(in) - 1.5f;
    frac = -0.41445418f + frac * (0.95909232f + frac * (-0.33951290f + frac * 0.16541097f));
    return 1 + integer + frac;
}

// xiph common.h lin2ulaw(), in a shorter instruction sequence that returns the same value for every fp32 input
// (tools/verify/lin2ulaw_exhaustive.c visits all 2^32 bit patterns against the test suite's restatement of the C source):
//   * u / 5.5451774445f as q0 = u * (1/c), r = fma(-q0, c, u), q = fma(r, 1/c, q0) -- the correctly rounded quotient for
//     every numerator that can occur (checked for all 2^-100 < |u| < 2^100), 3 instructions instead of the 11 of an IEEE
//     division.  The fused operations are internal to the division; they replace v_div_scale/v_rcp/v_fma.../v_div_fixup,
//     which are fused as well.
//   * the clamp to [0, 255] as max/min, floor(.5 + (double)u) as floorf(u + .5f): exact for 0 <= u <= 255.
// The speculation evaluates this 8 times per lane and sample (16 in the two-utterance kernel), between barriers B and
// C where the CU is issue-bound: 37 -> 21 VALU instructions each.
__device__ __forceinline__ int dss_lin2ulaw(float x)
{
    const float scale = 255.f / 32768.f;
    const float c = 5.5451774445f, rc = 1.0f / 5.5451774445f;
    const float s128 = (x < 0) ? -128.f : 128.f;         // s * (128 * t) == (s * 128) * t: both factors are exact scalings
    x = fabsf(x);
    float u = s128 * (0.69315f * dss_log2_approx(1 + scale * x));
    const float q0 = u * rc;
    const float r = __builtin_fmaf(-q0, c, u);
    u = __builtin_fmaf(r, rc, q0);
    u = 128 + u;
    u = __builtin_fminf(__builtin_fmaxf(u, 0.f), 255.f);
    return (int)floorf(u + .5f);            // (v_cvt_rpi_i32_f32 does this in one instruction and passes the sweep, but as inline asm it measured 0.3 % slower)
}

// kiss99.c
struct DssKiss99 { uint32_t z, w, jsr, jcong; };

__device__ __forceinline__ uint32_t dss_kiss99_rand(DssKiss99 &c)
{
    const uint32_t znew = 36969u * (c.z & 0xFFFF) + (c.z >> 16);
    const uint32_t wnew = 18000u * (c.w & 0xFFFF) + (c.w >> 16);
    const uint32_t mwc = (znew << 16) + wnew;
    uint32_t shr3 = c.jsr ^ (c.jsr << 17);
    shr3 ^= shr3 >> 13;
    shr3 ^= shr3 << 5;
    const uint32_t cong = 69069u * c.jcong + 1234567u;
    c.z = znew; c.w = wnew; c.jsr = shr3; c.jcong = cong;
    return (mwc ^ cong) + shr3;
}
