/* Development aid / proof: the short forms of vec.h's table tanh and sigmoid that the CU-resident sample kernel uses
 * (csrc/lpcnet_device.h dss_tanh_mag / dss_tanh_times / dss_sigmoid_short) return the bits of the forms they replace
 * (dss_tanh_approx / dss_sigmoid_approx, restatements of xiph vec.h) for EVERY fp32 input.
 *
 *   gcc -O2 -ffp-contract=off -fopenmp -o /tmp/tansig tools/verify/tansig_exhaustive.c -lm
 *   /tmp/tansig [stride [edges]]
 *
 * stride 1 visits all 2^32 bit patterns of x.  With a second argument the patterns within +-64 of every index boundary
 * of the 201-entry table (x = (k - .5) / 25, and twice that for the sigmoid, k = 0..200), of 0 and of the clamps
 * (8, 8.02, 16, 16.04) are visited as well, in both signs: what tests/test_cpu_tansig_pairs.py runs with stride 256.
 * Outputs must be bit-equal; a NaN in must give a NaN out of both forms.
 * The float-to-int conversion is modelled as the device does it (v_cvt_i32_f32: truncation, saturating, NaN -> 0); the
 * short form only converts values in [.5, 200].  The two-operand folds a * (s * r) == (s * a) * r cannot be swept: they
 * are compared on 2^24 pseudo-random (a, x) pairs that include subnormals, +-0 and arguments at the clamp. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define TANSIG_Y 208
static float T[TANSIG_Y + 201];          /* [0, 201) y, [208, 409) 1 - y*y: as dss_lpcnet_model.cpp builds them */

static void tables(void)
{
    for (int i = 0; i < 201; ++i) {
        T[i] = (float)(floor(tanh(.04 * i) * 1e6 + .5) / 1e6);
        volatile float yy = T[i] * T[i];
        T[TANSIG_Y + i] = 1.f - yy;
    }
}

static int cvt_i32(float v)              /* v_cvt_i32_f32 */
{
    if (v != v) return 0;
    if (v >= 2147483648.f) return INT32_MAX;
    if (v <= -2147483648.f) return INT32_MIN;
    return (int)v;
}

/* ---- the forms of vec.h (csrc/lpcnet_device.h dss_tanh_approx / dss_sigmoid_approx) ---- */
static float tanh_old(float x)
{
    float sign = 1.f;
    if (x < 0) { x = -x; sign = -1.f; }
    int i = cvt_i32(floorf(.5f + 25 * x));
    i = i < 0 ? 0 : i;
    i = i > 200 ? 200 : i;
    x -= .04f * i;
    const float y = T[i];
    const float dy = 1 - y * y;
    const float r = y + x * dy * (1 - y * x);
    return sign * r;
}
static float sigmoid_old(float x) { return .5f + .5f * tanh_old(.5f * x); }

/* ---- the short forms ---- */
static float core_new(float t, float ax)
{
    const int i = cvt_i32(fminf(.5f + t, 200.f));
    const float dy = T[TANSIG_Y + i], y = T[i];
    const float x = ax - .04f * i;
    return y + x * dy * (1 - y * x);
}
static float tanh_mag_new(float x) { const float ax = fabsf(x); return core_new(25 * ax, ax); }
static float tanh_times_new(float a, float x) { const float sa = x < 0 ? -a : a; return sa * tanh_mag_new(x); }
static float sigmoid_new(float x)
{
    const float ax = fabsf(x);
    const float sh = x < 0 ? -.5f : .5f;
    return fmaf(sh, core_new(12.5f * ax, .5f * ax), .5f);
}

static int same(float a, float b) { return memcmp(&a, &b, 4) == 0 || (a != a && b != b); }

static int check(uint32_t bits, uint64_t *bad_t, uint64_t *bad_s, uint64_t *bad_nan)
{
    float x;
    memcpy(&x, &bits, 4);
    const float to = tanh_old(x), tn = tanh_times_new(1.f, x), so = sigmoid_old(x), sn = sigmoid_new(x);
    int bad = 0;
    if (!same(to, tn)) { if (*bad_t < 5) fprintf(stderr, "tanh differs at %a (%08x): %a vs %a\n", x, bits, to, tn); ++*bad_t; bad = 1; }
    if (!same(so, sn)) { if (*bad_s < 5) fprintf(stderr, "sigmoid differs at %a (%08x): %a vs %a\n", x, bits, so, sn); ++*bad_s; bad = 1; }
    if (x != x && !(tn != tn && sn != sn && to != to && so != so)) { ++*bad_nan; bad = 1; }
    return bad;
}

static uint32_t rng_state = 0x2545F491u;
static uint32_t rng(void) { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 17; rng_state ^= rng_state << 5; return rng_state; }

int main(int argc, char **argv)
{
    const uint64_t stride = argc > 1 ? strtoull(argv[1], 0, 10) : 1;
    const int edges = argc > 2;
    uint64_t bad_t = 0, bad_s = 0, bad_nan = 0, seen = 0, seen_edges = 0, bad_pair = 0;
    if (!stride) return 2;
    tables();
#pragma omp parallel for reduction(+ : bad_t, bad_s, bad_nan, seen) schedule(static)
    for (int64_t chunk = 0; chunk < 4096; ++chunk) {
        for (uint64_t k = (uint64_t)chunk << 20; k < ((uint64_t)chunk + 1) << 20; k += stride) {
            ++seen;
            check((uint32_t)k, &bad_t, &bad_s, &bad_nan);
        }
    }
    if (edges) {
        float pts[2 * 201 + 5];
        int n = 0;
        for (int k = 0; k <= 200; ++k) { pts[n++] = (k - .5f) / 25; pts[n++] = 2 * (k - .5f) / 25; }
        pts[n++] = 0.f; pts[n++] = 8.f; pts[n++] = 8.02f; pts[n++] = 16.f; pts[n++] = 16.04f;
        for (int p = 0; p < n; ++p) {
            uint32_t c;
            memcpy(&c, &pts[p], 4);
            for (int d = -64; d <= 64; ++d)
                for (uint32_t s = 0; s < 2; ++s) {
                    ++seen_edges;
                    check(((c & 0x7fffffffu) + (uint32_t)d) ^ (s << 31), &bad_t, &bad_s, &bad_nan);    /* (below +0: wraps into the NaNs, also fine) */
                }
        }
    }
    /* the two-operand folds: a * tanh(x) with the sign of tanh folded into a */
    for (uint32_t k = 0; k < (1u << 24); ++k) {
        uint32_t ab = rng(), xb = rng();
        if ((k & 15) == 0) ab &= 0x807fffffu;                                    /* subnormal or zero factor */
        if ((k & 15) == 1) xb &= 0x807fffffu;                                    /* subnormal or zero argument */
        if ((k & 15) == 2) xb = (xb & 0x80000000u) | (0x41000000u + (xb & 0x3ffff));    /* at the clamp: 8 .. 8.25 */
        if ((k & 15) == 3) xb = (xb & 0x80000000u) | (0x3ca3d70au - 32 + (xb & 63));    /* around the first boundary, .02 */
        if ((ab & 0x7f800000u) == 0x7f800000u) ab &= ~0x00800000u;               /* finite factors */
        float a, x;
        memcpy(&a, &ab, 4);
        memcpy(&x, &xb, 4);
        const float want = a * tanh_old(x), got = tanh_times_new(a, x);
        if (!same(want, got)) { if (bad_pair < 5) fprintf(stderr, "a * tanh(x) differs at a = %a, x = %a: %a vs %a\n", a, x, want, got); ++bad_pair; }
    }
    printf("patterns visited: %llu (stride %llu) + %llu at the edges; tanh mismatches: %llu, sigmoid mismatches: %llu, NaN lost: %llu; "
           "a * tanh(x) on 2^24 pairs: %llu mismatches\n",
           (unsigned long long)seen, (unsigned long long)stride, (unsigned long long)seen_edges, (unsigned long long)bad_t,
           (unsigned long long)bad_s, (unsigned long long)bad_nan, (unsigned long long)bad_pair);
    return bad_t || bad_s || bad_nan || bad_pair ? 1 : 0;
}
