/* Development aid / proof: the two scalar forms of the sampling-tree walk of the CU-resident sample kernels
 * (csrc/lpcnet_sample_common.h DSS_TREE_WALK_AT) give the same value for every mask of decision bits.
 *
 *   gcc -O2 -o /tmp/tree_walk tools/verify/tree_walk_check.c && /tmp/tree_walk [masks per leaf] [random masks] [seed]
 *
 * Both are restated instruction by instruction, SCC included.  The 256 decision bits are four 64-bit masks: node n of the
 * heap-ordered tree (root 1, children 2n and 2n + 1) is bit n & 63 of mask n >> 6; the walk reads one bit per level, eight
 * levels, and returns the leaf 0..255 (bit 7 decided at the root).
 *   prefix form (24 instructions): val holds the decisions so far WITHOUT the level marker, so the node index is rebuilt
 *     by an s_or_b32 in front of each of levels 1..5;
 *   heap form (19 instructions): n = 1; n = n + n + bit(n).  The sum already is the child's index; s_bitcmp1_b64 takes
 *     only the low six bits of its index, so from level 6 on (n >= 64) n serves as it is; the marker, by then bit 8, comes
 *     off once at the end.
 * Checked: for every leaf, masks whose on-path bits spell the leaf and whose other 248 bits are random -- both forms return
 * the leaf, which is also what a plain walk over the nodes returns; then fully random masks -- the three agree. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

static uint64_t rng_state;
static uint64_t rnd64(void)                      /* splitmix64 */
{
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

/* s_bitcmp1_b64 S0, S1: SCC = S0[S1[5:0]];  s_addc_u32 D, S0, S1: D = S0 + S1 + SCC (the carry out is not used) */
static unsigned bitcmp1_b64(uint64_t s0, uint32_t s1) { return (unsigned)(s0 >> (s1 & 63)) & 1u; }
static uint32_t addc_u32(uint32_t a, uint32_t b, unsigned scc) { return a + b + scc; }

static uint32_t walk_prefix(const uint64_t m[4])
{
    uint32_t val = 0, node;                                                        /* s_mov_b32 val, 0 */
    unsigned scc;
    scc = bitcmp1_b64(m[0], 1);                      val = addc_u32(val, val, scc);
    for (uint32_t marker = 2; marker <= 32; marker <<= 1) {
        node = val | marker;                                                       /* s_or_b32 */
        scc = bitcmp1_b64(m[0], node);               val = addc_u32(val, val, scc);
    }
    scc = bitcmp1_b64(m[1], val);                    val = addc_u32(val, val, scc);
    const uint64_t mm = val < 64 ? m[2] : m[3];                                    /* s_cmp_lt_u32 val, 64; s_cselect_b64 */
    scc = bitcmp1_b64(mm, val);                      val = addc_u32(val, val, scc);
    return val;
}

static uint32_t walk_heap(const uint64_t m[4])
{
    uint32_t n;
    unsigned scc;
    scc = bitcmp1_b64(m[0], 1);                      n = addc_u32(1, 1, scc);      /* level 0: the child of node 1 */
    for (int level = 1; level <= 5; ++level) {
        scc = bitcmp1_b64(m[0], n);                  n = addc_u32(n, n, scc);
    }
    scc = bitcmp1_b64(m[1], n);                      n = addc_u32(n, n, scc);      /* n in 64..127: bit n - 64 of m1 */
    const uint64_t mm = n < 0xc0 ? m[2] : m[3];                                    /* s_cmp_lt_u32 n, 0xc0; s_cselect_b64 */
    scc = bitcmp1_b64(mm, n);                        n = addc_u32(n, n, scc);
    return n & 0xff;                                                               /* s_and_b32 */
}

static uint32_t walk_plain(const uint64_t m[4])
{
    uint32_t n = 1;
    for (int level = 0; level < 8; ++level) n = 2 * n + (uint32_t)((m[n >> 6] >> (n & 63)) & 1);
    return n - 256;
}

int main(int argc, char **argv)
{
    const long per_leaf = argc > 1 ? atol(argv[1]) : 4096, n_random = argc > 2 ? atol(argv[2]) : 1000000;
    rng_state = argc > 3 ? strtoull(argv[3], 0, 10) : 20211;
    unsigned long long bad_leaf = 0, bad_random = 0;
    for (uint32_t leaf = 0; leaf < 256; ++leaf)
        for (long k = 0; k < per_leaf; ++k) {
            uint64_t m[4] = {rnd64(), rnd64(), rnd64(), rnd64()};
            for (uint32_t n = 1, level = 0; level < 8; ++level) {                  /* the path's eight bits spell the leaf */
                const uint64_t bit = (leaf >> (7 - level)) & 1;
                m[n >> 6] = (m[n >> 6] & ~(1ull << (n & 63))) | (bit << (n & 63));
                n = 2 * n + (uint32_t)bit;
            }
            const uint32_t a = walk_prefix(m), b = walk_heap(m), c = walk_plain(m);
            if (a != leaf || b != leaf || c != leaf) {
                if (bad_leaf < 5) fprintf(stderr, "leaf %u: prefix form %u, heap form %u, plain walk %u\n", leaf, a, b, c);
                ++bad_leaf;
            }
        }
    for (long k = 0; k < n_random; ++k) {
        const uint64_t m[4] = {rnd64(), rnd64(), rnd64(), rnd64()};
        const uint32_t a = walk_prefix(m), b = walk_heap(m), c = walk_plain(m);
        if (a != b || a != c) {
            if (bad_random < 5) fprintf(stderr, "random mask %ld: prefix form %u, heap form %u, plain walk %u\n", k, a, b, c);
            ++bad_random;
        }
    }
    printf("leaves x masks: 256 x %ld, mismatches: %llu; random masks: %ld, mismatches: %llu\n", per_leaf, bad_leaf, n_random, bad_random);
    return bad_leaf || bad_random ? 1 : 0;
}
