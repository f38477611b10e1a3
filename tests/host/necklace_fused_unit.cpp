// Host-side check of the fused form of cbl_amd/csrc/necklace.hpp (rotations without a ring mask of their own under an AND, the
// helpers and_or / mask_or / bit_select): necklace_pos_fast and necklace_pos_halves against necklace_pos_naive, rev_comp64 / 128
// against a bit-by-bit reverse complement. Exhaustive on small rings, then the rings of K = 31, 33, 45, 59 on random, sparse,
// periodic and degenerate words and on zero runs around the L = 11 step. Built with -fsanitize=address,undefined and run by
// tests/test_necklace_fused_host.py.
#include "../../cbl_amd/csrc/necklace.hpp"
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
using namespace cblx;

static uint64_t s = 0xC0FFEE;
static uint64_t rnd() { s += 0x9E3779B97F4A7C15ull; uint64_t z = s; z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static nk_u128 rnd128() { return ((nk_u128)rnd() << 64) | rnd(); }
static nk_u128 mask_of(unsigned BITS) { return ((nk_u128)1 << BITS) - 1; }
static nk_u128 rotl(nk_u128 x, unsigned BITS, unsigned p) { p %= BITS; return p ? ((x << p) | (x >> (BITS - p))) & mask_of(BITS) : x; }

static long bad = 0, checked = 0;
static void fail(const char* what, unsigned BITS, nk_u128 x, unsigned got, unsigned want) {
    if (bad++ < 10) fprintf(stderr, "%s mismatch BITS=%u x=%016llx%016llx pos %u, definition %u\n", what, BITS, (unsigned long long)(x >> 64), (unsigned long long)x, got, want);
}
// one word through every function that takes a ring of this width
static void check(nk_u128 x, unsigned BITS) {
    x &= mask_of(BITS);
    nk_u128 want;
    unsigned wp;
    necklace_pos_naive<nk_u128>(x, BITS, want, wp);
    ++checked;
    if (BITS <= 62) {
        uint64_t a;
        unsigned pa;
        necklace_pos_fast<uint64_t>((uint64_t)x, BITS, a, pa);
        if (a != (uint64_t)want || pa != wp) fail("fast<u64>", BITS, x, pa, wp);
    }
    if ((BITS & 1u) == 0) {
        nk_u128 a;
        unsigned pa;
        necklace_pos_halves(x, BITS, a, pa);
        if (a != want || pa != wp) fail("halves", BITS, x, pa, wp);
    }
    nk_u128 a;  // even rings: hands over to the halves; odd ones: the 128-bit ring itself
    unsigned pa;
    necklace_pos_fast<nk_u128>(x, BITS, a, pa);
    if (a != want || pa != wp) fail("fast<u128>", BITS, x, pa, wp);
}

// a run of exactly `len` zeros whose lowest bit is `at` (wrapping round the ring), the other bits taken from `rest`
static nk_u128 zero_run(unsigned BITS, unsigned len, unsigned at, nk_u128 rest) {
    nk_u128 run = rotl(mask_of(len), BITS, at);
    nk_u128 x = (rest & mask_of(BITS)) & ~run;
    if (len < BITS) x |= rotl(1, BITS, at + len);             // a one above the run ...
    if (len + 1 < BITS) x |= rotl(1, BITS, at + BITS - 1);     // ... and one below it
    return x;
}

static void ring(unsigned BITS, long nrandom) {
    const nk_u128 MASK = mask_of(BITS);
    for (long i = 0; i < nrandom; ++i) check(rnd128(), BITS);
    for (long i = 0; i < nrandom / 10; ++i) {  // sparse: 1-3 set bits, and 1-3 clear bits
        nk_u128 x = 0;
        const unsigned n = 1 + (unsigned)(rnd() % 3);
        for (unsigned k = 0; k < n; ++k) x |= (nk_u128)1 << (rnd() % BITS);
        check(x, BITS);
        check(~x, BITS);
    }
    for (unsigned d = 1; d < BITS; ++d) {  // periodic words of every period dividing the ring
        if (BITS % d) continue;
        const long n = d <= 12 ? (1l << d) : 4096;
        for (long i = 0; i < n; ++i) {
            const nk_u128 w = (d <= 12 ? (nk_u128)i : rnd128()) & mask_of(d);
            nk_u128 x = 0;
            for (unsigned b = 0; b < BITS; b += d) x |= w << b;
            check(x, BITS);
        }
    }
    check(0, BITS);
    check(MASK, BITS);
    for (unsigned b = 0; b < BITS; ++b) {
        check(MASK & ~((nk_u128)1 << b), BITS);  // a single zero
        check((nk_u128)1 << b, BITS);            // a single one: a run of BITS - 1 zeros
    }
    const unsigned lens[] = {3, 4, 5, 9, 10, 11, 12, 13, BITS - 2, BITS - 1};
    for (unsigned len : lens) {
        if (len >= BITS) continue;
        for (unsigned at = 0; at < BITS; ++at) {
            check(zero_run(BITS, len, at, MASK), BITS);                                        // alone among ones
            for (int k = 0; k < 8; ++k) {
                const nk_u128 odd = MASK / 3;                                                  // 0101..: no other run of two zeros
                check(zero_run(BITS, len, at, rnd128() | odd), BITS);
                check(zero_run(BITS, len, at, rnd128() | rnd128()), BITS);                     // other runs, mostly shorter
                // a second run of the same length somewhere else: the tie goes to the comparison of the rotations
                const unsigned at2 = (at + len + 1 + (unsigned)(rnd() % BITS)) % BITS;
                check(zero_run(BITS, len, at, rnd128() | odd) & zero_run(BITS, len, at2, MASK), BITS);
            }
        }
    }
}

static void rev_comp_checks() {
    for (unsigned K = 1; K <= 32; ++K)
        for (int i = 0; i < 5000; ++i) {
            uint64_t x = K == 32 ? rnd() : rnd() & ((1ull << (2 * K)) - 1), r = 0, y = x;
            if (i < 4) x = y = (i & 1 ? ~0ull : 0ull) & (K == 32 ? ~0ull : (1ull << (2 * K)) - 1);
            for (unsigned j = 0; j < 2 * K; j += 2) {  // bit by bit: base j / 2 from the bottom goes to the top, complemented (XOR 0b10)
                const uint64_t b0 = (y >> j) & 1, b1 = ((y >> (j + 1)) & 1) ^ 1;
                r |= b0 << (2 * K - 2 - j);
                r |= b1 << (2 * K - 1 - j);
            }
            ++checked;
            if (rev_comp64(x, K) != r && bad++ < 10) fprintf(stderr, "rev_comp64 mismatch K=%u\n", K);
        }
    for (unsigned K = 33; K <= 64; ++K)
        for (int i = 0; i < 3000; ++i) {
            nk_u128 x = rnd128(), r = 0;
            if (K < 64) x &= mask_of(2 * K);
            for (unsigned j = 0; j < 2 * K; j += 2) {
                const nk_u128 b0 = (x >> j) & 1, b1 = ((x >> (j + 1)) & 1) ^ 1;
                r |= b0 << (2 * K - 2 - j);
                r |= b1 << (2 * K - 1 - j);
            }
            ++checked;
            if (rev_comp128(x, K) != r && bad++ < 10) fprintf(stderr, "rev_comp128 mismatch K=%u\n", K);
        }
}

int main() {
    for (unsigned BITS = 6; BITS <= 20; ++BITS)  // every word of every small ring
        for (uint64_t x = 0; x < (1ull << BITS); ++x) check(x, BITS);
    for (unsigned BITS : {62u, 66u, 90u, 118u}) ring(BITS, 1000000);
    for (unsigned BITS : {42u, 50u, 58u}) ring(BITS, 100000);   // K = 21, 25, 29
    for (unsigned BITS : {61u, 67u, 117u}) ring(BITS, 50000);   // odd rings: the 128-bit ring of necklace_pos_fast itself
    rev_comp_checks();
    printf("checked=%ld bad=%ld\n", checked, bad);
    return bad ? 1 : 0;
}
