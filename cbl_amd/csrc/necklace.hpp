// necklace.hpp — k-mer -> (necklace, pos) word transform, usable from device and host code.
//
// Definition (normative, /root/reference/src/necklace/mod.rs:13-25): necklace = min over p in [0, BITS) of
// rotl_BITS(x, p), pos = the SMALLEST p attaining it; word = necklace << POS_BITS | pos
// (/root/reference/src/cbl.rs:181-184). The reference's streaming NecklaceQueue
// (src/necklace/queue.rs) returns the same pair; a GPU lane per k-mer has no use for the queue.
//
// Method (ours): the minimal rotation must start at the top of a LONGEST cyclic run of zero bits. Runs are
// found with r <- r & rotl(r, 1) (r starts as ~x): after L-1 steps bit s of r says "bits s, s-1, .., s-L+1 of x
// are all zero". The last non-zero r marks the tops of the longest runs; only those candidates (usually 1-2)
// are compared, highest s (= smallest p) first with a strict '<' so ties keep the smallest p.
// ~100-200 integer ops per k-mer instead of BITS full-width rotate+compare steps.
#pragma once
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cblx {

typedef unsigned __int128 nk_u128;

template <typename T> struct NkBits;
template <> struct NkBits<uint64_t> {
    static __host__ __device__ inline int clz(uint64_t v) { return __builtin_clzll(v); }
};
template <> struct NkBits<nk_u128> {
    static __host__ __device__ inline int clz(nk_u128 v) {
        uint64_t hi = (uint64_t)(v >> 64);
        return hi ? __builtin_clzll(hi) : 64 + __builtin_clzll((uint64_t)v);
    }
};

// Three-input bit operations. The necklace's logic is written on 64-bit words; the compiler splits a 64-bit `or` / `and` into 32-bit
// halves and only then looks for three-input patterns, after they are gone — so on gfx950 the helpers hand the halves to
// v_bitop3_b32 themselves. Its truth table is the formula evaluated on 0xF0, 0xCC, 0xAA for its first, second and third operand.
// A half whose mask is known to be all ones when the code is compiled stays a plain OR: v_bitop3_b32 issues at the rate of a shift
// (4.4 cycles per wave, tools/dev_valu_rate.cpp), an OR or AND of two registers in 2.5. Everywhere else (host, other targets) the
// helpers are the plain expression.
#if defined(__HIP_DEVICE_COMPILE__) && defined(__gfx950__) && defined(__has_builtin)
#if __has_builtin(__builtin_amdgcn_bitop3_b32)
#define CBLX_NK_BITOP3 1
#endif
#endif
#ifdef CBLX_NK_BITOP3
__device__ inline uint64_t nk_join(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }
__device__ inline uint32_t nk_and_or32(uint32_t a, uint32_t b, uint32_t c) {
    if (__builtin_constant_p(c) && c == 0xFFFFFFFFu) return a | b;
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0xA8);  // (0xF0 | 0xCC) & 0xAA
}
__device__ inline uint32_t nk_mask_or32(uint32_t a, uint32_t m, uint32_t b) {
    if (__builtin_constant_p(m) && m == 0xFFFFFFFFu) return a | b;
    return __builtin_amdgcn_bitop3_b32(a, m, b, 0xEA);  // (0xF0 & 0xCC) | 0xAA
}
__device__ inline uint32_t nk_select32(uint32_t m, uint32_t a, uint32_t b) {
    return __builtin_amdgcn_bitop3_b32(m, a, b, 0xCA);  // (0xCC & 0xF0) | (0xAA & ~0xF0)
}
__device__ inline uint64_t and_or(uint64_t a, uint64_t b, uint64_t c) {  // (a | b) & c
    return nk_join(nk_and_or32((uint32_t)(a >> 32), (uint32_t)(b >> 32), (uint32_t)(c >> 32)), nk_and_or32((uint32_t)a, (uint32_t)b, (uint32_t)c));
}
__device__ inline uint64_t mask_or(uint64_t a, uint64_t m, uint64_t b) {  // (a & m) | b
    return nk_join(nk_mask_or32((uint32_t)(a >> 32), (uint32_t)(m >> 32), (uint32_t)(b >> 32)), nk_mask_or32((uint32_t)a, (uint32_t)m, (uint32_t)b));
}
__device__ inline uint64_t bit_select(uint64_t m, uint64_t a, uint64_t b) {  // (a & m) | (b & ~m)
    return nk_join(nk_select32((uint32_t)(m >> 32), (uint32_t)(a >> 32), (uint32_t)(b >> 32)), nk_select32((uint32_t)m, (uint32_t)a, (uint32_t)b));
}
#else
__host__ __device__ inline uint64_t and_or(uint64_t a, uint64_t b, uint64_t c) { return (a | b) & c; }
__host__ __device__ inline uint64_t mask_or(uint64_t a, uint64_t m, uint64_t b) { return (a & m) | b; }
__host__ __device__ inline uint64_t bit_select(uint64_t m, uint64_t a, uint64_t b) { return (a & m) | (b & ~m); }
#endif
// (the 128-bit ring of necklace_pos_fast: only words with an odd number of bits stay on it, which no k-mer has)
__host__ __device__ inline nk_u128 and_or(nk_u128 a, nk_u128 b, nk_u128 c) { return (a | b) & c; }
__host__ __device__ inline nk_u128 mask_or(nk_u128 a, nk_u128 m, nk_u128 b) { return (a & m) | b; }

// The same method for a ring of 2H bits (a k-mer of K = H bases wider than 64 bits) kept as TWO 64-bit halves of H bits each: a
// rotation by s < H is hi' = (hi << s | lo >> (H - s)) & M, lo' = (lo << s | hi >> (H - s)) & M — four 64-bit shifts and four
// logic operations — and one by s >= H swaps the halves first; on a 128-bit integer the compiler needs six shifts and more glue per
// rotation (every shift costs 1.7 logic operations on this part, tools/dev_valu_rate.cpp). Steps and tie rule are those of
// necklace_pos_fast below, which hands wide words with an even number of bits over to this function.
__host__ __device__ inline void necklace_pos_halves(nk_u128 x, unsigned BITS, nk_u128& necklace, unsigned& pos) {
    const unsigned H = BITS >> 1;  // < 64
    const uint64_t M = (1ull << H) - 1;
    const uint64_t xh = (uint64_t)(x >> H) & M, xl = (uint64_t)x & M;
    if ((xh | xl) == 0 || (xh & xl) == M) {  // single-symbol words: every rotation equal, smallest p = 0
        necklace = x;
        pos = 0;
        return;
    }
    // (oh, ol) = rotl(h:l, s) & (mh:ml) on the ring, 0 <= s <= BITS, for h, l, mh, ml <= M (0 and BITS are the identity: b >> H is 0
    // and the bits a << t puts above M vanish under the mask). The shifted parts carry no mask of their own. With mh = ml = M this is
    // the rotation itself; the run-finding steps pass the run mask they AND the rotation with anyway, which is within M.
    // rot_and: the wrap OR and the AND as one three-input operation per 32 bits (the shifts by a variable).
    // rot_and_c: the constant steps 1, 2, 4 — the two parts are disjoint, so their OR is a sum, which folds into the left shift
    // (v_lshl_add_u64 takes shifts up to 4); handed to the three-input helper instead, the 64-bit shift falls apart into three 32-bit ones.
    auto rot_and = [&](uint64_t h, uint64_t l, unsigned s, uint64_t mh, uint64_t ml, uint64_t& oh, uint64_t& ol) {
        const bool sw = s >= H;
        const unsigned t = sw ? s - H : s;
        const uint64_t a = sw ? l : h, b = sw ? h : l;
        oh = and_or(a << t, b >> (H - t), mh);
        ol = and_or(b << t, a >> (H - t), ml);
    };
    auto rot_and_c = [&](uint64_t h, uint64_t l, unsigned s, uint64_t mh, uint64_t ml, uint64_t& oh, uint64_t& ol) {
        const bool sw = s >= H;
        const unsigned t = sw ? s - H : s;
        const uint64_t a = sw ? l : h, b = sw ? h : l;
        oh = ((a << t) + (b >> (H - t))) & mh;
        ol = ((b << t) + (a >> (H - t))) & ml;
    };
    uint64_t rh = ~xh & M, rl = ~xl & M, th, tl;  // invariant: rh, rl <= M from here on
    unsigned L = 1;
    {
        uint64_t r2h, r2l, r4h, r4l;
        rot_and_c(rh, rl, 1, rh, rl, r2h, r2l);      // runs >= 2
        rot_and_c(r2h, r2l, 2, r2h, r2l, r4h, r4l);  // runs >= 4
        if (r4h | r4l) {
            rh = r4h; rl = r4l; L = 4;
            rot_and_c(rh, rl, 4, rh, rl, th, tl); if (th | tl) { rh = th; rl = tl; L += 4; }
            rot_and_c(rh, rl, 2, rh, rl, th, tl); if (th | tl) { rh = th; rl = tl; L += 2; }
        } else if (r2h | r2l) {
            rh = r2h; rl = r2l; L = 2;
        }
    }
    {
        rot_and_c(rh, rl, 1, rh, rl, th, tl);
        if (th | tl) { rh = th; rl = tl; ++L; }
        if (L == 11) {
            for (;;) {
                rot_and_c(rh, rl, 1, rh, rl, th, tl);
                if ((th | tl) == 0) break;
                rh = th; rl = tl;
                ++L;
            }
        }
    }
    {
        rot_and(~xh & M, ~xl & M, L + 1, rh, rl, th, tl);
        if (th | tl) { rh = th; rl = tl; }
    }
    uint64_t bh = M, bl = M;
    unsigned bestp = 0;
    bool first = true;
    while (rh | rl) {
        unsigned s;  // highest remaining candidate
        // (bit b is set: the XOR clears it, in one instruction per 32 bits where AND-NOT of the shifted bit takes a three-input one)
        if (rh) { const unsigned b = 63u - (unsigned)__builtin_clzll(rh); rh ^= 1ull << b; s = H + b; }
        else { const unsigned b = 63u - (unsigned)__builtin_clzll(rl); rl ^= 1ull << b; s = b; }
        const unsigned p = BITS - 1 - s;
        rot_and(xh, xl, p, M, M, th, tl);
        if (first || th < bh || (th == bh && tl < bl)) {
            bh = th; bl = tl;
            bestp = p;
            first = false;
        }
    }
    necklace = ((nk_u128)bh << H) | bl;
    pos = bestp;
}

// x must already be masked to BITS bits, BITS < 8 * sizeof(T). T = uint64_t (BITS <= 62) or nk_u128 (BITS <= 118).
template <typename T> __host__ __device__ inline void necklace_pos_fast(T x, unsigned BITS, T& necklace, unsigned& pos) {
    if constexpr (sizeof(T) == 16) {
        if ((BITS & 1u) == 0 && BITS < 128) {
            nk_u128 nk;
            necklace_pos_halves((nk_u128)x, BITS, nk, pos);
            necklace = (T)nk;
            return;
        }
    }
    const T MASK = (BITS >= sizeof(T) * 8) ? ~(T)0 : ((((T)1) << BITS) - 1);
    if (x == 0 || x == MASK) {  // single-symbol words: every rotation equal, smallest p = 0
        necklace = x;
        pos = 0;
        return;
    }
    // rotl by s on the BITS-bit ring (0 < s <= BITS) is (up & MASK) | dn of the two shifted parts; up keeps what it shifted past the
    // top of the ring.
    auto up = [&](T v, unsigned s) -> T { return v << s; };
    auto dn = [&](T v, unsigned s) -> T { return v >> (BITS - s); };
    // m & rotl(v, s) for v <= MASK and a mask m <= MASK: the AND clears what up left above the ring, so the rotation needs no ring mask
    // of its own. Every run mask r below satisfies r <= MASK: it starts as ~x & MASK and only ever loses bits.
    // and_rotl: the wrap OR and the AND as one three-input operation per 32 bits (the shift by a variable).
    // and_rotl_c: the constant steps 1, 2, 4 — up and dn are disjoint, so their OR is a sum, which folds into the left shift
    // (v_lshl_add_u64 takes shifts up to 4); handed to the three-input helper instead, the 64-bit shift falls apart into three 32-bit ones.
    auto and_rotl = [&](T m, T v, unsigned s) -> T { return and_or(up(v, s), dn(v, s), m); };
    auto and_rotl_c = [&](T m, T v, unsigned s) -> T { return m & (up(v, s) + dn(v, s)); };
    T r = ~x & MASK;  // bit s: x has a zero at s                       (runs >= 1)
    unsigned L = 1;   // length of the runs r marks
    {   // Doubling, then a greedy binary refinement: with R_L = "a run of >= L zeros ends (downwards) at bit s",
        // R_{L+d} = R_L & rotl(R_L, d) for d <= L. Every lane of a wave executes the same few steps (a lane-dependent
        // linear search cost every lane the length of the longest run in the wave).
        const T r2 = and_rotl_c(r, r, 1);     // runs >= 2
        const T r4 = and_rotl_c(r2, r2, 2);   // runs >= 4
        if (r4) {
            r = r4;                                            // L = 4
            L = 4;
            T t = and_rotl_c(r, r, 4); if (t) { r = t; L += 4; }    // L in {4, 8}
            t = and_rotl_c(r, r, 2); if (t) { r = t; L += 2; }      // L in {4, 6, 8, 10}
        } else if (r2) {
            r = r2;                                            // L in {2, 3}
            L = 2;
        }
    }
    {   // One +1 step settles every case but one: the doubling above left L in {1, 2, 4, 6, 8, 10} with the longest run known
        // to be < L + 2 unless L = 10 (L = 1: no run of 2 at all, the step is a no-op), so a second step can only succeed
        // after 10 -> 11. (A plain loop paid one extra rotate-and-test per k-mer to find that out.)
        T t = and_rotl_c(r, r, 1);
        if (t != 0) { r = t; ++L; }
        if (L == 11) {
            for (;;) {
                t = and_rotl_c(r, r, 1);
                if (t == 0) break;
                r = t;
                ++L;
            }
        }
    }
    {   // Every candidate reads 0^L 1 from its top; the next bit decides next: keep only the candidates that continue with
        // a 0, if there are any (a cheap mask operation that saves a round of the rotate-and-compare loop below for the
        // slowest lane of most waves).
        const T z = ~x & MASK;
        const T t = and_rotl(r, z, L + 1);  // L + 1 <= BITS; a rotation by BITS is the identity here (up(z, BITS) lies above the ring)
        r = t ? t : r;
    }
    constexpr int TB = (int)sizeof(T) * 8;
    T best = MASK;
    unsigned bestp = 0;
    bool first = true;
    while (r != 0) {
        int s = TB - 1 - NkBits<T>::clz(r);  // highest remaining candidate
        r ^= ((T)1) << s;  // bit s is set: the XOR clears it (one instruction per 32 bits; AND-NOT of the shifted bit takes a three-input one)
        unsigned p = BITS - 1 - (unsigned)s;
        // BITS < bit width of T (K is odd): p = 0 shifts right by BITS, which leaves 0 of the masked x
        T rot = mask_or(up(x, p), MASK, dn(x, p));  // the rotation's value itself is used: the ring mask stays, folded into the OR
        if (first || rot < best) {
            best = rot;
            bestp = p;
            first = false;
        }
    }
    necklace = best;
    pos = bestp;
}

// The definition, verbatim in spirit (used by tests and as a debug variant).
template <typename T> __host__ __device__ inline void necklace_pos_naive(T x, unsigned BITS, T& necklace, unsigned& pos) {
    T nk = x, rot = x;
    unsigned p = 0;
    for (int i = (int)BITS - 1; i >= 0; --i) {
        rot = ((rot & 1) << (BITS - 1)) | (rot >> 1);
        if (rot <= nk) { nk = rot; p = (unsigned)i; }
    }
    necklace = nk;
    pos = p;
}

// Reverse complement of a K-base packed k-mer (/root/reference/src/kmer.rs:293-348; code A=0 C=1 T=2 G=3, so
// complement = XOR 0b10): reverse the 2-bit groups, complement each, drop the 2*(W/2-K) pad bits.
__host__ __device__ inline uint64_t rev_comp64(uint64_t x, unsigned K) {
    uint64_t r = x;
    // swap level s under mask m (m << s == ~m): ((r >> s) & m) | ((r & m) << s) == select by m between r >> s and r << s
    r = bit_select(0x3333333333333333ull, r >> 2, r << 2);
    r = bit_select(0x0F0F0F0F0F0F0F0Full, r >> 4, r << 4);
    r = __builtin_bswap64(r);
    r ^= 0xAAAAAAAAAAAAAAAAull;
    return r >> (2 * (32 - K));
}
__host__ __device__ inline nk_u128 rev_comp128(nk_u128 x, unsigned K) {
    uint64_t lo = (uint64_t)x, hi = (uint64_t)(x >> 64);
    // reverse all 64 groups of the 128-bit value: swap halves, reverse groups inside each
    uint64_t rlo = rev_comp64(hi, 32), rhi = rev_comp64(lo, 32);
    nk_u128 r = ((nk_u128)rhi << 64) | rlo;
    return r >> (2 * (64 - K));
}

__host__ __device__ inline unsigned popcount128(nk_u128 x) {
    return (unsigned)__builtin_popcountll((uint64_t)x) + (unsigned)__builtin_popcountll((uint64_t)(x >> 64));
}

// nucleotide code (/root/reference/src/kmer.rs:11-24): A/a=0 C/c=1 T/t=2 G/g=3, anything else invalid (skipped).
// For the 8 valid bytes the code is (b >> 1) & 3.
__host__ __device__ inline bool nuc_valid(uint8_t b) {
    uint8_t u = b & 0xDF;  // upper-case
    return u == 'A' || u == 'C' || u == 'G' || u == 'T';
}
__host__ __device__ inline unsigned nuc_code(uint8_t b) { return (b >> 1) & 3u; }

}  // namespace cblx
