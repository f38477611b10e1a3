// kernels_gfa.hpp — the links between the unitigs of a compaction, and the GFA 1.0 text of the compacted graph. Both forms: the
// plain unitigs of a non-canonical index (section 6k; `reversed` is null) and the bidirected ones of a canonical index (section 6l).
//   image, slot      unitig u has its kept image, side 0 ('+'), and in the bidirected form the mirror image, side 1 ('-'): the oriented k-mers (i, 1 - s)
//                    in reverse offset order. Slot 2 u + side; in the plain form only even slots hold anything.
//   tail of an image its last oriented k-mer: of the kept image the member at offset length - 1 with s = reversed, of the mirror the kept head with s flipped
//   link             every edge of the graph that does not join two consecutive offsets of one image. It leaves the tail of an image and enters the
//                    head of one, and ALL out-edges of a tail are links: a slot has popcount(out-nibble of its tail) of them, in ascending base code.
//   link table       link_start (CSR over the slots, 2 U + 1 entries), link_to (the target's unitig), link_rev (0: the target is entered at the head of
//                    its kept image, 1: at the head of its mirror)
// Plain C++ HIP. Every output element has one writer: plain vector stores only.
#pragma once
#include "kernels_biunitig.hpp"

namespace cblx {

static const u32 GFA_HEADER_BYTES = 11;  // "H\tVN:Z:1.0\n"

// The out-nibble of oriented k-mer (i, s) from the neighbour mask of stored k-mer i: section 6l's rule — bit c of the out-nibble of (i, 1) is bit
// 4 + (c ^ 2) of the mask.
__device__ __forceinline__ u32 gfa_out_nibble(u32 mk, u32 s) {
    const u32 in4 = mk >> 4;
    return s ? (((in4 & 3u) << 2) | (in4 >> 2)) : (mk & 15u);
}
// decimal digits of v, by comparison with the powers of ten
__device__ __forceinline__ u32 gfa_digits(u32 v) {
    return 1u + (v >= 10u) + (v >= 100u) + (v >= 1000u) + (v >= 10000u) + (v >= 100000u) + (v >= 1000000u) + (v >= 10000000u) + (v >= 100000000u) + (v >= 1000000000u);
}
// v in d = gfa_digits(v) decimal digits at p; returns p + d
__device__ __forceinline__ u8* gfa_put_dec(u8* p, u32 v, u32 d) {
    for (u32 j = d; j-- > 0;) { p[j] = (u8)('0' + v % 10u); v /= 10u; }
    return p + d;
}
// Of a mirror pair of links one is written: the link from slot a to slot b whose pair (a, b) is lexicographically <= its mirror's pair (b ^ 1, a ^ 1).
// With a = b ^ 1 the second components are equal (the link is its own mirror), so the rule is a <= (b ^ 1). The plain form has no mirrors.
__device__ __forceinline__ bool gfa_link_written(bool bi, u64 a, u64 b) { return !bi || a <= (b ^ 1ull); }

// cnt[slot] = the links that leave it; cnt (2 U elements) is zeroed by the caller, so the odd slots of the plain form stay 0. One lane per stored k-mer:
// the tail of the kept image writes cnt[2 u], and in the bidirected form the kept head writes cnt[2 u + 1], the out-degree of its flipped orientation.
__global__ __launch_bounds__(256) void k_gfa_link_counts(const u32* __restrict__ unitig, const u32* __restrict__ offset, const u8* __restrict__ reversed,
                                                          const u32* __restrict__ length, const u8* __restrict__ masks, u64 n, u32* __restrict__ cnt) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 u = unitig[i], off = offset[i], mk = masks[i];
    const u32 rev = reversed ? (u32)(reversed[i] != 0) : 0u;
    if (off + 1u == length[u]) cnt[2ull * u] = (u32)__builtin_popcount(gfa_out_nibble(mk, rev));
    if (reversed && off == 0) cnt[2ull * u + 1ull] = (u32)__builtin_popcount(gfa_out_nibble(mk, rev ^ 1u));
}

// The links of one export pass: QL lanes per (k-mer, side) — work group 2 i + s in the bidirected form, i in the plain one (s = 0). A group whose
// oriented k-mer is not the tail of an image leaves. Otherwise, for every set bit c of the out-nibble in ascending order, y = append(sigma(i, s), c),
// t = whether y is the form that is not stored, r = the ordinal of y's stored form (rank_of_word: all lanes of the group take part), and the first lane
// writes link j of the slot: link_to = unitig[r], link_rev = reversed[r] != t. link_to / link_rev may be null.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_gfa_link_fill(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u8* __restrict__ masks,
                                                        const u32* __restrict__ unitig, const u32* __restrict__ offset, const u8* __restrict__ reversed,
                                                        const u32* __restrict__ length, Consts P, DirView dir, const u64* __restrict__ a_lo,
                                                        const u64* __restrict__ a_hi, const u64* __restrict__ res_off, const u64* __restrict__ link_start,
                                                        u32* __restrict__ link_to, u8* __restrict__ link_rev) {
    const u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / QL;
    const bool bi = reversed != nullptr;
    const u64 i = bi ? g >> 1 : g;
    const u32 s = bi ? (u32)g & 1u : 0u;
    if (i >= m) return;  // whole groups leave together (QL divides the workgroup size)
    const u64 e = e0 + i;
    const u32 u = unitig[e], off = offset[e];  // the group's lanes read the same elements
    const u32 rev = bi ? (u32)(reversed[e] != 0) : 0u;
    const u32 side = s == rev ? 0u : 1u;
    if (side == 0 ? off + 1u != length[u] : off != 0) return;
    const u32 out = gfa_out_nibble(masks[e], s);
    if (out == 0) return;
    typedef typename KmerT<WIDE>::type T;
    T x = (T)k_lo[i];
    if constexpr (WIDE) x |= (T)(k_hi ? k_hi[i] : 0ull) << 64;
    if (s) {
        if constexpr (WIDE) x = rev_comp128(x, P.K); else x = rev_comp64(x, P.K);
    }
    const T MASK = (((T)1) << P.KB) - 1;
    u64 at = link_start[2ull * u + side];
    const bool first = (threadIdx.x & (QL - 1u)) == 0;
    for (u32 o = out; o; o &= o - 1u, ++at) {  // group-uniform
        const T y = ((x << 2) | (T)__builtin_ctz(o)) & MASK;
        const bool t = bi && !kmer_is_fwd<WIDE>(y);
        u64 lo, hi;
        kmer_word<WIDE>(y, P, t, lo, hi);
        const u64 r = rank_of_word(lo, hi, P.SB, P.PB, dir, a_lo, a_hi, res_off);
        if (!first || r == ~0ull) continue;  // (the mask says the successor is there)
        if (link_to) link_to[at] = unitig[r];
        if (link_rev) link_rev[at] = bi ? (u8)((reversed[r] != 0) != t) : (u8)0;
    }
}

// ---- the GFA text: the header, "S\t<u>\t<line u of the unitig text>" for every unitig, then "L\t<u>\t<+|->\t<v>\t<+|->\t<K - 1>M\n" for every link that
// is written, in table order. bytes[u] of an S line: its prefix, the K + length[u] - 1 letters and the '\n'.
__global__ __launch_bounds__(256) void k_gfa_s_bytes(const u32* __restrict__ length, u64 nu, u32 K, u32* __restrict__ bytes) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nu) bytes[u] = 3u + gfa_digits((u32)u) + K + length[u];
}
// In place over base[u], the exclusive scan of k_gfa_s_bytes: the prefix of S line u is written at text + origin + base[u], and base[u] becomes the offset
// in `text` of the line's letters, which k_unitig_text / k_biunitig_text write. The first lane also writes the header (the grid has it when nu = 0).
__global__ __launch_bounds__(256) void k_gfa_s_prefix(u64* base, u64 nu, u64 origin, u8* __restrict__ text) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u == 0) {
        const u64 h0 = 0x2E313A5A3A4E5609ull;  // "\tVN:Z:1." little-endian
        text[0] = 'H';
        for (u32 j = 0; j < 8; ++j) text[1 + j] = (u8)(h0 >> (8u * j));
        text[9] = '0';
        text[10] = '\n';
    }
    if (u >= nu) return;
    const u64 at = origin + base[u];
    u8* p = text + at;
    const u32 d = gfa_digits((u32)u);
    p[0] = 'S';
    p[1] = '\t';
    p = gfa_put_dec(p + 2, (u32)u, d);
    p[0] = '\t';
    base[u] = at + 3u + d;
}
// One lane per slot: bytes[slot] = the bytes of the L lines of its links and lines[slot] = how many they are; a link whose mirror is written counts 0.
__global__ __launch_bounds__(256) void k_gfa_l_bytes(const u64* __restrict__ link_start, const u32* __restrict__ link_to, const u8* __restrict__ link_rev, u64 nslots,
                                                      bool bi, u32 K1, u32* __restrict__ bytes, u32* __restrict__ lines) {
    const u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= nslots) return;
    const u32 fixed = 10u + gfa_digits(K1) + gfa_digits((u32)(a >> 1));
    u32 b = 0, ln = 0;
    for (u64 l = link_start[a], end = link_start[a + 1]; l < end; ++l) {
        const u32 v = link_to[l];
        if (!gfa_link_written(bi, a, 2ull * v + link_rev[l])) continue;
        b += fixed + gfa_digits(v);
        ++ln;
    }
    bytes[a] = b;
    lines[a] = ln;
}
// One lane per slot: the L lines of its links from text + origin + base[slot] (the exclusive scan of k_gfa_l_bytes)
__global__ __launch_bounds__(256) void k_gfa_l_text(const u64* __restrict__ link_start, const u32* __restrict__ link_to, const u8* __restrict__ link_rev,
                                                     const u64* __restrict__ base, u64 nslots, bool bi, u32 K1, u64 origin, u8* __restrict__ text) {
    const u64 a = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (a >= nslots) return;
    const u32 u = (u32)(a >> 1), du = gfa_digits(u), dk = gfa_digits(K1);
    u8* p = text + origin + base[a];
    for (u64 l = link_start[a], end = link_start[a + 1]; l < end; ++l) {
        const u32 v = link_to[l], r = link_rev[l];
        if (!gfa_link_written(bi, a, 2ull * v + r)) continue;
        p[0] = 'L';
        p[1] = '\t';
        p = gfa_put_dec(p + 2, u, du);
        p[0] = '\t';
        p[1] = (a & 1ull) ? '-' : '+';
        p[2] = '\t';
        p = gfa_put_dec(p + 3, v, gfa_digits(v));
        p[0] = '\t';
        p[1] = r ? '-' : '+';
        p[2] = '\t';
        p = gfa_put_dec(p + 3, K1, dk);
        p[0] = 'M';
        p[1] = '\n';
        p += 2;
    }
}

}  // namespace cblx
