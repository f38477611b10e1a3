// kernels_biunitig.hpp — bidirected unitigs: the unitigs of a CANONICAL index with odd K. Stored k-mer i (ordinal i, x_i the
// form kmer_is_fwd accepts) has two oriented copies: (i, 0) spells x_i and (i, 1) spells rc(x_i); the id of (i, s) is v = 2 i + s, its mirror 2 i + 1 - s.
//   edge (i, s) -> (j, t)   sigma(j, t) = append(sigma(i, s), c) with x_j in the set; its mirror (j, 1 - t) -> (i, 1 - s) is an edge too
//   degrees                 from the neighbour mask m_i of section 6j alone: out(i, 0) = popcount(m & 15), in(i, 0) = popcount(m >> 4),
//                           out(i, 1) = in(i, 0), in(i, 1) = out(i, 0); bit c of the out-nibble of (i, 1) is bit 4 + (c ^ 2) of m
//   simple                  out(i, s) = 1, in(j, t) = 1 and j != i: an edge between a stored k-mer and itself (the hairpin (i, s) -> (i, 1 - s), the
//                           homopolymer loop) is never simple, though it counts in the degrees — unlike section 6k, poly-A alone is not circular
// next / prev, list ranking and the cycle cut are section 6k's kernels (kernels_unitig.hpp) on arrays of 2 n ids. What is new: the links on oriented
// k-mers, the choice of one of each unitig's two mirror images, and the text with reverse-complemented members. Plain C++ HIP, plain vector stores.
#pragma once
#include "kernels_unitig.hpp"

namespace cblx {

// The links of one export pass: QL lanes per (k-mer, side), work group 2 i + s of the pass. A group whose oriented k-mer has not exactly one
// successor does no look-up. Otherwise z = sigma(i, s), y = append(z, c), t = whether y is the form that is not stored, r = the ordinal of y's stored
// form; the edge is dropped when r is i itself or when (r, t) has not exactly one predecessor. prev[2 r + t] has one writer — the one oriented
// predecessor of (r, t) — and the mirror edge is written by the group of (r, 1 - t): plain stores. next / prev are filled with UNITIG_NONE by the caller.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_biunitig_links(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u8* __restrict__ masks, Consts P,
                                                         DirView dir, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, const u64* __restrict__ res_off,
                                                         u32* __restrict__ next, u32* __restrict__ prev) {
    const u64 g = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / QL;
    const u64 i = g >> 1;
    const u32 s = (u32)g & 1u;
    if (i >= m) return;  // whole groups leave together (QL divides the workgroup size)
    const u32 mk = masks[e0 + i];  // the group's lanes read the same byte
    const u32 in4 = mk >> 4;
    const u32 out = s ? (((in4 & 3u) << 2) | (in4 >> 2)) : (mk & 15u);
    if (__builtin_popcount(out) != 1) return;
    typedef typename KmerT<WIDE>::type T;
    T x = (T)k_lo[i];
    if constexpr (WIDE) x |= (T)(k_hi ? k_hi[i] : 0ull) << 64;
    if (s) {
        if constexpr (WIDE) x = rev_comp128(x, P.K); else x = rev_comp64(x, P.K);
    }
    const T MASK = (((T)1) << P.KB) - 1;
    const T y = ((x << 2) | (T)__builtin_ctz(out)) & MASK;
    const bool t = !kmer_is_fwd<WIDE>(y);
    u64 lo, hi;
    kmer_word<WIDE>(y, P, t, lo, hi);
    const u64 r = rank_of_word(lo, hi, P.SB, P.PB, dir, a_lo, a_hi, res_off);
    if ((threadIdx.x & (QL - 1u)) != 0 || r == ~0ull) return;  // (the mask says the successor is there)
    if (r == e0 + i) return;  // a stored k-mer and itself: never simple
    const u32 mr = masks[r];
    if (__builtin_popcount(t ? (mr & 15u) : (mr >> 4)) != 1) return;
    const u32 v = (u32)(2u * (e0 + i)) + s, w = (u32)(2u * r) + (t ? 1u : 0u);
    next[v] = w;
    prev[w] = v;
}

// ---- the choice of an image. After the ranking every id has anc = its head and dist = its offset; a path and its mirror, and a cut cycle and its
// mirror, are both there. tail[h] = the id without a simple out-edge whose head is h: one writer per head.
__global__ __launch_bounds__(256) void k_biunitig_tails(const u32* __restrict__ anc, const u32* __restrict__ next, u64 n2, u32* __restrict__ tail) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n2) return;
    if (next[v] == UNITIG_NONE) tail[anc[v]] = (u32)v;
}
// In place over `tail`: is_head[v] = 1 where v is the head of the image that is kept, 0 everywhere else (a lane reads and writes its own element).
//   path    head (h, s), tail (t, u): kept when h < t, or h = t and s = 0 (length 1; a longer path never holds both copies of a stored k-mer)
//   cycle   both images were cut in front of the same stored k-mer, the smallest ordinal: kept when that head has s = 0
__global__ __launch_bounds__(256) void k_biunitig_keep(const u32* __restrict__ prev, const u8* __restrict__ circular, u64 n2, u32* tail_is_head) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n2) return;
    u32 keep = 0;
    if (prev[v] == UNITIG_NONE) {
        const u32 h = (u32)v >> 1, s = (u32)v & 1u, t = tail_is_head[v] >> 1;
        keep = circular[v] ? (s == 0) : (h < t || (h == t && s == 0));
    }
    tail_is_head[v] = keep;
}
// Every output may be null. An id whose head is kept writes unitig / offset / reversed of its stored k-mer v >> 1 — each stored k-mer lies on exactly
// one kept image, so each is written once; the head writes head[u] and flags[u], the tail writes length[u].
__global__ __launch_bounds__(256) void k_biunitig_number(const u32* __restrict__ anc, const u32* __restrict__ dist, const u32* __restrict__ next, const u32* __restrict__ is_head,
                                                          const u32* __restrict__ uid, const u8* __restrict__ circular, u64 n2, u32* __restrict__ unitig,
                                                          u32* __restrict__ offset, u8* __restrict__ reversed, u32* __restrict__ head, u32* __restrict__ length,
                                                          u8* __restrict__ flags) {
    const u64 v = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n2) return;
    const u32 h = anc[v];
    if (!is_head[h]) return;
    const u32 d = dist[v], u = uid[h];
    const u64 i = v >> 1;
    if (unitig) unitig[i] = u;
    if (offset) offset[i] = d;
    if (reversed) reversed[i] = (u8)(v & 1u);
    if (h == (u32)v) {
        if (head) head[u] = (u32)i;
        if (flags) flags[u] = circular[v];
    }
    if (length && next[v] == UNITIG_NONE) length[u] = d + 1u;
}

// ---- text: k_unitig_text's layout — line u = the K letters of sigma(head), the last letter of sigma of every following member in offset order, '\n':
// K + length[u] bytes from base[u]. A reversed head is written as its reverse complement; the last letter of a reversed member is the complement
// of its stored form's first base. One lane per stored k-mer of an export pass.
__global__ __launch_bounds__(256) void k_biunitig_text(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u32* __restrict__ unitig,
                                                        const u32* __restrict__ offset, const u8* __restrict__ reversed, const u32* __restrict__ length,
                                                        const u64* __restrict__ base, u32 K, u8* __restrict__ text) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const u32 u = unitig[e0 + i], off = offset[e0 + i];
    const bool rev = reversed[e0 + i] != 0;
    u8* const line = text + base[u];
    u128 x = (u128)k_lo[i];
    if (k_hi) x |= (u128)k_hi[i] << 64;
    if (off == 0) {
        if (rev) x = rev_comp128(x, K);
        for (u32 j = 0; j < K; ++j) line[j] = (u8)((0x47544341u >> (8u * ((u32)(x >> (2u * (K - 1u - j))) & 3u))) & 0xFFu);  // b"ACTG"[code], first base first
    } else {
        const u32 code = rev ? (((u32)(x >> (2u * (K - 1u))) & 3u) ^ 2u) : ((u32)x & 3u);
        line[K - 1u + off] = (u8)((0x47544341u >> (8u * code)) & 0xFFu);
    }
    if (off + 1u == length[u]) line[K + off] = '\n';
}

}  // namespace cblx
