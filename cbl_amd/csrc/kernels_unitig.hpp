// kernels_unitig.hpp — unitigs of the de Bruijn graph whose nodes are the k-mers of a non-canonical index:
// the rank of a k-mer (the inverse of the iteration order), the links that the ranks of the one-successor k-mers make, list
// ranking over those links by pointer jumping, the cut of the pure cycles, numbering, and the text of the unitigs.
//   edge x -> y     y = append(x, c), both in the set; simple when out(x) = 1 and in(y) = 1 (degrees of the neighbour masks, section 6j)
//   next[i] / prev[i]  the ordinal at the other end of i's simple out- / in-edge, UNITIG_NONE where it has none
// Plain C++ HIP; the only atomics are the counters that are read back (unfinished k-mers per round, circular unitigs).
#pragma once
#include "kernels_graph.hpp"

namespace cblx {

static const u32 UNITIG_NONE = 0xFFFFFFFFu;

// The ordinal of a word in the iteration order, ~0 when the index does not hold it; the QL lanes of a group share the query and all
// return the same value. The search is k_contains': a Vec bucket is scanned QL suffixes per step, a Trie bucket by a (QL + 1)-ary
// search; where k_contains raises a flag, the position j of the match in its bucket r gives res_off[r] + j (a Trie bucket is stored
// ascending and a Vec bucket in first-occurrence order, which is the order k_export_range reads them in).
__device__ __forceinline__ u64 rank_of_word(u64 lo, u64 hi, u32 SB, u32 PB, const DirView& dir, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi,
                                            const u64* __restrict__ res_off) {
    const u32 lane = threadIdx.x & 63u, sub = lane & (QL - 1u), gsh = lane & ~(QL - 1u);
    const u32 p = get_bits(lo, hi, SB, PB);
    u64 r;
    if (!dir_lookup(dir, p, r)) return ~0ull;
    const u128 M = (((u128)1) << SB) - 1;
    const u128 key = (((u128)hi << 64) | lo) & M;
    const u64 s0 = dir.start[r];
    const u32 c = dir.count[r];
    auto at = [&](u32 j) -> u128 {
        u128 v = a_lo[s0 + j];
        if (a_hi) v |= (u128)a_hi[s0 + j] << 64;
        return v & M;
    };
    u32 l = 0, h = c;  // candidates [l, h)
    if (dir.kind[r] == KIND_TRIE) {
        while (h - l > QL) {  // group-uniform
            const u32 width = h - l;
            const u32 m = l + (u32)(((u64)(sub + 1u) * width) / (QL + 1u));  // l < m < h, ascending in sub
            const bool less = at(m) < key;
            const u32 cnt = (u32)__builtin_popcountll((__ballot(less) >> gsh) & ((1ull << QL) - 1ull));
            const u32 nl = cnt ? l + (u32)(((u64)cnt * width) / (QL + 1u)) + 1u : l;
            const u32 nh = cnt < QL ? l + (u32)(((u64)(cnt + 1u) * width) / (QL + 1u)) + 1u : h;
            l = nl;
            h = nh;
        }
    }
    for (u32 j0 = l; j0 < h; j0 += QL) {  // group-uniform trip count
        const u32 j = j0 + sub;
        const u32 hit = (u32)((__ballot(j < h && at(j) == key) >> gsh) & ((1ull << QL) - 1ull));
        if (hit) return res_off[r] + j0 + (u32)__builtin_ctz(hit);  // a set holds a word once: one bit
    }
    return ~0ull;
}

// rank[i] = the ordinal of word i, ~0 when absent: k_contains with a position where that has a flag
template <typename HiT>
__global__ __launch_bounds__(256) void k_rank(const u64* __restrict__ w_lo, const HiT* __restrict__ w_hi, u64 n, u32 SB, u32 PB, DirView dir, const u64* __restrict__ a_lo,
                                               const u64* __restrict__ a_hi, const u64* __restrict__ res_off, u64* __restrict__ rank) {
    const u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / QL;
    if (i >= n) return;  // whole groups leave together (QL divides the workgroup size)
    const u64 r = rank_of_word(w_lo[i], ld_hi<HiT>(w_hi, i), SB, PB, dir, a_lo, a_hi, res_off);
    if ((threadIdx.x & (QL - 1u)) == 0) rank[i] = r;
}

// The links of one export pass: k-mer i of the pass has ordinal e0 + i and neighbour mask masks[e0 + i]. A k-mer with exactly one successor
// forms it, looks up its ordinal r (QL lanes, as k_rank) and, where that successor has exactly one predecessor, the edge is simple:
// next[e0 + i] = r and prev[r] = e0 + i. Every other k-mer does no look-up. next / prev are filled with UNITIG_NONE by the caller. prev[r] has
// one writer — the one predecessor of r — so these are plain stores.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_unitig_links(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u8* __restrict__ masks, Consts P,
                                                       DirView dir, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, const u64* __restrict__ res_off,
                                                       u32* __restrict__ next, u32* __restrict__ prev) {
    const u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / QL;
    if (i >= m) return;
    const u32 out = masks[e0 + i] & 15u;
    if (__builtin_popcount(out) != 1) return;  // the group's lanes read the same byte
    typedef typename KmerT<WIDE>::type T;
    T x = (T)k_lo[i];
    if constexpr (WIDE) x |= (T)(k_hi ? k_hi[i] : 0ull) << 64;
    const T MASK = (((T)1) << P.KB) - 1;
    const T y = ((x << 2) | (T)__builtin_ctz(out)) & MASK;
    u64 lo, hi;
    kmer_word<WIDE>(y, P, false, lo, hi);
    const u64 r = rank_of_word(lo, hi, P.SB, P.PB, dir, a_lo, a_hi, res_off);
    if ((threadIdx.x & (QL - 1u)) != 0 || r == ~0ull) return;  // (the mask says the successor is there)
    if (__builtin_popcount((u32)masks[r] >> 4) != 1) return;
    next[e0 + i] = (u32)r;
    prev[r] = (u32)(e0 + i);
}

// ---- list ranking by pointer jumping. State of k-mer i: anc[i], an ancestor along the simple in-edges, and dist[i], the simple edges
// between the two. A head has anc = itself and dist = 0; every other k-mer has dist >= 1, so "a is a head" is dist[a] == 0 and costs no
// load of its own: the round gathers dist[anc[i]] anyway. A k-mer is finished when its ancestor is a head.
__global__ __launch_bounds__(256) void k_unitig_rank_init(const u32* __restrict__ prev, u64 n, u32* __restrict__ anc, u32* __restrict__ dist) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 p = prev[i];
    anc[i] = p == UNITIG_NONE ? (u32)i : p;
    dist[i] = p == UNITIG_NONE ? 0u : 1u;
}
// One round, from (anc, dist) into (anc2, dist2), never in place: a k-mer whose ancestor a is no head moves to a's ancestor and adds a's
// distance (saturating: on a pure cycle the distance only doubles, and is thrown away). unfinished[0] += the k-mers that were not finished
// when the round began: one LDS reduction and one atomic per workgroup.
__global__ __launch_bounds__(256) void k_unitig_jump(const u32* __restrict__ anc, const u32* __restrict__ dist, u64 n, u32* __restrict__ anc2, u32* __restrict__ dist2,
                                                      u64* __restrict__ unfinished) {
    __shared__ u32 s_cnt[4];
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 open = 0;
    if (i < n) {
        const u32 a = anc[i], d = dist[i];
        const u32 da = dist[a];
        if (da != 0) {
            const u64 s = (u64)d + da;
            anc2[i] = anc[a];
            dist2[i] = s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (u32)s;
            open = 1;
        } else {
            anc2[i] = a;
            dist2[i] = d;
        }
    }
    const u32 w = (u32)__builtin_popcountll(__ballot(open));
    if ((threadIdx.x & 63u) == 0) s_cnt[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) {
        const u32 t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (t) atomicAdd((unsigned long long*)unfinished, (unsigned long long)t);
    }
}

// ---- pure cycles. When the count of unfinished k-mers repeats, every path is finished and the unfinished k-mers are exactly the members of
// the cycles made of simple edges only. Min-doubling over next: lo[i] = the smallest ordinal among i and its 2^r - 1 successors.
__global__ __launch_bounds__(256) void k_cycle_init(const u32* __restrict__ anc, const u32* __restrict__ dist, const u32* __restrict__ next, u64 n, u32* __restrict__ lo,
                                                     u32* __restrict__ ptr) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool member = dist[anc[i]] != 0;
    lo[i] = member ? (u32)i : UNITIG_NONE;
    ptr[i] = member ? next[i] : UNITIG_NONE;  // a member's simple out-edge stays inside its cycle
}
__global__ __launch_bounds__(256) void k_cycle_min(const u32* __restrict__ lo, const u32* __restrict__ ptr, u64 n, u32* __restrict__ lo2, u32* __restrict__ ptr2) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 p = ptr[i];
    if (p == UNITIG_NONE) { lo2[i] = lo[i]; ptr2[i] = p; return; }
    const u32 a = lo[i], b = lo[p];
    lo2[i] = a < b ? a : b;
    ptr2[i] = ptr[p];
}
// lo[i] = the smallest ordinal of i's cycle (UNITIG_NONE for the k-mers of paths). That member becomes the head: the simple edge into it is
// cut (prev[i], and next of its predecessor: one writer each) and circular[i] is set; then the members start the ranking again.
__global__ __launch_bounds__(256) void k_cycle_cut(const u32* __restrict__ lo, u64 n, u32* __restrict__ next, u32* __restrict__ prev, u8* __restrict__ circular,
                                                    u32* __restrict__ anc, u32* __restrict__ dist, u64* __restrict__ n_circular) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 m = lo[i];
    if (m == UNITIG_NONE) return;
    if (m == (u32)i) {
        next[prev[i]] = UNITIG_NONE;
        prev[i] = UNITIG_NONE;
        circular[i] = 1;
        anc[i] = (u32)i;
        dist[i] = 0;
        atomicAdd((unsigned long long*)n_circular, 1ull);
    } else {
        anc[i] = prev[i];  // (no other lane writes the prev of a k-mer that is not the smallest)
        dist[i] = 1;
    }
}

// ---- numbering: is_head -> exclusive scan -> uid (the unitigs in ascending ordinal of their heads)
__global__ __launch_bounds__(256) void k_unitig_heads(const u32* __restrict__ prev, u64 n, u32* __restrict__ is_head) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) is_head[i] = prev[i] == UNITIG_NONE ? 1u : 0u;
}
// Every output may be null. The head writes head[u] and flags[u], the tail (no simple out-edge) writes length[u].
__global__ __launch_bounds__(256) void k_unitig_number(const u32* __restrict__ anc, const u32* __restrict__ dist, const u32* __restrict__ next, const u32* __restrict__ uid,
                                                        const u8* __restrict__ circular, u64 n, u32* __restrict__ unitig, u32* __restrict__ offset, u32* __restrict__ head,
                                                        u32* __restrict__ length, u8* __restrict__ flags) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 h = anc[i], d = dist[i], u = uid[h];
    if (unitig) unitig[i] = u;
    if (offset) offset[i] = d;
    if (h == (u32)i) {
        if (head) head[u] = (u32)i;
        if (flags) flags[u] = circular[i];
    }
    if (length && next[i] == UNITIG_NONE) length[u] = d + 1u;
}

// ---- text: line u = the K letters of its head, the last letter of every following k-mer in offset order, '\n': K + length[u] bytes from
// base[u] (exclusive scan of K + length). One lane per k-mer of an export pass.
__global__ __launch_bounds__(256) void k_unitig_line_bytes(const u32* __restrict__ length, u64 nu, u32 K, u32* __restrict__ bytes) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u < nu) bytes[u] = K + length[u];
}
__global__ __launch_bounds__(256) void k_unitig_text(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u32* __restrict__ unitig,
                                                      const u32* __restrict__ offset, const u32* __restrict__ length, const u64* __restrict__ base, u32 K,
                                                      u8* __restrict__ text) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const u32 u = unitig[e0 + i], off = offset[e0 + i];
    u8* const line = text + base[u];
    u128 x = (u128)k_lo[i];
    if (k_hi) x |= (u128)k_hi[i] << 64;
    if (off == 0) {
        for (u32 j = 0; j < K; ++j) line[j] = (u8)((0x47544341u >> (8u * ((u32)(x >> (2u * (K - 1u - j))) & 3u))) & 0xFFu);  // b"ACTG"[code], first base first
    } else {
        line[K - 1u + off] = (u8)((0x47544341u >> (8u * ((u32)x & 3u))) & 0xFFu);
    }
    if (off + 1u == length[u]) line[K + off] = '\n';
}

}  // namespace cblx
