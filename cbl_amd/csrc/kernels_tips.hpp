// kernels_tips.hpp — tip clipping on the compacted de Bruijn graph: the degrees at the two ends of every unitig, the mark of the
// short dead ends, and the selection of their k-mers for one WordSet::remove_batch. Both forms, as in kernels_gfa.hpp: the plain unitigs of a
// non-canonical index (section 6k; `reversed` is null) and the bidirected ones of a canonical index (section 6l).
//   right(u)      the out-degree of the tail of the kept image: the links that leave slot 2 u (section 6m)
//   left(u)       the in-degree of the head of the kept image: in the bidirected form the links that leave slot 2 u + 1
//   kind[u]       0; TIP_TIP when length[u] <= max_kmers and exactly one of left, right is 0; TIP_ISOLATED when both are. Self-edges and hairpins count in
//                 the degrees, so a circular unitig has left, right >= 1 and is never marked.
// Plain C++ HIP. Every output element has one writer: plain vector stores only; the atomics are the four counters that are read back.
#pragma once
#include "kernels_gfa.hpp"

namespace cblx {

static const u32 TIP_NONE = 0, TIP_TIP = 1, TIP_ISOLATED = 2;

// One lane per stored k-mer: the head of the kept image writes left[u], its tail writes right[u] (a unitig of length 1: both from one lane). The in-nibble of
// oriented k-mer (i, 1) is a permutation of the out-nibble of (i, 0) and the other way round, so a reversed end only swaps the nibbles that are counted.
// left / right may be null.
__global__ __launch_bounds__(256) void k_tip_ends(const u32* __restrict__ unitig, const u32* __restrict__ offset, const u8* __restrict__ reversed,
                                                   const u32* __restrict__ length, const u8* __restrict__ masks, u64 n, u8* __restrict__ left, u8* __restrict__ right) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 u = unitig[i], off = offset[i], mk = masks[i];
    const bool rev = reversed && reversed[i] != 0;
    const u32 out = mk & 15u, in = mk >> 4;
    if (left && off == 0) left[u] = (u8)__builtin_popcount(rev ? out : in);
    if (right && off + 1u == length[u]) right[u] = (u8)__builtin_popcount(rev ? in : out);
}

// One lane per unitig: kind[u] (may be null), and counts[0 .. 3] += the tips, their k-mers, the isolated unitigs, their k-mers: a reduction per wave, one
// LDS sum and one atomic per workgroup and counter. counts is zeroed by the caller.
__global__ __launch_bounds__(256) void k_tip_mark(const u32* __restrict__ length, const u8* __restrict__ left, const u8* __restrict__ right, u64 nu, u64 max_kmers,
                                                   u8* __restrict__ kind, u64* __restrict__ counts) {
    __shared__ u64 s_sum[4][4];
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 kd = TIP_NONE, len = 0;
    if (u < nu) {
        len = length[u];
        const bool l0 = left[u] == 0, r0 = right[u] == 0;
        if ((u64)len <= max_kmers) kd = (l0 && r0) ? TIP_ISOLATED : (l0 != r0) ? TIP_TIP : TIP_NONE;
        if (kind) kind[u] = (u8)kd;
    }
    const u64 tips = (u64)__builtin_popcountll(__ballot(kd == TIP_TIP)), lone = (u64)__builtin_popcountll(__ballot(kd == TIP_ISOLATED));
    const u64 tip_kmers = wave_reduce_sum<u64>(kd == TIP_TIP ? len : 0u), lone_kmers = wave_reduce_sum<u64>(kd == TIP_ISOLATED ? len : 0u);
    if ((threadIdx.x & 63u) == 0) {
        u64* s = s_sum[threadIdx.x >> 6];
        s[0] = tips; s[1] = tip_kmers; s[2] = lone; s[3] = lone_kmers;
    }
    __syncthreads();
    if (threadIdx.x < 4) {
        const u64 t = s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x] + s_sum[2][threadIdx.x] + s_sum[3][threadIdx.x];
        if (t) atomicAdd((unsigned long long*)(counts + threadIdx.x), (unsigned long long)t);
    }
}

// One lane per stored k-mer: sel[i] = 1 when the kind of its unitig is wanted (bit kind of `want`), the input of the scan that gives the output positions
__global__ __launch_bounds__(256) void k_tip_select(const u32* __restrict__ unitig, const u8* __restrict__ kind, u64 n, u32 want, u32* __restrict__ sel) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sel[i] = (want >> kind[unitig[i]]) & 1u;
}

// One export pass: k-mer i of the pass has ordinal e0 + i; a selected one stores its packed k-mer at pos[e0 + i], the exclusive scan of sel, so the output
// is in iteration order. out_hi is null for K <= 31 (and k_hi with it).
__global__ __launch_bounds__(256) void k_tip_gather(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u32* __restrict__ sel,
                                                     const u32* __restrict__ pos, u64* __restrict__ out_lo, u64* __restrict__ out_hi) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || sel[e0 + i] == 0) return;
    const u32 p = pos[e0 + i];
    out_lo[p] = k_lo[i];
    if (out_hi) out_hi[p] = k_hi ? k_hi[i] : 0ull;
}

}  // namespace cblx
