// kernels_graph.hpp — the index as the node set of a de Bruijn graph: which of a k-mer's eight neighbours the set holds
// (Kmer::successors / Kmer::predecessors, src/kmer.rs:82-90 of the reference, each looked up with CBL::contains src/cbl.rs:219-221),
// and the table of (out-degree, in-degree) pairs over the whole index. DESIGN.md section 6j.
//   append(x, c)  = ((x << 2) | c) & MASK          successor by base c   -> bit c of the mask
//   prepend(x, c) = (x >> 2) | (c << 2 (K - 1))    predecessor by base c -> bit 4 + c
#pragma once
#include "kernels_kmer.hpp"

namespace cblx {

// x = packed k-mer i of a caller's arrays, read with the layout rules of k_kmers_to_words (k_hi may be null for K <= 31); false when it has bits above 2K
template <bool WIDE>
__device__ __forceinline__ bool load_kmer(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 i, const Consts& P, typename KmerT<WIDE>::type& x) {
    if constexpr (WIDE) {
        x = ((u128)(k_hi ? k_hi[i] : 0ull) << 64) | (u128)k_lo[i];  // K = 31 with a > 64-bit suffix runs this layout too
        return (x >> P.KB) == 0;
    } else {
        x = k_lo[i];
        return (x >> P.KB) == 0 && !(k_hi && k_hi[i] != 0);
    }
}
// bad[0] += the k-mers of a caller's batch that are no IntKmer<K>. A batch of several passes is checked as a whole before the first pass writes
// a mask: a refusal writes nothing.
template <bool WIDE>
__global__ __launch_bounds__(256) void k_kmers_check(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 n, Consts P, u32* __restrict__ bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typename KmerT<WIDE>::type x;
    if (!load_kmer<WIDE>(k_lo, k_hi, i, P, x)) atomicAdd(bad, 1u);
}

// Word of neighbour j (0 .. 7) of k-mer i, work item 8 i + j: the eight lanes of a k-mer sit side by side, so the loads of x are
// broadcasts inside a lane group and the stores are coalesced. x is read with the layout rules of k_kmers_to_words (k_hi may be null
// for K <= 31; bits above 2K bump bad[0] once per k-mer). The neighbour is canonicalised where the index is canonical, x itself is
// taken as given. TAGGED: the 16-byte query record of k_query_tag is written directly — w_hi[8 i + j] = hi bits | (8 i + j) << 32 —
// for words of at most 96 bits.
template <bool WIDE, typename HiT, bool TAGGED>
__global__ __launch_bounds__(256) void k_neighbor_words(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 n, Consts P, u64* __restrict__ w_lo,
                                                        typename std::conditional<TAGGED, u64, HiT>::type* __restrict__ w_hi, u32* __restrict__ bad) {
    const u64 t = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 i = t >> 3;
    const u32 j = (u32)t & 7u;
    if (i >= n) return;
    typedef typename KmerT<WIDE>::type T;
    T x;
    if (!load_kmer<WIDE>(k_lo, k_hi, i, P, x)) { if (j == 0) atomicAdd(bad, 1u); x = 0; }
    const T MASK = (((T)1) << P.KB) - 1;  // KB <= 62 in 64 bits, <= 118 in 128
    const T code = (T)(j & 3u);
    const T y = j < 4 ? (((x << 2) | code) & MASK) : ((x >> 2) | (code << (P.KB - 2)));  // K = 33: a shift by exactly 64, in the 128-bit type
    u64 lo, hi;
    kmer_word<WIDE>(y, P, P.canonical && !kmer_is_fwd<WIDE>(y), lo, hi);
    w_lo[t] = lo;
    if constexpr (TAGGED) w_hi[t] = hi | (t << 32);
    else st_hi<HiT>(w_hi, t, hi);
}

// mask[i] = bit j set where flag[8 i + j] != 0: one aligned 8-byte load and one byte stored per k-mer
__global__ __launch_bounds__(256) void k_fold_neighbor_flags(const u64* __restrict__ flags8 /* 8 flag bytes per k-mer */, u64 n, u8* __restrict__ mask) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    u64 v = flags8[i];
    v |= v >> 4; v |= v >> 2; v |= v >> 1;  // bit 0 of every byte = OR of its eight bits (what the shifts bring in from the byte above stops at bit 2)
    v &= 0x0101010101010101ull;
    mask[i] = (u8)((v * 0x0102040810204080ull) >> 56);  // byte j's bit 0 -> bit j of the top byte; the partial products do not overlap
}

// table[5 * out + in] += the k-mers of masks[0 .. n) with out = popcount(mask & 15), in = popcount(mask >> 4): per wave one LDS add per
// bin that occurs in it (ballot), per workgroup one 64-bit global add per non-zero bin. Integer sums: the table does not depend on the
// schedule.
static const u32 DEGREE_BINS = 25;
__global__ __launch_bounds__(256) void k_degree_tally(const u8* __restrict__ masks, u64 n, u64* __restrict__ table) {
    __shared__ u32 s_bin[DEGREE_BINS];
    const u32 tid = threadIdx.x, lane = tid & 63u;
    if (tid < DEGREE_BINS) s_bin[tid] = 0;
    __syncthreads();
    const u64 stride = (u64)gridDim.x * blockDim.x;
    for (u64 base = (u64)blockIdx.x * blockDim.x; base < n; base += stride) {  // base is uniform over the workgroup: every wave runs the same rounds
        const u64 i = base + tid;
        const bool valid = i < n;
        u32 bin = 0;
        if (valid) {
            const u32 m = masks[i];
            bin = 5u * (u32)__builtin_popcount(m & 15u) + (u32)__builtin_popcount(m >> 4);
        }
        u64 todo = __ballot(valid);
        while (todo) {  // wave-uniform
            const u32 leader = (u32)__builtin_ctzll(todo);
            const u32 b = (u32)__shfl((int)bin, (int)leader, 64);
            const u64 same = __ballot(valid && bin == b);
            if (lane == leader) atomicAdd(&s_bin[b], (u32)__builtin_popcountll(same));
            todo &= ~same;
        }
    }
    __syncthreads();
    if (tid < DEGREE_BINS && s_bin[tid]) atomicAdd((unsigned long long*)&table[tid], (unsigned long long)s_bin[tid]);
}

}  // namespace cblx
