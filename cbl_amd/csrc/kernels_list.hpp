// kernels_list.hpp — reading the index out: a RANGE of the iteration order as packed k-mers or as text lines
// (CBL::iter /root/reference/src/cbl.rs:358-361 and the `list` loop examples/cbl.rs:190-199), and the node count of every
// bucket (CBL::buckets_nodes src/cbl.rs:386-390 -> src/wordset/mod.rs:282-295 -> TrieVec::count_nodes src/trievec/mod.rs:37-42
// -> TrieNode::count_nodes src/trie.rs:90-102).
#pragma once
#include "kernels_serde.hpp"

namespace cblx {

static const u32 LIST_THREADS = 256;   // elements per workgroup of k_export_range
static const u32 LIST_MAX_LINE = 60;   // K <= 59: K bases + '\n'

// Four 2-bit nucleotide codes, the first in bits 7:6 of b, as four ASCII bytes, the first in byte 0: b"ACTG"[code]
// (src/kmer.rs:26-27). The codes are spread to one per byte, reversed, and mapped without a table:
// 'A' + 2 * bit0 + 0x13 * bit1 - 0xF * (bit0 & bit1) = 'A', 'C', 'T', 'G'; no byte carries into its neighbour.
__device__ __forceinline__ u32 nuc4(u32 b) {
    u32 x = (b | (b << 12)) & 0x000F000Fu;
    x = (x | (x << 6)) & 0x03030303u;
    x = __builtin_bswap32(x);
    const u32 b0 = x & 0x01010101u, b1 = (x >> 1) & 0x01010101u;
    return 0x41414141u + 2u * b0 + 0x13u * b1 - 0xFu * (b0 & b1);
}

// Elements [e0, e0 + n) of the iteration order (prefixes ascending, a Vec bucket in stored order, a Trie bucket ascending:
// kernels_kmer.hpp k_export_kmers) -> word -> k-mer (revert_necklace_pos, src/necklace/mod.rs:29-31), written from index 0 of
// the outputs: packed (out_lo / out_hi, out_hi may be null) or, TEXT, as lines of K bytes of IntKmer::to_nucs + '\n'.
// res_off[nb + 1] = exclusive scan of the bucket lengths (+ the total).
//
// One workgroup takes LIST_THREADS consecutive elements. It searches the bucket b0 of the first one; then thread t looks
// at bucket b0 + t and, when it begins inside the workgroup's elements, marks the element where it begins (buckets are not
// empty, so at most LIST_THREADS of them meet the workgroup); a running maximum over the marks gives every element its
// bucket. No per-element search.
// TEXT: the lines are staged in LDS at their place in the workgroup's byte range and leave in 16-byte stores. The range
// begins at blockIdx.x * LIST_THREADS * LINE bytes, a multiple of 16 whatever LINE is, so with a 16-byte aligned out_text no
// workgroup has an unaligned head; only the last workgroup of a range can end off a 16-byte boundary, and those (< 16) bytes
// are stored one by one. LINE = K + 1 is even: an odd line starts on a 2-byte boundary when LINE % 4 == 2.
template <bool TEXT, bool WS>
__global__ __launch_bounds__(LIST_THREADS) void k_export_range(u64 e0, u64 n, u64 nb, const u64* __restrict__ res_off, const u32* __restrict__ bucket_prefix,
                                                               const u64* __restrict__ start, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, Consts P,
                                                               u64* __restrict__ out_lo, u64* __restrict__ out_hi, u8* __restrict__ out_text) {
    constexpr u32 NW = LIST_THREADS / 64;
    __shared__ u32 s_head[LIST_THREADS];
    __shared__ u32 s_wmax[NW];
    __shared__ __attribute__((aligned(16))) u8 s_stage[TEXT ? LIST_THREADS * LIST_MAX_LINE : 16];
    const u32 tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const u64 rel0 = (u64)blockIdx.x * LIST_THREADS;  // first element of the workgroup, relative to e0
    if (rel0 >= n) return;
    const u32 cnt = (u32)(n - rel0 < LIST_THREADS ? n - rel0 : LIST_THREADS);
    const u64 eb = e0 + rel0;
    s_head[tid] = 0;
    // the bucket of the first element, by a LIST_THREADS-ary search of the whole workgroup: three rounds of one load each for 2^24 buckets, where a
    // binary search by one thread is 24 dependent loads with the other lanes waiting
    u64 b0 = 0, h = nb;  // res_off[b0] <= eb < res_off[h]
    while (h - b0 > 1) {
        const u64 step = (h - b0 + LIST_THREADS - 1) / LIST_THREADS;
        const u64 at = b0 + (u64)tid * step;
        const u32 c = (u32)__syncthreads_count(at < h && res_off[at] <= eb);  // the probes are ascending: true ... true false ... false, thread 0 is true
        b0 += (u64)(c - 1u) * step;
        h = b0 + step < h ? b0 + step : h;
    }
    __syncthreads();  // s_head is clear (an index of one bucket skips the search and its barriers)
    if (b0 + tid < nb) {
        const u64 ro = res_off[b0 + tid];
        if (ro < eb + cnt) atomicMax(&s_head[ro > eb ? (u32)(ro - eb) : 0u], tid);
    }
    __syncthreads();
    // inclusive running maximum over s_head
    u32 m = s_head[tid];
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u32 t = __shfl_up(m, o, 64);
        if (lane >= (u32)o) m = m > t ? m : t;
    }
    if (lane == 63) s_wmax[w] = m;
    __syncthreads();
    for (u32 i = 0; i < w; ++i) m = m > s_wmax[i] ? m : s_wmax[i];

    if (tid < cnt) {
        const u64 b = b0 + m;
        const u64 slot = start[b] + (eb + tid - res_off[b]);
        const Sfx<WS> s = arena_sfx<WS>(a_lo, a_hi, slot, P.SB);
        u128 sfx = (u128)s.lo;
        if constexpr (WS) sfx |= (u128)s.hi << 64;
        const u128 word = ((u128)bucket_prefix[b] << P.SB) | sfx;
        const u128 necklace = word >> P.POS;
        const u32 pos = (u32)word & ((1u << P.POS) - 1u);
        const u128 MASK = (((u128)1) << P.KB) - 1;  // KB <= 118
        const u128 kmer = ((necklace << (P.KB - pos)) & MASK) | (necklace >> pos);
        if constexpr (!TEXT) {
            out_lo[rel0 + tid] = (u64)kmer;
            if (out_hi) out_hi[rel0 + tid] = (u64)(kmer >> 64);
        } else {
            const u32 LINE = P.K + 1, nd = LINE >> 2;
            u128 y = kmer << (128u - P.KB);  // the first base in the top two bits; what follows the last base is zero
            u8* const sl = s_stage + tid * LINE;
            if (!(LINE & 2u)) {  // K % 4 == 3: whole dwords, the last one ends with '\n'
                u32* const p = reinterpret_cast<u32*>(sl);
                for (u32 i = 0; i < nd; ++i) {
                    u32 d = nuc4((u32)(y >> 120));
                    y <<= 8;
                    if (i == nd - 1) d = (d & 0x00FFFFFFu) | 0x0A000000u;
                    p[i] = d;
                }
            } else {  // K % 4 == 1: lines start on 2-byte boundaries; the last half holds one base and '\n'
                u16* const p = reinterpret_cast<u16*>(sl);
                for (u32 i = 0; i < nd; ++i) {
                    const u32 d = nuc4((u32)(y >> 120));
                    y <<= 8;
                    p[2 * i] = (u16)d;
                    p[2 * i + 1] = (u16)(d >> 16);
                }
                p[2 * nd] = (u16)((nuc4((u32)(y >> 120)) & 0xFFu) | 0x0A00u);
            }
        }
    }
    if constexpr (TEXT) {
        __syncthreads();
        const u32 nbytes = cnt * (P.K + 1), n16 = nbytes >> 4;
        u8* const dst = out_text + rel0 * (P.K + 1);
        for (u32 i = tid; i < n16; i += LIST_THREADS) reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(s_stage)[i];
        const u32 t = (n16 << 4) + tid;
        if (tid < 16 && t < nbytes) dst[t] = s_stage[t];
    }
}

// ---- node statistics: nodes[r] = TrieVec::count_nodes of bucket r. A Vec gives its length. A Trie of byte strings of BYTES
// bytes has its root plus one node per distinct proper byte prefix of length 1 .. BYTES - 1 (TrieNode::count_nodes counts the
// nodes that hold a bitvector: the last byte lives in the bitvector of its parent). Over the ascending suffixes x[0 .. n) the
// first one brings the root and BYTES - 1 nodes, x[j] the nodes below what it shares with x[j - 1]: BYTES - 1 - lcp[j], which is
// the little-endian index of the most significant byte where the two differ (kernels_serde.hpp top_diff_byte):
//   nodes = BYTES + sum over j >= 1 of top_diff_byte(x[j], x[j - 1]).
// One wave per bucket; a Trie of more than NODES_WAVE_MAX words is left to a workgroup (k_bucket_nodes_long) through a list.
static const u32 NODES_WAVE_MAX = 8192, NODES_LONG_THREADS = 1024;

template <bool WS>
__global__ __launch_bounds__(256) void k_bucket_nodes(u64 r0, u64 nb, const u64* __restrict__ start, const u32* __restrict__ count, const u8* __restrict__ kind,
                                                      const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, u32 SB, u32 BYTES, u64* __restrict__ nodes,
                                                      u32* __restrict__ long_list, u32* __restrict__ long_n, u32 long_cap) {
    const u64 r = r0 + (((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const u32 lane = threadIdx.x & 63;
    if (r >= nb) return;
    const u32 c = count[r];
    if (kind[r] != KIND_TRIE) {
        if (lane == 0) nodes[r] = c;
        return;
    }
    if (c > NODES_WAVE_MAX) {
        if (lane == 0) {
            const u32 at = atomicAdd(long_n, 1u);  // one per long bucket
            if (at < long_cap) long_list[at] = (u32)r;
        }
        return;
    }
    const u64 s0 = start[r];
    u32 sum = 0;
    for (u32 j = lane + 1; j < c; j += 64) sum += top_diff_byte<WS>(arena_sfx<WS>(a_lo, a_hi, s0 + j, SB), arena_sfx<WS>(a_lo, a_hi, s0 + j - 1, SB));
    sum = wave_reduce_sum(sum);
    if (lane == 0) nodes[r] = (u64)BYTES + sum;
}

template <bool WS>
__global__ __launch_bounds__(NODES_LONG_THREADS) void k_bucket_nodes_long(const u32* __restrict__ long_list, const u32* __restrict__ long_n, const u64* __restrict__ start,
                                                                          const u32* __restrict__ count, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, u32 SB,
                                                                          u32 BYTES, u64* __restrict__ nodes) {
    constexpr u32 NW = NODES_LONG_THREADS / 64;
    __shared__ u64 s_sum[NW];
    if (blockIdx.x >= *long_n) return;
    const u32 r = long_list[blockIdx.x];
    const u64 s0 = start[r];
    const u32 c = count[r], tid = threadIdx.x;
    u64 sum = 0;
    for (u64 j = (u64)tid + 1; j < c; j += NODES_LONG_THREADS)
        sum += top_diff_byte<WS>(arena_sfx<WS>(a_lo, a_hi, s0 + j, SB), arena_sfx<WS>(a_lo, a_hi, s0 + j - 1, SB));
    sum = wave_reduce_sum(sum);
    if ((tid & 63u) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        u64 t = BYTES;
        for (u32 i = 0; i < NW; ++i) t += s_sum[i];
        nodes[r] = t;
    }
}

}  // namespace cblx
