// kernels_abundance.hpp — k-mer abundances from reads: the tally of a batch of query words into a caller's array of counts, the
// spectrum of such an array, the coverage of the unitigs, the LN / KC tags of the GFA S lines, and the selection of the weakly supported k-mers for one
// WordSet::remove_batch. The index stays a set: the counts belong to the caller.
//   ordinal        of a stored k-mer: its index in the iteration order of the moment (section 6k); n = count()
//   occurrence     one k-mer of a batch of reads as the query path enumerates it: sequence after sequence, get_seq_words order; bytes that are not ACGT
//                  are skipped as contains_seqs skips them, a sequence shorter than K gives none, a canonical index counts both strands for the one stored k-mer
//   tally          counts[i] = min(2^32 - 1, counts[i] + occ_i), occ_i = the occurrences of the batch whose word has ordinal i; the call accumulates
//   spectrum       hist[j] = the ordinals with counts[i] == j for j < 255; hist[255] = those with counts[i] >= 255
//   coverage       kc[u] = the sum of counts[i] over the k-mers of unitig u (64-bit: at most length[u] (2^32 - 1))
//   tagged S line  "S\t<u>\t<letters>\tLN:i:<length[u] + K - 1>\tKC:i:<kc[u]>\n", decimal without padding; without counts the KC tag and its tab are absent
//   filter         k-mer rule: counts[i] < min_count; unitig rule: every k-mer of a unitig with kc[u] < min_count length[u] (mean coverage below min_count)
// Plain C++ HIP. The atomics: the compare-and-swap loop of the saturating add and the 64-bit sums of kc and of the spectrum (integer adds: the results do
// not depend on the order), and the two counters that are read back.
#pragma once
#include "kernels_gfa.hpp"

namespace cblx {

static const u32 ABUNDANCE_MAX = 0xFFFFFFFFu;

// *p = min(2^32 - 1, *p + a): a plain atomicAdd would wrap, so a compare-and-swap loop that stops at the ceiling. A saturated count is final (the array
// only grows during a tally), so such an add ends without a swap.
__device__ __forceinline__ void abundance_add_sat(u32* p, u32 a) {
    u32 old = __atomic_load_n(p, __ATOMIC_RELAXED);
    while (old != ABUNDANCE_MAX) {
        const u32 nw = old > ABUNDANCE_MAX - a ? ABUNDANCE_MAX : old + a;
        const u32 seen = atomicCAS(p, old, nw);
        if (seen == old) return;
        old = seen;
    }
}

// The tally of n query words: k_rank's shape — QL lanes per word, rank_of_word — but instead of storing the ordinal r, the group's first lane adds to
// counts[r]: 8 bytes per occurrence are neither written nor read back. The leaders whose ordinal is that of the wave's first leader with a hit are summed in
// the wave (a ballot and a popcount) and that leader adds the sum; the others issue their own. A wave has 64 / QL = 8 leaders, so this merges at most 8 adds
// into one: a poly-A read still sends one compare-and-swap per wave to one address. An ordinal at or above n_counts is never written (the host refuses n_counts != n before the launch). totals[0] += the words,
// totals[1] += those the index holds: ballots, one LDS sum and one atomic per workgroup and counter. totals is zeroed by the caller.
template <typename HiT>
__global__ __launch_bounds__(256) void k_rank_tally(const u64* __restrict__ w_lo, const HiT* __restrict__ w_hi, u64 n, u32 SB, u32 PB, DirView dir,
                                                     const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, const u64* __restrict__ res_off, u32* counts,
                                                     u64 n_counts, u64* __restrict__ totals) {
    __shared__ u32 s_cnt[4][2];
    const u64 i = ((u64)blockIdx.x * blockDim.x + threadIdx.x) / QL;
    const bool live = i < n;  // whole groups are live or not (QL divides the workgroup size)
    u64 r = ~0ull;
    if (live) r = rank_of_word(w_lo[i], ld_hi<HiT>(w_hi, i), SB, PB, dir, a_lo, a_hi, res_off);
    const bool leader = live && (threadIdx.x & (QL - 1u)) == 0;
    const bool hit = leader && r < n_counts;  // (~0: absent)
    const u64 hits = __ballot(hit);
    if (hits) {  // wave-uniform
        const u32 lead = (u32)__builtin_ctzll(hits);
        const u64 r0 = __shfl(r, (int)lead, 64);
        const bool same = hit && r == r0;
        const u32 cnt = (u32)__builtin_popcountll(__ballot(same));
        if (same) {
            if (lane_id() == lead) abundance_add_sat(counts + r0, cnt);
        } else if (hit) {
            abundance_add_sat(counts + r, 1u);
        }
    }
    const u32 w_all = (u32)__builtin_popcountll(__ballot(leader)), w_hit = (u32)__builtin_popcountll(hits);
    if ((threadIdx.x & 63u) == 0) { s_cnt[threadIdx.x >> 6][0] = w_all; s_cnt[threadIdx.x >> 6][1] = w_hit; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const u32 t = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (t) atomicAdd((unsigned long long*)(totals + threadIdx.x), (unsigned long long)t);
    }
}

// The bases of the sequences a tally keeps (those of at least K bases), side by side: one lane per byte i of [first, first + m) of the compacted batch. Kept
// sequence s (the last one with dst_off[s] <= i, by bisection over the nk + 1 ascending entries; dst_off[nk] = all bytes) has its bases at src + src_off[s].
__global__ __launch_bounds__(256) void k_abundance_compact(const u8* __restrict__ src, const u64* __restrict__ src_off, const u64* __restrict__ dst_off, u64 nk, u64 first, u64 m,
                                                            u8* __restrict__ dst) {
    const u64 j = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m) return;
    const u64 i = first + j;
    u64 lo = 0, hi = nk;  // invariant: dst_off[lo] <= i < dst_off[hi]
    while (hi - lo > 1) {
        const u64 mid = (lo + hi) >> 1;
        if (dst_off[mid] <= i) lo = mid; else hi = mid;
    }
    dst[i] = src[src_off[lo] + (i - dst_off[lo])];
}

// One lane per ordinal: a 256-bin histogram of the workgroup in LDS (a bin holds at most the 256 lanes), flushed with one 64-bit atomic per non-empty
// bin. hist (256 words) is zeroed by the caller.
__global__ __launch_bounds__(256) void k_abundance_hist(const u32* __restrict__ counts, u64 n, u64* __restrict__ hist) {
    __shared__ u32 s_bin[256];
    s_bin[threadIdx.x] = 0;
    __syncthreads();
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const u32 v = counts[i];
        atomicAdd(s_bin + (v < 255u ? v : 255u), 1u);
    }
    __syncthreads();
    const u32 t = s_bin[threadIdx.x];
    if (t) atomicAdd((unsigned long long*)(hist + threadIdx.x), (unsigned long long)t);
}

// One lane per ordinal: kc[unitig[i]] += counts[i] (kc: nu words zeroed by the caller). Consecutive ordinals often share a unitig, and one giant unitig
// would put every lane on one address: k_cc_sizes' combination — the lanes whose unitig is that of the wave's first active lane are summed in the wave and
// that lane issues one atomic; the others issue their own. A unitig at or above nu is never written.
__global__ __launch_bounds__(256) void k_unitig_kc(const u32* __restrict__ unitig, const u32* __restrict__ counts, u64 n, u64 nu, u64* __restrict__ kc) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u32 u = i < n ? unitig[i] : 0u;
    const bool active = i < n && (u64)u < nu;
    const u32 v = active ? counts[i] : 0u;
    const u64 live = __ballot(active);
    if (live == 0) return;  // wave-uniform
    const u32 lead = (u32)__builtin_ctzll(live);
    const u32 u0 = (u32)__shfl((int)u, (int)lead, 64);
    const bool same = active && u == u0;
    const u64 sum = wave_reduce_sum<u64>(same ? (u64)v : 0ull);
    if (!active) return;
    if (same) {
        if (lane_id() == lead && sum) atomicAdd((unsigned long long*)(kc + u0), (unsigned long long)sum);
    } else if (v) {
        atomicAdd((unsigned long long*)(kc + u), (unsigned long long)v);
    }
}

// One lane per ordinal: sel[i] = 1 when the k-mer goes, the input of the scan that gives the output positions. unitig == null: the k-mer rule,
// counts[i] < min_count. Otherwise the unitig rule on the table's unitig / length and kc: kc[u] < min_count length[u] (below 2^64: length < 2^32).
__global__ __launch_bounds__(256) void k_abundance_select(const u32* __restrict__ counts, u64 n, u32 min_count, const u32* __restrict__ unitig,
                                                           const u64* __restrict__ kc, const u32* __restrict__ length, u32* __restrict__ sel) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (!unitig) { sel[i] = counts[i] < min_count ? 1u : 0u; return; }
    const u32 u = unitig[i];
    sel[i] = kc[u] < (u64)min_count * (u64)length[u] ? 1u : 0u;
}

// One lane per unitig, the unitig rule's stats: gone[0] += the unitigs with kc[u] < min_count length[u], gone[1] += their k-mers — what the scan of sel must
// add up to. k_tip_mark's reduction: per wave, one LDS sum and one atomic per workgroup and counter. gone is zeroed by the caller.
__global__ __launch_bounds__(256) void k_abundance_unitig_stats(const u64* __restrict__ kc, const u32* __restrict__ length, u64 nu, u32 min_count, u64* __restrict__ gone) {
    __shared__ u64 s_sum[4][2];
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u32 len = 0;
    bool goes = false;
    if (u < nu) {
        len = length[u];
        goes = kc[u] < (u64)min_count * (u64)len;
    }
    const u64 cnt = (u64)__builtin_popcountll(__ballot(goes)), kmers = wave_reduce_sum<u64>(goes ? (u64)len : 0ull);
    if ((threadIdx.x & 63u) == 0) { s_sum[threadIdx.x >> 6][0] = cnt; s_sum[threadIdx.x >> 6][1] = kmers; }
    __syncthreads();
    if (threadIdx.x < 2) {
        const u64 t = s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x] + s_sum[2][threadIdx.x] + s_sum[3][threadIdx.x];
        if (t) atomicAdd((unsigned long long*)(gone + threadIdx.x), (unsigned long long)t);
    }
}

// One export pass: k-mer i of the pass has ordinal e0 + i; a selected one stores its packed k-mer at pos[e0 + i], the exclusive scan of sel, so the output
// is in iteration order. out_hi is null for K <= 31 (and k_hi with it). k_tip_gather's body, as a kernel of this file.
__global__ __launch_bounds__(256) void k_abundance_gather(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u32* __restrict__ sel,
                                                           const u32* __restrict__ pos, u64* __restrict__ out_lo, u64* __restrict__ out_hi) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m || sel[e0 + i] == 0) return;
    const u32 p = pos[e0 + i];
    out_lo[p] = k_lo[i];
    if (out_hi) out_hi[p] = k_hi ? k_hi[i] : 0ull;
}

// ---- the tags of the S lines. decimal digits of a 64-bit v (up to 20), by comparison with the powers of ten
__device__ __forceinline__ u32 abundance_digits(u64 v) {
    u32 d = 1;
    for (u64 p = 10ull; d < 20u && v >= p; p *= 10ull) ++d;  // (p = 10^19 is the last one compared; its product is not)
    return d;
}
// v in d = abundance_digits(v) decimal digits at p; returns p + d
__device__ __forceinline__ u8* abundance_put_dec(u8* p, u64 v, u32 d) {
    for (u32 j = d; j-- > 0;) { p[j] = (u8)('0' + (u32)(v % 10ull)); v /= 10ull; }
    return p + d;
}
// bytes[u] of a tagged S line: k_gfa_s_bytes' prefix, letters and '\n', then "\tLN:i:" and its number, and with kc "\tKC:i:" and its number
__global__ __launch_bounds__(256) void k_gfa_s_bytes_tagged(const u32* __restrict__ length, const u64* __restrict__ kc, u64 nu, u32 K, u32* __restrict__ bytes) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nu) return;
    const u32 len = length[u];
    u32 b = 3u + gfa_digits((u32)u) + K + len + 6u + abundance_digits((u64)len + K - 1u);
    if (kc) b += 6u + abundance_digits(kc[u]);
    bytes[u] = b;
}
// One lane per unitig, behind the text kernels on the stream: base[u] is the offset in `text` of the line's letters (k_gfa_s_prefix), whose K + length[u] - 1
// bytes and a '\n' behind them the text kernels wrote. That '\n' becomes the '\t' of the first tag — the one byte with two writers, ordered by the stream —
// and the tags and the line's own '\n' follow.
__global__ __launch_bounds__(256) void k_gfa_s_tags(const u32* __restrict__ length, const u64* __restrict__ kc, const u64* __restrict__ base, u64 nu, u32 K,
                                                     u8* __restrict__ text) {
    const u64 u = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= nu) return;
    const u64 ln = (u64)length[u] + K - 1u;
    u8* p = text + base[u] + ln;
    p[0] = '\t'; p[1] = 'L'; p[2] = 'N'; p[3] = ':'; p[4] = 'i'; p[5] = ':';
    p = abundance_put_dec(p + 6, ln, abundance_digits(ln));
    if (kc) {
        const u64 v = kc[u];
        p[0] = '\t'; p[1] = 'K'; p[2] = 'C'; p[3] = ':'; p[4] = 'i'; p[5] = ':';
        p = abundance_put_dec(p + 6, v, abundance_digits(v));
    }
    p[0] = '\n';
}

}  // namespace cblx
