// kernels_bubbles.hpp — bubble popping on the compacted de Bruijn graph: the marks of the simple bubbles on the link table of
// section 6m, the selection of the popped arms' k-mers for one WordSet::remove_batch, and the carry of a caller's counts (section 6p) through that
// removal. Both forms, as in kernels_gfa.hpp: the plain unitigs of a non-canonical index and the bidirected ones of a canonical index.
//   out(x), in(x)   of image slot x = 2 p + s: the links of slot x, and the in-degree of that image's head — out(x ^ 1) in the bidirected form (mirror
//                   closure), left(p) of section 6n in the plain form, where only s = 0 exists
//   qualified arm   image x of unitig p from source slot a to target slot T: a -> x is a link, in(x) == out(x) == 1, the one link of x enters T,
//                   length[p] <= max_kmers, and p is neither the unitig of a nor that of T
//   group           the qualified arms that share (a, T), as distinct unitigs: at most 4. Bidirected: (a, T) and (T ^ 1, a ^ 1) are one group
//   order           u above v: kc[u] length[v] > kc[v] length[u] (exact, 128-bit products); then the longer; then the lower number. Without counts
//                   the first clause is absent
//   kind[u]         BUBBLE_KEPT: u is in a group of >= 2 unitigs and above all others; BUBBLE_POPPED: another member is above it; else 0
// Plain C++ HIP. Every output element has one writer: plain vector stores only; the atomics are the three counters that are read back.
#pragma once
#include "kernels_abundance.hpp"

namespace cblx {

static const u32 BUBBLE_NONE = 0, BUBBLE_POPPED = 1, BUBBLE_KEPT = 2;

// One lane per stored k-mer of the plain form: the head of a unitig writes left[u], the in-degree of its head — the head half of k_tip_ends
__global__ __launch_bounds__(256) void k_bubble_left(const u32* __restrict__ unitig, const u32* __restrict__ offset, const u8* __restrict__ masks, u64 n,
                                                      u8* __restrict__ left) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (offset[i] == 0) left[unitig[i]] = (u8)__builtin_popcount((u32)masks[i] >> 4);
}

// u above v in the order; `counted` is false without counts: the coverage clause is skipped
__device__ __forceinline__ bool bubble_above(u64 kc_u, u32 len_u, u32 u, u64 kc_v, u32 len_v, u32 v, bool counted) {
    if (counted) {
        const u64 a_lo = kc_u * (u64)len_v, a_hi = __umul64hi(kc_u, (u64)len_v);  // kc < 2^64, length < 2^32: the products reach 2^96
        const u64 b_lo = kc_v * (u64)len_u, b_hi = __umul64hi(kc_v, (u64)len_u);
        if (a_hi != b_hi) return a_hi > b_hi;
        if (a_lo != b_lo) return a_lo > b_lo;
    }
    if (len_u != len_v) return len_u > len_v;
    return u < v;
}

// One lane per source slot a: every slot in the bidirected form (`bi`), the even slots in the plain one (lane l is slot 2 l; left != null). The lane
// reads its <= 4 links, qualifies each arm, and compares the qualified arms of equal target pairwise. kind (nu bytes, or null: counts only) is zeroed by
// the caller. One writer per kind[u]: an arm has in(x) == 1, so one source sees image x; in the bidirected form the group (a, T) is also seen from T ^ 1
// as (T ^ 1, a ^ 1), and the view with the smaller source slot writes; when a == T ^ 1 the two views are one lane, which holds both images of every arm
// and writes from the even image (link_rev == 0). A member is never compared with its own other image. counts[0 .. 2] += the kept arms, the popped arms,
// the k-mers of the popped arms: k_tip_mark's reduction — ballots and wave sums, one LDS sum and one atomic per workgroup and counter. counts is zeroed by
// the caller. A target unitig at or above nu (never written by the fill) disqualifies the arm: nothing is read or written out of bounds.
__global__ __launch_bounds__(256) void k_bubble_mark(const u64* __restrict__ link_start, const u32* __restrict__ link_to, const u8* __restrict__ link_rev,
                                                      const u32* __restrict__ length, const u8* __restrict__ left, const u64* __restrict__ kc, u64 nu, bool bi,
                                                      u64 max_kmers, u8* __restrict__ kind, u64* __restrict__ counts) {
    __shared__ u64 s_sum[4][3];
    const u64 lane = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 a = bi ? lane : 2ull * lane;
    u32 kept = 0, popped = 0;
    u64 popped_kmers = 0;
    if (a < 2ull * nu) {
        const u64 ls = link_start[a];
        const u32 d = (u32)min((u64)4, link_start[a + 1] - ls);
        u32 arm[4], len[4];
        u64 tgt[4], cov[4];
        bool q[4], even[4];
        if (d >= 2) {  // a group of two unitigs needs two links
#pragma unroll
            for (u32 j = 0; j < 4; ++j) {
                q[j] = false; arm[j] = 0; len[j] = 0; tgt[j] = 0; cov[j] = 0; even[j] = true;
                if (j >= d) continue;
                const u32 p = link_to[ls + j], r = link_rev[ls + j];
                if ((u64)p >= nu || r > 1u) continue;
                const u64 x = 2ull * p + r;
                const u64 xs = link_start[x];
                if (link_start[x + 1] - xs != 1) continue;  // out(x) == 1
                const u64 in = bi ? link_start[(x ^ 1ull) + 1] - link_start[x ^ 1ull] : (u64)left[p];
                if (in != 1) continue;
                const u32 tp = link_to[xs], tr = link_rev[xs];
                const u32 ln = length[p];
                if ((u64)tp >= nu || tr > 1u || (u64)ln > max_kmers || p == (u32)(a >> 1) || p == tp) continue;
                q[j] = true; arm[j] = p; len[j] = ln; tgt[j] = 2ull * tp + tr; even[j] = r == 0;
                cov[j] = kc ? kc[p] : 0ull;
            }
#pragma unroll
            for (u32 j = 0; j < 4; ++j) {
                if (!q[j]) continue;
                const u64 view = tgt[j] ^ 1ull;  // the source slot of the mirror view
                if (bi && (a > view || (a == view && !even[j]))) continue;  // the other view, or the other image, writes
                bool others = false, beaten = false;
#pragma unroll
                for (u32 k = 0; k < 4; ++k) {
                    if (k == j || !q[k] || tgt[k] != tgt[j] || arm[k] == arm[j]) continue;
                    others = true;
                    beaten = beaten || bubble_above(cov[k], len[k], arm[k], cov[j], len[j], arm[j], kc != nullptr);
                }
                if (!others) continue;
                if (kind) kind[arm[j]] = (u8)(beaten ? BUBBLE_POPPED : BUBBLE_KEPT);
                if (beaten) { ++popped; popped_kmers += len[j]; } else ++kept;
            }
        }
    }
    const u64 w_kept = wave_reduce_sum<u64>((u64)kept), w_popped = wave_reduce_sum<u64>((u64)popped), w_kmers = wave_reduce_sum<u64>(popped_kmers);
    if ((threadIdx.x & 63u) == 0) {
        u64* s = s_sum[threadIdx.x >> 6];
        s[0] = w_kept; s[1] = w_popped; s[2] = w_kmers;
    }
    __syncthreads();
    if (threadIdx.x < 3) {
        const u64 t = s_sum[0][threadIdx.x] + s_sum[1][threadIdx.x] + s_sum[2][threadIdx.x] + s_sum[3][threadIdx.x];
        if (t) atomicAdd((unsigned long long*)(counts + threadIdx.x), (unsigned long long)t);
    }
}

// One lane per stored k-mer: sel[i] = 1 when its unitig is popped, the input of the scan that gives the output positions. k_tip_select's body, as a
// kernel of this file.
__global__ __launch_bounds__(256) void k_bubble_select(const u32* __restrict__ unitig, const u8* __restrict__ kind, u64 n, u32* __restrict__ sel) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sel[i] = kind[unitig[i]] == BUBBLE_POPPED ? 1u : 0u;
}

// One export pass: k-mer i of the pass has ordinal e = e0 + i; a selected one stores its packed k-mer at pos[e], the exclusive scan of sel, so the output
// is in iteration order (k_tip_gather's body). With counts (keep_lo != null) the others go to the complement position e - pos[e] of keep_lo / keep_hi,
// their count with them: the survivors in iteration order. out_hi / keep_hi are null for K <= 31 (and k_hi with them).
__global__ __launch_bounds__(256) void k_bubble_gather(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 e0, u64 m, const u32* __restrict__ sel,
                                                        const u32* __restrict__ pos, u64* __restrict__ out_lo, u64* __restrict__ out_hi,
                                                        const u32* __restrict__ counts, u64* __restrict__ keep_lo, u64* __restrict__ keep_hi,
                                                        u32* __restrict__ keep_counts) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const u64 e = e0 + i;
    const u32 p = pos[e];
    if (sel[e]) {
        out_lo[p] = k_lo[i];
        if (out_hi) out_hi[p] = k_hi ? k_hi[i] : 0ull;
    } else if (keep_lo) {
        const u64 kp = e - p;
        keep_lo[kp] = k_lo[i];
        if (keep_hi) keep_hi[kp] = k_hi ? k_hi[i] : 0ull;
        keep_counts[kp] = counts[e];
    }
}

// The carry: survivor i, of count keep_counts[i], has the new ordinal rank[i]: out[rank[i]] = keep_counts[i]. The ranks of the m survivors are a
// permutation of [0, m), so every element has one writer; a rank at or above m (~0: absent) is not written and raises *bad.
__global__ __launch_bounds__(256) void k_counts_scatter(const u64* __restrict__ rank, const u32* __restrict__ keep_counts, u64 m, u32* __restrict__ out,
                                                         u32* __restrict__ bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m) return;
    const u64 r = rank[i];
    if (r >= m) { *bad = 1u; return; }
    out[r] = keep_counts[i];
}

}  // namespace cblx
