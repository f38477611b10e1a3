// kernels_remove.hpp — WordSet::remove_batch (src/wordset/mod.rs:218-237) over a whole batch of words, per bucket.
//
// Nothing is inserted during a removal, so of all the removal words aimed at a bucket only the FIRST stream occurrence of each suffix the
// bucket holds changes anything (the "effective" removals, at most one per stored word). The kernels below find them without sorting the
// batch: the stored words of the visited buckets go into one hash table, every removal word probes it and leaves its ordinal in its stored
// word's slot by atomicMin. The group of a removal word (a maximal run of equal prefix inside one remove_batch call = one chunk) is the number
// of group starts at or before it — a scan over the batch — so a bucket learns the group of an effective removal from its ordinal and no mark
// has to travel with the word. k_bucket_remove then replays the effective removals of one bucket in stream order:
//   Vec:  swap_remove (src/trievec/mod.rs:91-108) with position tracking — pos[t] = where stored word t stands now, elem[p] = which stored word
//         stands at p — O(1) per removal;
//   Trie: plain set difference up to the end of the group in which the length reaches 1024 (adapt_container_shrink, src/wordset/mod.rs:232-235,
//         runs after every group that visits the prefix), an ascending Vec from there, swap_remove for the effective removals of later groups.
#pragma once
#include "kernels_kmer.hpp"

namespace cblx {

static const u32 RM_NONE = 0xFFFFFFFFu;
static const u64 RM_EMPTY = ~0ull;
// a bucket's tables (sort keys, pos, elem) live in LDS up to this many slots (the bucket's length rounded up to a power of two), else in global memory
static const u32 RM_SMALL = 64, RM_LDS = 2048;

__host__ __device__ inline u32 rm_pow2(u32 c) {  // c <= 2^31 (k_rm_caps refuses longer buckets)
    u64 p = 1;
    while (p < c) p <<= 1;
    return (u32)p;
}
__device__ __forceinline__ u64 rm_hash(u64 r, u64 s_lo, u64 s_hi) { return mix64(s_lo + 0x9E3779B97F4A7C15ull * (r + 1)) ^ mix64(s_hi ^ 0xD1B54A32D192ED03ull); }

// first word of every chunk starts a group (a chunk is one remove_batch call); gstart was zeroed
__global__ void k_rm_chunk_marks(const u64* __restrict__ kmer_off, u64 nchunks, u64 n, u32* __restrict__ gstart) {
    const u64 ch = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= nchunks) return;
    const u64 k = kmer_off[ch];
    if (k < n) gstart[k] = 1u;
}
// per removal word: its bucket's rank (RM_NONE: the index lacks the prefix), the group-start mark, and the bucket marked as visited
template <typename HiT>
__global__ __launch_bounds__(256) void k_rm_visit(const u64* __restrict__ w_lo, const HiT* __restrict__ w_hi, u64 n, u32 SB, u32 PB, DirView dir, u32 every,
                                                  u32* __restrict__ gstart, u32* __restrict__ wrank, u32* __restrict__ visited) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u32 p = get_bits(w_lo[i], ld_hi<HiT>(w_hi, i), SB, PB);
    if (every || i == 0 || get_bits(w_lo[i - 1], ld_hi<HiT>(w_hi, i - 1), SB, PB) != p) gstart[i] = 1u;
    u64 r;
    if (dir_lookup(dir, p, r)) { wrank[i] = (u32)r; visited[r] = 1u; }
    else wrank[i] = RM_NONE;
}
// table slots of a bucket: its length rounded up to a power of two when the batch visits it (the replay sorts that many keys), else none
__global__ void k_rm_caps(u64 nb, const u32* __restrict__ visited, const u32* __restrict__ cnt, u32* __restrict__ cap, u32* __restrict__ too_long) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nb) return;
    if (visited[r] && cnt[r] > 0x80000000u) { *too_long = 1u; cap[r] = 0u; return; }  // the host refuses the call
    cap[r] = visited[r] ? rm_pow2(cnt[r]) : 0u;
}
// shortest sequence of a batch (the check in front of a batch that goes in as several sub-batches)
__global__ void k_rm_min_len(const u64* __restrict__ offsets, u64 nseq, unsigned long long* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nseq) atomicMin(out, (unsigned long long)(offsets[i + 1] - offsets[i]));
}
// the new arena: bucket r's new_cnt words from its slots of the replay's output when the replay rewrote it, else from its old run; LPB lanes per bucket
template <bool WS, int LPB>
__global__ __launch_bounds__(256) void k_rm_gather(u64 nb, const u64* __restrict__ new_start, const u32* __restrict__ new_cnt, const u8* __restrict__ moved,
                                                   const u64* __restrict__ voff, const u64* __restrict__ start, const u64* __restrict__ o_lo, const u64* __restrict__ o_hi,
                                                   const u64* __restrict__ x_lo, const u64* __restrict__ x_hi, u64* __restrict__ n_lo, u64* __restrict__ n_hi) {
    const u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x, r = g / LPB;
    if (r >= nb) return;
    const u32 c = new_cnt[r];
    const u64 d0 = new_start[r];
    const bool mv = moved[r] != 0;
    const u64* s_lo = mv ? x_lo + voff[r] : o_lo + start[r];
    for (u32 j = (u32)(g % LPB); j < c; j += LPB) n_lo[d0 + j] = s_lo[j];
    if constexpr (WS) {
        const u64* s_hi = mv ? x_hi + voff[r] : o_hi + start[r];
        for (u32 j = (u32)(g % LPB); j < c; j += LPB) n_hi[d0 + j] = s_hi[j];
    }
}
// visited buckets by table size: list 0 = up to RM_SMALL slots, 1 = up to RM_LDS, 2 = longer
__global__ void k_rm_classify(u64 nb, const u32* __restrict__ cap, u32* __restrict__ lists, u32* __restrict__ list_n) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nb || cap[r] == 0) return;
    const u32 cls = cap[r] <= RM_SMALL ? 0u : (cap[r] <= RM_LDS ? 1u : 2u);
    lists[(u64)cls * nb + atomicAdd(&list_n[cls], 1u)] = (u32)r;
}
// every stored word of the visited buckets into the hash table (slot v of the table space -> bucket by search in voff); the words of an index
// are distinct, so an insert never meets its own key
__global__ __launch_bounds__(256) void k_rm_build(u64 vbase, u64 nslots, u64 nb, const u64* __restrict__ voff, const u32* __restrict__ cnt, const u64* __restrict__ start,
                                                  const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, u32 SB, u64* __restrict__ table, u64 hmask) {
    const u64 v = vbase + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nslots) return;
    u64 l = 0, h = nb;  // last bucket with voff <= v (its slot count is not zero)
    while (h - l > 1) {
        const u64 mid = (l + h) >> 1;
        if (voff[mid] <= v) l = mid; else h = mid;
    }
    const u64 t = v - voff[l];
    if (t >= cnt[l]) return;  // padding
    const u128 M = (((u128)1) << SB) - 1;
    u128 s = a_lo[start[l] + t];
    if (a_hi) s |= (u128)a_hi[start[l] + t] << 64;
    s &= M;
    const u64 e = (l << 32) | t;
    u64 hsh = rm_hash(l, (u64)s, (u64)(s >> 64)) & hmask;
    while (atomicCAS((unsigned long long*)&table[hsh], (unsigned long long)RM_EMPTY, (unsigned long long)e) != (unsigned long long)RM_EMPTY) hsh = (hsh + 1) & hmask;
}
// every removal word looks its stored word up: first[slot] = the smallest ordinal that names it, mingroup[bucket] = the first group that visits it
template <typename HiT>
__global__ __launch_bounds__(256) void k_rm_probe(const u64* __restrict__ w_lo, const HiT* __restrict__ w_hi, u64 n, u32 SB, const u32* __restrict__ wrank,
                                                  const u32* __restrict__ gstart, const u32* __restrict__ gbefore, const u64* __restrict__ voff, const u64* __restrict__ start,
                                                  const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, const u64* __restrict__ table, u64 hmask,
                                                  u32* __restrict__ first, u32* __restrict__ mingroup, u64* __restrict__ wslot) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (wslot) wslot[i] = RM_EMPTY;
    const u32 r = wrank[i];
    if (r == RM_NONE) return;
    atomicMin(&mingroup[r], gbefore[i] + gstart[i]);
    const u128 M = (((u128)1) << SB) - 1;
    const u128 key = ((((u128)ld_hi<HiT>(w_hi, i)) << 64) | w_lo[i]) & M;
    const u64 s0 = start[r];
    u64 hsh = rm_hash(r, (u64)key, (u64)(key >> 64)) & hmask;
    for (;;) {
        const u64 e = table[hsh];
        if (e == RM_EMPTY) return;
        if ((u32)(e >> 32) == r) {
            const u32 t = (u32)e;
            u128 s = a_lo[s0 + t];
            if (a_hi) s |= (u128)a_hi[s0 + t] << 64;
            if ((s & M) == key) {
                atomicMin(&first[voff[r] + t], (u32)i);
                if (wslot) wslot[i] = voff[r] + t;
                return;
            }
        }
        hsh = (hsh + 1) & hmask;
    }
}
// CBL::remove's return value per word: it was present iff it is the effective removal of its stored word
__global__ void k_rm_flags(u64 n, const u64* __restrict__ wslot, const u32* __restrict__ first, u8* __restrict__ out) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (wslot[i] != RM_EMPTY && first[wslot[i]] == (u32)i) ? 1 : 0;
}

// One workgroup of T threads per visited bucket; CAP > 0: tables of CAP slots in LDS, CAP = 0: in global memory at the bucket's slots.
// Reads the bucket from the arena and writes what is left to the bucket's slots of x_lo / x_hi (moved[r] = 1; a bucket no word hit keeps its run), its length and kind.
template <bool WS, int T, int CAP>
__global__ __launch_bounds__(T) void k_bucket_remove(const u32* __restrict__ list, const u32* __restrict__ list_n, const u64* __restrict__ start, const u32* __restrict__ cnt,
                                                     const u8* __restrict__ kind, const u64* __restrict__ voff, const u32* __restrict__ first,
                                                     const u32* __restrict__ gstart, const u32* __restrict__ gbefore, const u32* __restrict__ mingroup,
                                                     const u64* __restrict__ o_lo, const u64* __restrict__ o_hi, u64* __restrict__ x_lo, u64* __restrict__ x_hi,
                                                     u32* __restrict__ new_cnt, u8* __restrict__ new_kind, u8* __restrict__ moved, u64* __restrict__ g_keys, u32* __restrict__ g_pos, u32* __restrict__ g_elem) {
    __shared__ u64 s_keys[CAP ? CAP : 1];
    __shared__ u32 s_pos[CAP ? CAP : 1], s_elem[CAP ? CAP : 1];
    __shared__ u32 s_scan[T / 64 + 1], s_E, s_n1;
    if (blockIdx.x >= *list_n) return;
    const u32 r = list[blockIdx.x], tid = threadIdx.x;
    const u32 L = cnt[r], K = kind[r];
    const u64 v0 = voff[r], s0 = start[r];
    const u32 cp = (u32)(voff[r + 1] - v0);  // power of two, >= L
    u64* keys = CAP ? s_keys : g_keys + v0;
    u32* pos = CAP ? s_pos : g_pos + v0;
    u32* elem = CAP ? s_elem : g_elem + v0;
    if (tid == 0) { s_E = 0; s_n1 = 0; }
    __syncthreads();
    // effective removals of the bucket: (ordinal, stored position), gathered at the front of the table (E <= L <= cp)
    for (u32 t = tid; t < L; t += T) {
        const u32 f = first[v0 + t];
        if (f != RM_NONE) keys[atomicAdd(&s_E, 1u)] = ((u64)f << 32) | t;
    }
    __syncthreads();
    const u32 E = s_E;
    const bool shrinks = K == KIND_TRIE && L <= VEC_THRESHOLD;  // a short Trie (set operations leave them) turns into a Vec at the first group that visits it
    if (E == 0) {  // only absent words came: the stored order is ascending already where the kind changes
        if (tid == 0) { new_cnt[r] = L; new_kind[r] = shrinks ? KIND_VEC : (u8)K; }
        return;
    }
    // stream order: bitonic sort of the E keys, padded with the largest key to a power of two (a long bucket hit by one word sorts nothing)
    const u32 pe = rm_pow2(E);
    for (u32 i = E + tid; i < pe; i += T) keys[i] = RM_EMPTY;
    __syncthreads();
    for (u32 k = 2; k <= pe; k <<= 1)
        for (u32 j = k >> 1; j > 0; j >>= 1) {
            for (u32 i = tid; i < pe; i += T) {
                const u32 x = i ^ j;
                if (x > i) {
                    const u64 a = keys[i], b = keys[x];
                    if ((a > b) == ((i & k) == 0)) { keys[i] = b; keys[x] = a; }
                }
            }
            __syncthreads();
        }
    // n1 = effective removals that are plain deletions (Trie, up to the end of the group that converts it); the others are swap_removed
    bool to_vec = K == KIND_VEC;
    if (K == KIND_TRIE) {
        const u32 j0 = L > VEC_THRESHOLD ? L - VEC_THRESHOLD : 0u;  // the j0-th effective removal brings the length down to 1024
        if (j0 && E < j0) {
            if (tid == 0) s_n1 = E;
        } else {
            to_vec = true;
            u32 gc;
            if (j0) { const u32 o = (u32)(keys[j0 - 1] >> 32); gc = gbefore[o] + gstart[o]; }
            else gc = mingroup[r];
            u32 c1 = 0;
            for (u32 j = tid; j < E; j += T) { const u32 o = (u32)(keys[j] >> 32); c1 += (gbefore[o] + gstart[o]) <= gc; }
            if (c1) atomicAdd(&s_n1, c1);
        }
    }
    for (u32 t = tid; t < L; t += T) pos[t] = 0;
    __syncthreads();
    const u32 n1 = s_n1;
    for (u32 j = tid; j < n1; j += T) pos[(u32)keys[j]] = 1u;  // deleted
    __syncthreads();
    // what stays keeps its order: pos / elem of the compacted list
    u32 base = 0;
    for (u32 t0 = 0; t0 < L; t0 += T) {
        const u32 t = t0 + tid;
        const u32 keep = (t < L && pos[t] == 0) ? 1u : 0u;
        u32 tot;
        const u32 ex = block_exclusive_scan<T, u32>(keep, s_scan, &tot);
        if (t < L) {
            if (keep) { pos[t] = base + ex; elem[base + ex] = t; }
            else pos[t] = RM_NONE;
        }
        base += tot;
    }
    __syncthreads();
    u32 len = L - n1;
    if (tid == 0) {  // swap_remove, in stream order: the last word moves into the hole
        for (u32 j = n1; j < E; ++j) {
            const u32 t = (u32)keys[j], p = pos[t], f = elem[--len];
            elem[p] = f;
            pos[f] = p;
        }
        s_n1 = len;
    }
    __syncthreads();
    len = s_n1;
    for (u32 p = tid; p < len; p += T) {
        const u32 src = elem[p];
        x_lo[v0 + p] = o_lo[s0 + src];
        if constexpr (WS) x_hi[v0 + p] = o_hi[s0 + src];
    }
    if (tid == 0) { moved[r] = 1; new_cnt[r] = len; new_kind[r] = to_vec ? (u8)KIND_VEC : (u8)KIND_TRIE; }
}

}  // namespace cblx
