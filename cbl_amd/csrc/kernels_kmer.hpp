// kernels_kmer.hpp — packed k-mers in and out of the index: CBL::insert / contains on an IntKmer
// (/root/reference/src/cbl.rs:199-228) and CBL::iter (:208-214,358-361). A packed k-mer is IntKmer::to_int(): 2K bits,
// first base most significant (/root/reference/src/kmer.rs:200-202); lo = low 64 bits, hi = the rest (K >= 33).
#pragma once
#include "kernels_bucket.hpp"

namespace cblx {

// get_word (src/cbl.rs:199-206): canonical() when the index is canonical (even popcount keeps the k-mer, src/kmer.rs:94-106),
// then necklace_pos + merge_necklace_pos. bad[0] counts k-mers with bits set above 2K (not an IntKmer<K>).
template <bool WIDE, typename HiT>
__global__ void k_kmers_to_words(const u64* __restrict__ k_lo, const u64* __restrict__ k_hi, u64 n, Consts P, u64* __restrict__ w_lo,
                                 HiT* __restrict__ w_hi, u32* __restrict__ bad) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    typedef typename KmerT<WIDE>::type T;
    T x;
    bool oob;
    if constexpr (WIDE) {
        x = ((u128)(k_hi ? k_hi[i] : 0ull) << 64) | (u128)k_lo[i];  // K = 31 with a > 64-bit suffix runs this layout too
        oob = (x >> P.KB) != 0;
    } else {
        x = k_lo[i];
        oob = (x >> P.KB) != 0 || (k_hi && k_hi[i] != 0);
    }
    if (oob) { atomicAdd(bad, 1u); x = 0; }
    u64 lo, hi;
    kmer_word<WIDE>(x, P, P.canonical && !kmer_is_fwd<WIDE>(x), lo, hi);
    w_lo[i] = lo;
    st_hi<HiT>(w_hi, i, hi);
}

// ---- "was this word absent so far?" for a batch of single inserts (WordSet::insert returns it, src/wordset/mod.rs:97-120):
// absent = not in the resident index AND no equal word earlier in the batch. The second half is a first-occurrence
// test: an open-addressing table of word INDICES (slot = i + 1, 0 = empty). Equal words follow the same probe sequence
// and stop at the first slot that is empty or holds an equal word, so every distinct word owns exactly one slot, which
// atomicMin turns into the smallest index of its class. -----------------------------------------------------------------
__device__ __forceinline__ u32 first_slot(u64 lo, u64 hi, u32 mask) { return (u32)(word_hash(lo, hi) >> 29) & mask; }

template <typename HiT>
__global__ void k_first_claim(const u64* __restrict__ w_lo, const HiT* __restrict__ w_hi, u64 n, u32* __restrict__ table, u32 mask) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 lo = w_lo[i], hi = ld_hi<HiT>(w_hi, i);
    u32 h = first_slot(lo, hi, mask);
    for (;;) {
        const u32 cur = atomicCAS(&table[h], 0u, (u32)i + 1u);
        if (cur == 0) return;  // claimed an empty slot
        const u32 j = cur - 1u;  // any member of the slot's class will do for the comparison
        if (w_lo[j] == lo && ld_hi<HiT>(w_hi, j) == hi) { atomicMin(&table[h], (u32)i + 1u); return; }
        h = (h + 1u) & mask;
    }
}
// flag[i] = (i is the first occurrence of its word) && !flag_in[i]   (flag_in = membership in the resident index)
template <typename HiT>
__global__ void k_first_flag(const u64* __restrict__ w_lo, const HiT* __restrict__ w_hi, u64 n, const u32* __restrict__ table, u32 mask,
                             u8* __restrict__ flag) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 lo = w_lo[i], hi = ld_hi<HiT>(w_hi, i);
    u32 h = first_slot(lo, hi, mask);
    for (;;) {
        const u32 j = table[h] - 1u;  // never empty along the probe sequence of an inserted word
        if (w_lo[j] == lo && ld_hi<HiT>(w_hi, j) == hi) { flag[i] = (j == (u32)i && !flag[i]) ? 1 : 0; return; }
        h = (h + 1u) & mask;
    }
}

// zeros[0] += number of zero bytes (contains_all = no zero among the membership flags)
__global__ void k_count_zero_u8(const u8* __restrict__ v, u64 n, u32* __restrict__ zeros) {
    u32 z = 0;
    for (u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (u64)gridDim.x * blockDim.x) z += v[i] == 0;
    z = wave_reduce_sum(z);
    if ((threadIdx.x & 63) == 0 && z) atomicAdd(zeros, z);
}

// ---- membership tallies by JOIN (the `cbl query` loop at scale, examples/cbl.rs:205-228): the query words go through the
// same stable partition as a batch of new words, so the queries of one prefix sit in one run; one workgroup then joins that
// run with the resident bucket of the prefix — the bucket is read once per workgroup instead of once per query:
//   a resident bucket of <= JOIN_TAB_MAX elements, Vec or Trie: an open-addressing table of (tag, element index) in LDS;
//   a longer Trie (ascending): binary search per query, the probes of the run's queries share the cache;
//   a longer Vec (only `|=` makes them): scanned per query.
// per_run[b] = queries of run b found. No per-query flags: the partition does not keep the queries' positions. -------------------
// hi64[i] = i << 32 | hi[i]: the ordinal of a query word rides through the partition in the unused upper half of a 64-bit
// hi part (words of at most 96 bits), so the join can write per-query flags in query order
template <typename HiT>
__global__ void k_query_tag(u64 n, const HiT* __restrict__ hi, u64* __restrict__ hi64) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) hi64[i] = (i << 32) | ld_hi<HiT>(hi, i);
}

static const u32 JOIN_THREADS = 256, JOIN_FULL_MAX = 2730, JOIN_TAB_MAX = 4095, JOIN_SLOTS = 8192;
// One resident bucket as a join workgroup sees it, and its class (uniform over the workgroup): `full` and `table` build an LDS table
// (join_build), a longer Trie is searched and a longer Vec scanned in place (join_probe). k_query_join and k_panel_join share the two.
template <bool WS> struct JoinBucket {
    const u64 *lo, *hi;  // the bucket's first arena slot
    u32 rc, SB;
    bool trie, full, table;
    __device__ __forceinline__ Sfx<WS> at(u32 j) const { return load_sfx<WS, u64>(lo, hi, j, SB); }
};
template <bool WS>
__device__ __forceinline__ JoinBucket<WS> join_bucket(const DirView& dir, u64 r, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, u32 SB) {
    const u64 rs = dir.start[r];  // the three directory reads first: they are in flight together
    const u32 rc = dir.count[r];
    const bool trie = dir.kind[r] == KIND_TRIE;
    JoinBucket<WS> B;
    B.lo = a_lo + rs;
    B.hi = WS ? a_hi + rs : a_hi;
    B.rc = rc;
    B.SB = SB;
    B.trie = trie;
    // Up to JOIN_TAB_MAX elements (Vec or Trie alike: the elements of a bucket are distinct) go into an open-addressing
    // table in LDS, at most half full; the tag keeps the probes off global memory until a candidate matches.
    B.full = !WS && SB < 64 && B.rc <= JOIN_FULL_MAX;
    B.table = !B.full && B.rc <= JOIN_TAB_MAX;
    return B;
}
// 32 KB of LDS, one of two tables: FULL = 4096 slots holding the suffix itself (narrow suffixes, up to JOIN_FULL_MAX
// elements: a probe never leaves LDS — a verifying read per hit cost 40 ps, 4x the rest of the join), or 8192 slots of
// 20-bit tag << 12 | element index (0xFFFFFFFF = empty; index 4095 is never used), verified in the bucket on a tag match.
// Every thread of the workgroup calls it (barriers inside); nobody may still probe what the table held before.
template <bool WS> __device__ __forceinline__ void join_build(u64* s_full, const JoinBucket<WS>& B, u32 tid) {
    u32* s_tab = reinterpret_cast<u32*>(s_full);
    if (B.full) {
        for (u32 i = tid; i < JOIN_SLOTS / 2; i += JOIN_THREADS) s_full[i] = ~0ull;
        __syncthreads();
        for (u32 j = tid; j < B.rc; j += JOIN_THREADS) {
            const Sfx<WS> e = B.at(j);
            u32 h = sfx_hash_bits<WS>(e, 12);
            while (atomicCAS((unsigned long long*)&s_full[h], ~0ull, (unsigned long long)e.lo) != ~0ull) h = (h + 1u) & (JOIN_SLOTS / 2 - 1u);
        }
        __syncthreads();
    }
    if (B.table) {
        for (u32 i = tid; i < JOIN_SLOTS; i += JOIN_THREADS) s_tab[i] = 0xFFFFFFFFu;
        __syncthreads();
        for (u32 j = tid; j < B.rc; j += JOIN_THREADS) {
            const u32 hv = sfx_hash_bits<WS>(B.at(j), 32);
            u32 h = hv >> 19;
            const u32 e = ((hv & 0xFFFFFu) << 12) | j;
            while (atomicCAS(&s_tab[h], 0xFFFFFFFFu, e) != 0xFFFFFFFFu) h = (h + 1u) & (JOIN_SLOTS - 1u);
        }
        __syncthreads();
    }
}
template <bool WS> __device__ __forceinline__ bool join_probe(const u64* s_full, const JoinBucket<WS>& B, const Sfx<WS>& key) {
    const u32* s_tab = reinterpret_cast<const u32*>(s_full);
    bool hit = false;
    if (B.full) {
        u32 h = sfx_hash_bits<WS>(key, 12);
        for (;;) {
            const u64 e = s_full[h];
            if (e == key.lo) { hit = true; break; }
            if (e == ~0ull) break;
            h = (h + 1u) & (JOIN_SLOTS / 2 - 1u);
        }
    } else if (B.table) {
        const u32 hv = sfx_hash_bits<WS>(key, 32);
        u32 h = hv >> 19;
        const u32 tag = hv & 0xFFFFFu;
        for (;;) {
            const u32 e = s_tab[h];
            if (e == 0xFFFFFFFFu) break;
            if ((e >> 12) == tag && B.at(e & 0xFFFu) == key) { hit = true; break; }
            h = (h + 1u) & (JOIN_SLOTS - 1u);
        }
    } else if (B.trie) {  // ascending: binary search, the probes of the run's queries share the cache
        auto less = [](const Sfx<WS>& x, const Sfx<WS>& y) -> bool {
            if constexpr (WS) { if (x.hi != y.hi) return x.hi < y.hi; }
            return x.lo < y.lo;
        };
        u32 l = 0, h = B.rc;
        while (l < h) {
            const u32 mid = (l + h) >> 1;
            if (less(B.at(mid), key)) l = mid + 1; else h = mid;
        }
        hit = l < B.rc && B.at(l) == key;
    } else {  // a Vec this long only comes out of `|=`
        for (u32 j = 0; j < B.rc && !hit; ++j) hit = B.at(j) == key;
    }
    return hit;
}
template <bool WS, typename HiT>
__global__ __launch_bounds__(JOIN_THREADS) void k_query_join(u64 nbq, u64 b0, const u32* __restrict__ q_prefix, const u64* __restrict__ q_start,
                                                             const u64* __restrict__ q_lo, const HiT* __restrict__ q_hi, u32 SB, DirView dir,
                                                             const u64* __restrict__ a_lo, const u64* __restrict__ a_hi,
                                                             u32* __restrict__ per_run /* zero-filled, one per run */,
                                                             u8* __restrict__ flags = nullptr /* zero-filled; ordinal = q_hi >> 32 */) {
    __shared__ u64 s_full[JOIN_SLOTS / 2];
    u32* s_tab = reinterpret_cast<u32*>(s_full);
    const u64 b = b0 + blockIdx.x;
    if (b >= nbq) return;
    u64 r;
    if (!dir_lookup(dir, q_prefix[b], r)) return;  // no resident bucket: every query of the run misses
    const u64 qs = q_start[b], qe = q_start[b + 1];
    const u32 tid = threadIdx.x;
    const JoinBucket<WS> B = join_bucket<WS>(dir, r, a_lo, a_hi, SB);
    join_build<WS>(s_full, B, tid);
    u32 found = 0;
    for (u64 q = qs + tid; q < qe; q += JOIN_THREADS) {
        const bool hit = join_probe<WS>(s_full, B, load_sfx<WS, HiT>(q_lo, q_hi, q, SB));
        found += hit ? 1u : 0u;
        if constexpr (std::is_same<HiT, u64>::value && !WS) {  // per-query flags: the query's ordinal rides in the upper half of hi
            if (flags && hit) flags[q_hi[q] >> 32] = 1;
        }
    }
    // one result per run (summed afterwards): 19 M wave-level atomics on ONE counter cost 47 ms at cfg 2
    found = wave_reduce_sum(found);
    __syncthreads();  // every probe of the table is done: its first word takes the tally
    if (tid == 0) s_tab[0] = 0;
    __syncthreads();
    if ((tid & 63u) == 0 && found) atomicAdd(&s_tab[0], found);
    __syncthreads();
    if (tid == 0) per_run[b] = s_tab[0];
}

// ---- a PANEL of indexes in one pass (cblx_contains_seqs_counts_many*): the query words are encoded, tagged with
// their ordinals and partitioned ONCE; one workgroup then walks a query run through the bucket its prefix has in each of up to 64
// indexes, and leaves one 64-bit membership mask per k-mer: bit j = index j holds it. The tallies are reduced from the masks. ---------
struct PanelEntry {  // one index of the panel; an empty index stays in its place with dir.bv = null, dir.nb = 0
    DirView dir;
    const u64 *a_lo, *a_hi;
};
// mask[ordinal of query q] |= 1 << j for every entry j whose bucket holds q. Lane `tid` owns the queries qs + tid + 256 i in every
// round: a mask word has one writing lane for the whole kernel, so plain read-modify-writes do (the first query's word stays in a
// register: most runs are shorter than a workgroup). Everything around a barrier is uniform: dir_lookup and the class depend on (run, j).
__global__ __launch_bounds__(JOIN_THREADS) void k_panel_join(u64 nbq, u64 b0, const u32* __restrict__ q_prefix, const u64* __restrict__ q_start,
                                                             const u64* __restrict__ q_lo, const u64* __restrict__ q_hi /* ordinal << 32 | hi bits */,
                                                             u32 SB, const PanelEntry* __restrict__ panel, u32 n,
                                                             u64* __restrict__ mask /* zero-filled, one word per query */) {
    __shared__ u64 s_full[JOIN_SLOTS / 2];
    const u64 b = b0 + blockIdx.x;
    if (b >= nbq) return;
    const u32 p = q_prefix[b], tid = threadIdx.x;
    const u64 qs = q_start[b], qe = q_start[b + 1];
    const bool mine = qs + tid < qe;  // the lane's first query: key, ordinal and mask word in registers
    Sfx<false> key0;
    key0.lo = 0;
    u64 m0 = 0;
    if (mine) key0 = load_sfx<false, u64>(q_lo, q_hi, qs + tid, SB);
    bool built = false;
    for (u32 j = 0; j < n; ++j) {
        const PanelEntry E = panel[j];
        u64 r;
        if (!dir_lookup(E.dir, p, r)) continue;  // entry j holds nothing on this prefix
        const JoinBucket<false> B = join_bucket<false>(E.dir, r, E.a_lo, E.a_hi, SB);
        if (built) __syncthreads();  // every probe of the previous entry's table is done before it is rebuilt
        join_build<false>(s_full, B, tid);
        built = B.full || B.table;
        const u64 bit = 1ull << j;
        if (mine && join_probe<false>(s_full, B, key0)) m0 |= bit;
        for (u64 q = qs + tid + JOIN_THREADS; q < qe; q += JOIN_THREADS)
            if (join_probe<false>(s_full, B, load_sfx<false, u64>(q_lo, q_hi, q, SB))) mask[q_hi[q] >> 32] |= bit;
    }
    if (mine && m0) mask[q_hi[qs + tid] >> 32] = m0;
}
// the fallback's per-index flags into the masks: mask[i] |= flag[i] << j (one lane per k-mer)
__global__ __launch_bounds__(256) void k_mask_or_flags(const u8* __restrict__ flag, u64 nk, u32 j, u64* __restrict__ mask) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nk && flag[i]) mask[i] |= 1ull << j;
}

// ---- per-sequence tallies (cblx_contains_seqs_counts*): k-mers queried and k-mers found of EVERY sequence of a batch, from the
// batch's flag bytes without bringing them to the host. The flags lie sequence after sequence, each in get_seq_words order, and
// kmer_off[c] is the first flag of chunk c, so the flags of sequence s are [kmer_off[seq_chunk[s]], kmer_off[seq_chunk[s + 1]]).
// Two levels: the flag bytes of every chunk are summed once (1 byte read per k-mer, 4 bytes written per chunk), then every
// sequence sums its chunks (4 bytes per chunk, 8 per sequence written). No tally goes through an atomic: every output has one
// writer and the sums are integers, so the result does not depend on the schedule. -------------------------------------------
// chunk_pos[c] = sum of the flag bytes of chunk c; one wave per chunk (at most CHUNK_KMERS = 2048 flags = two 16-byte loads per
// lane). kmer_off[c] is not aligned in general: the at most 15 bytes in front of and behind the 16-byte aligned run are read
// bytewise by the upper lanes, which a read's chunk (120 flags: eight aligned runs at most) leaves idle anyway.
__global__ __launch_bounds__(256) void k_chunk_tally(const u8* __restrict__ flags, const u64* __restrict__ kmer_off /* nchunks + 1 */, u64 c0, u64 nchunks,
                                                     u32* __restrict__ chunk_pos) {
    const u64 c = c0 + (((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const u32 lane = threadIdx.x & 63;
    if (c >= nchunks) return;
    const u64 a = kmer_off[c];
    const u32 n = (u32)(kmer_off[c + 1] - a);
    const u8* p = flags + a;
    const u32 mis = (16u - (u32)((uintptr_t)p & 15u)) & 15u;
    const u32 head = mis < n ? mis : n;
    const u32 nvec = (n - head) >> 4, tail0 = head + (nvec << 4);
    const uint4* v = reinterpret_cast<const uint4*>(p + head);
    u32 s = 0;
    for (u32 i = lane; i < nvec; i += 64) {
        const uint4 w = v[i];
        s = __builtin_amdgcn_sad_u8(w.x, 0u, s);  // s += the four bytes of the word
        s = __builtin_amdgcn_sad_u8(w.y, 0u, s);
        s = __builtin_amdgcn_sad_u8(w.z, 0u, s);
        s = __builtin_amdgcn_sad_u8(w.w, 0u, s);
    }
    if (lane >= 32 && lane - 32 < head) s += p[lane - 32];
    if (lane >= 48 && tail0 + (lane - 48) < n) s += p[tail0 + (lane - 48)];
    s = wave_reduce_sum(s);
    if (lane == 0) chunk_pos[c] = s;
}
// seq_total[s] = k-mers of sequence s, seq_pos[s] = the sum of chunk_pos over its chunks (either may be null). A read has one
// chunk, a chromosome tens of thousands: a sequence of up to SEQ_TALLY_LANE_MAX chunks takes one lane (reads: a coalesced
// gather), a longer one is left to a workgroup (k_seq_tally_long) through a list, as k_bucket_nodes leaves its long Tries.
// The list's counter is the only atomic: it decides where a long sequence waits, never what is written for it.
static const u32 SEQ_TALLY_LANE_MAX = 8, SEQ_TALLY_LONG_THREADS = 256;
__global__ __launch_bounds__(256) void k_seq_tally(const u64* __restrict__ seq_chunk /* nseq + 1 */, const u64* __restrict__ kmer_off, const u32* __restrict__ chunk_pos,
                                                   u64 nseq, u32* __restrict__ seq_total, u32* __restrict__ seq_pos, u32* __restrict__ long_list,
                                                   u32* __restrict__ long_n, u32 long_cap) {
    const u64 s = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseq) return;
    const u64 a = seq_chunk[s], b = seq_chunk[s + 1];
    if (seq_total) seq_total[s] = (u32)(kmer_off[b] - kmer_off[a]);
    if (!seq_pos) return;
    if (b - a > SEQ_TALLY_LANE_MAX) {
        const u32 at = atomicAdd(long_n, 1u);  // one per long sequence
        if (at < long_cap) long_list[at] = (u32)s;
        return;
    }
    u32 p = 0;
    for (u64 j = a; j < b; ++j) p += chunk_pos[j];
    seq_pos[s] = p;
}
__global__ __launch_bounds__(SEQ_TALLY_LONG_THREADS) void k_seq_tally_long(const u32* __restrict__ long_list, const u32* __restrict__ long_n,
                                                                           const u64* __restrict__ seq_chunk, const u32* __restrict__ chunk_pos,
                                                                           u32* __restrict__ seq_pos) {
    constexpr u32 NW = SEQ_TALLY_LONG_THREADS / 64;
    __shared__ u32 s_sum[NW];
    if (blockIdx.x >= *long_n) return;
    const u32 s = long_list[blockIdx.x], tid = threadIdx.x;
    const u64 a = seq_chunk[s], b = seq_chunk[s + 1];
    u32 p = 0;
    for (u64 j = a + tid; j < b; j += SEQ_TALLY_LONG_THREADS) p += chunk_pos[j];
    p = wave_reduce_sum(p);
    if ((tid & 63u) == 0) s_sum[tid >> 6] = p;
    __syncthreads();
    if (tid == 0) {
        u32 t = 0;
        for (u32 i = 0; i < NW; ++i) t += s_sum[i];
        seq_pos[s] = t;
    }
}

// ---- the same two levels from membership MASKS (k_panel_join): n tallies per chunk and per sequence, one per index of the panel.
// chunk_pos[c * n + j] = k-mers of chunk c that index j holds. One wave per chunk, 64 mask words per round (8-byte loads, coalesced); for
// j < n the ballot of bit j over the round's words is a row of the transposed 64 x 64 bit matrix, and lane j adds its popcount. The
// accumulator is one register per lane, selected by lane == j: no per-lane array, no scratch.
__global__ __launch_bounds__(256) void k_chunk_tally_mask(const u64* __restrict__ mask, const u64* __restrict__ kmer_off /* nchunks + 1 */, u64 c0, u64 nchunks, u32 n,
                                                          u32* __restrict__ chunk_pos /* nchunks * n */) {
    const u64 c = c0 + (((u64)blockIdx.x * blockDim.x + threadIdx.x) >> 6);
    const u32 lane = threadIdx.x & 63;
    if (c >= nchunks) return;  // whole waves leave together
    const u64 a = kmer_off[c];
    const u32 cnt = (u32)(kmer_off[c + 1] - a);
    u32 acc = 0;
    for (u32 i0 = 0; i0 < cnt; i0 += 64) {
        const u64 m = i0 + lane < cnt ? mask[a + i0 + lane] : 0ull;  // a short last round: the lanes past the end hold no bit
        if (!__any(m != 0)) continue;
        for (u32 j = 0; j < n; ++j) {
            const u64 row = __ballot((int)((m >> j) & 1ull));
            if (lane == j) acc += (u32)__popcll(row);
        }
    }
    if (lane < n) chunk_pos[c * n + lane] = acc;
}
// seq_pos[j * nseq + s] = the sum of chunk_pos[. * n + j] over the chunks of sequence s: one lane per (sequence, index), the n lanes of a
// sequence side by side (their reads of a chunk's n tallies coalesce). Sequences of more than SEQ_TALLY_LANE_MAX chunks go through the long
// list (entered once per sequence, by its lane of index 0) to k_seq_tally_long_mask: one workgroup per (long sequence, index).
__global__ __launch_bounds__(256) void k_seq_tally_mask(const u64* __restrict__ seq_chunk /* nseq + 1 */, const u32* __restrict__ chunk_pos, u64 s0, u64 s1 /* this launch's sequences */,
                                                        u64 nseq, u32 n, u32* __restrict__ seq_pos /* n * nseq */, u32* __restrict__ long_list, u32* __restrict__ long_n,
                                                        u32 long_cap) {
    const u64 i = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    const u64 s = s0 + i / n;
    const u32 j = (u32)(i % n);
    if (s >= s1) return;
    const u64 a = seq_chunk[s], b = seq_chunk[s + 1];
    if (b - a > SEQ_TALLY_LANE_MAX) {
        if (j == 0) {
            const u32 at = atomicAdd(long_n, 1u);  // one per long sequence
            if (at < long_cap) long_list[at] = (u32)s;
        }
        return;
    }
    u32 p = 0;
    for (u64 ch = a; ch < b; ++ch) p += chunk_pos[ch * n + j];
    seq_pos[(u64)j * nseq + s] = p;
}
__global__ __launch_bounds__(SEQ_TALLY_LONG_THREADS) void k_seq_tally_long_mask(const u32* __restrict__ long_list, const u32* __restrict__ long_n,
                                                                                const u64* __restrict__ seq_chunk, const u32* __restrict__ chunk_pos, u64 nseq, u32 n,
                                                                                u32* __restrict__ seq_pos) {
    constexpr u32 NW = SEQ_TALLY_LONG_THREADS / 64;
    __shared__ u32 s_sum[NW];
    if (blockIdx.x >= *long_n) return;
    const u32 s = long_list[blockIdx.x], j = blockIdx.y, tid = threadIdx.x;
    const u64 a = seq_chunk[s], b = seq_chunk[s + 1];
    u32 p = 0;
    for (u64 ch = a + tid; ch < b; ch += SEQ_TALLY_LONG_THREADS) p += chunk_pos[ch * n + j];
    p = wave_reduce_sum(p);
    if ((tid & 63u) == 0) s_sum[tid >> 6] = p;
    __syncthreads();
    if (tid == 0) {
        u32 t = 0;
        for (u32 w = 0; w < NW; ++w) t += s_sum[w];
        seq_pos[(u64)j * nseq + s] = t;
    }
}

// CBL::iter: element e of the index in iteration order (prefixes ascending, bucket order as stored: a Vec in
// first-occurrence order, a Trie ascending — src/wordset/mod.rs:298-309, src/trievec/mod.rs:198-206) -> word ->
// recover_kmer (src/cbl.rs:208-214, revert_necklace_pos src/necklace/mod.rs:29-31).
__global__ void k_export_kmers(u64 e0, u64 nelem, u64 nb, const u64* __restrict__ res_off, const u32* __restrict__ bucket_prefix,
                               const u64* __restrict__ start, const u64* __restrict__ a_lo, const u64* __restrict__ a_hi, Consts P,
                               u64* __restrict__ out_lo, u64* __restrict__ out_hi) {
    const u64 e = e0 + (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nelem) return;
    u64 l = 0, h = nb;
    while (h - l > 1) {
        const u64 mid = (l + h) >> 1;
        if (res_off[mid] <= e) l = mid; else h = mid;
    }
    const u64 j = e - res_off[l];
    u128 sfx = (u128)a_lo[start[l] + j];
    if (a_hi) sfx |= (u128)a_hi[start[l] + j] << 64;
    sfx &= (((u128)1) << P.SB) - 1;
    const u128 word = ((u128)bucket_prefix[l] << P.SB) | sfx;
    const u128 necklace = word >> P.POS;
    const u32 pos = (u32)word & ((1u << P.POS) - 1u);
    const u128 MASK = (((u128)1) << P.KB) - 1;  // KB <= 118
    const u128 kmer = ((necklace << (P.KB - pos)) & MASK) | (necklace >> pos);
    out_lo[e] = (u64)kmer;
    if (out_hi) out_hi[e] = (u64)(kmer >> 64);
}

}  // namespace cblx
