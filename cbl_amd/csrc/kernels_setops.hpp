// kernels_setops.hpp — set algebra between resident indexes, bucket by bucket: `self |= other` of two Tries (k_bucket_union), `a OP b` into a new index
// (k_setop_plan, k_setop_gather, k_bucket_setop), CBL::merge / CBL::intersect of n operands (k_many_*, k_bucket_setop_many) and the assigning forms
// `a &= b`, `a -= b`, `a ^= b` (k_bucket_setop_assign). The directory kernels they share with the build (k_setop_bv, k_merge_table, k_merge_gather,
// k_classify_merge) are in kernels_bucket.hpp; the host side is setops.hpp. At the end: |a AND b| without a result index (k_common_*).
#pragma once
#include "common_route.hpp"
#include "kernels_bucket.hpp"

namespace cblx {

// ---- Trie |= Trie: the union of two ASCENDING lists is a merge, not a sort (/root/reference/src/trievec/set_ops.rs:43-71 merges two
// sorted iterators with two pointers; src/trievec/mod.rs:118-136 inserts what self lacks) ------------------------------------------------
// One workgroup per bucket, any length. Rounds of UNI_TILE outputs: the next <= UNI_TILE words of either list are staged in LDS
// (coalesced loads from the two indexes' own arenas — the merged run is written, never read), every thread finds the co-rank of the
// END of its UNI_ITEMS consecutive outputs by a binary search on the round's diagonal (merge path; ties take self's copy first) and gets
// its start from its neighbour, loads n + n candidates into registers and merges them with a fixed network — min(a[k], b[n-1-k]) leaves
// the n smallest as a bitonic sequence, log2 n compare-exchange stages sort it — so no lane follows data-dependent control flow. The
// outputs go back to LDS (one padding word per 8: a lane's 64-byte row would otherwise hit the banks of its neighbours'), are
// compared with their predecessor there (equal = other's copy of a word self holds: dropped) and leave compacted in order. The
// co-rank of the round's last output says how far either list was consumed. HBM traffic: every word read once (the staging areas are
// rings since round 5: a round refills only the slots it consumed — see UniRounds), the union written once.
// Workgroup shape, measured on cfg 5's share (`bench.py --config merge`, stage bucket_big) / at the 8-GPU depth of cfg 5 (`tools/emulate_rank.py --merge`:
// 752 M + 752 M words in buckets of 10 635 each): 256 threads x 8 outputs 3.18 / 9.4 ms, 128 x 8 3.09, 256 x 4 2.14 / 6.3, **128 x 4 2.07 / 6.2**, 256 x 2 2.53 — half the registers
// (a[], b[], o[]), half the merge network and a shorter search per round buy more than the extra rounds cost; padding one word per 4 instead of 8: 2.33 / 6.7.
static const int UNI_THREADS = 128, UNI_ITEMS = 4, UNI_TILE = UNI_THREADS * UNI_ITEMS;
__device__ __forceinline__ u32 uni_pad(u32 i) { return i + (i >> 3); }
// An element of a union: the suffix alone — one u64, or (hi, lo) for suffixes wider than 64 bits (round 5: those took the sorting
// classes whatever their kinds; the rings hold their two halves in two arrays of the same shape).
template <bool WS> struct UniE;
template <> struct UniE<false> { u64 lo; };
template <> struct UniE<true> { u64 lo, hi; };
template <bool WS> __device__ __forceinline__ bool uni_lt(const UniE<WS>& a, const UniE<WS>& b) {
    if constexpr (WS) return a.hi < b.hi || (a.hi == b.hi && a.lo < b.lo);
    else return a.lo < b.lo;
}
template <bool WS> __device__ __forceinline__ bool uni_eq(const UniE<WS>& a, const UniE<WS>& b) {
    if constexpr (WS) return a.lo == b.lo && a.hi == b.hi;
    else return a.lo == b.lo;
}
template <bool WS> __device__ __forceinline__ UniE<WS> uni_inf() {
    UniE<WS> e;
    e.lo = ~0ull;
    if constexpr (WS) e.hi = ~0ull;
    return e;
}
// (selects word by word: a select between two structs sends the arrays they sit in to scratch memory — 224 bytes per lane and 1.4 TB/s
//  as first written)
template <bool WS> __device__ __forceinline__ UniE<WS> uni_sel(bool take_a, const UniE<WS>& a, const UniE<WS>& b) {
    UniE<WS> e;
    e.lo = take_a ? a.lo : b.lo;
    if constexpr (WS) e.hi = take_a ? a.hi : b.hi;
    return e;
}
template <bool WS> __device__ __forceinline__ void uni_cmpx(UniE<WS>& a, UniE<WS>& b) {
    const bool sw = uni_lt<WS>(b, a);
    const UniE<WS> lo = uni_sel<WS>(sw, b, a), hi = uni_sel<WS>(sw, a, b);
    a = lo;
    b = hi;
}
// narrow: suffix = lo & mask; wide: (hi & mask(SB - 64), lo)
template <bool WS> __device__ __forceinline__ u64 suffix_mask(u32 SB) {
    return WS ? ((1ull << (SB - 64)) - 1ull) : (SB >= 64 ? ~0ull : ((1ull << SB) - 1ull));
}
// Ordered compaction over the NW waves of a workgroup. Thread t = (wave w, lane) holds ITEMS flags, flag j standing at position
// w * 64 * ITEMS + j * 64 + lane (wave-contiguous slices keep the order): before[j] = the flags set in front of it, returns how many are set
// in all. `s_wtot`: NW words of LDS from the caller, who synchronises before they are used again.
template <int NW, int ITEMS> __device__ __forceinline__ u32 count_before(const bool (&f)[ITEMS], u32* s_wtot, u32 (&before)[ITEMS]) {
    const u32 w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    u64 bal[ITEMS];
    u32 wh = 0;
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) { bal[j] = __ballot(f[j]); wh += (u32)__builtin_popcountll(bal[j]); }
    if (lane == 0) s_wtot[w] = wh;
    __syncthreads();
    u32 run = 0, tot = 0;
#pragma unroll
    for (int ww = 0; ww < NW; ++ww) { const u32 t = s_wtot[ww]; if ((u32)ww < w) run += t; tot += t; }
#pragma unroll
    for (int j = 0; j < ITEMS; ++j) { before[j] = run + mbcnt(bal[j]); run += (u32)__builtin_popcountll(bal[j]); }
    return tot;
}
template <int NW> __device__ __forceinline__ u32 count_before(bool f, u32* s_wtot, u32& before) {
    const bool fs[1] = {f};
    u32 bs[1];
    const u32 tot = count_before<NW, 1>(fs, s_wtot, bs);
    before = bs[0];
    return tot;
}
// The rounds of a merge path over two ascending lists A (cs words) and B (co words), shared by k_bucket_union and k_bucket_setop. The LDS arrays
// belong to the kernel: s_in / s_inh hold A's ring at logical [0, T) and B's at [T, 2T) and, after write_back, the round's outputs in the slots it
// consumed; s_split the co-ranks at the wave edges.
// The two staging areas are RINGS of T slots (round 5): word g of a list lives in slot g mod T of its ring, a round consumes nout
// words — iend from A, the rest from B — and only those nout slots are refilled in front of the next round; the round's outputs pass
// through exactly the slots it freed. As first written every round staged the next T words of BOTH lists again and consumed T in
// all: every word crossed the L2 twice, and with 16 workgroups per CU holding 8 KB each the second read missed — 6.3 GB fetched for
// 4.0 GB of lists by the TCC counters (profiles/r05_merge_hbm_traffic.md).
template <bool WS> struct UniRounds {
    typedef UniE<WS> E;
    static constexpr int NW = UNI_THREADS / 64;
    static constexpr u32 T = UNI_TILE;
    static_assert((T & (T - 1)) == 0, "the staging rings index by g mod T");
    static constexpr u32 SLOTS = T * 2 + (T * 2) / 8 + 8;
    u64 *s_in, *s_inh;
    u32* s_split;
    const u64 *A, *B, *Ah, *Bh;
    u64 mask;
    u32 cs, co;
    u32 ia = 0, ib = 0, written = 0;
    u32 ha = 0, hb = 0;  // words of A from ia / of B from ib already in the rings
    E carry = uni_inf<WS>();  // the last output of the round before
    bool have_carry = false;
    u32 na, nb, nout;    // this round: words of A / of B in the rings, outputs
    u32 i0, i1, iend;    // co-ranks of the start and the end of this thread's outputs, and of nout
    __device__ __forceinline__ static u32 ra(u32 g) { return uni_pad(g & (T - 1)); }
    __device__ __forceinline__ static u32 rb(u32 g) { return uni_pad(T + (g & (T - 1))); }
    __device__ __forceinline__ E get(u32 slot) const { E e; e.lo = s_in[slot]; if constexpr (WS) e.hi = s_inh[slot]; return e; }
    __device__ __forceinline__ void put(u32 slot, const E& e) const { s_in[slot] = e.lo; if constexpr (WS) s_inh[slot] = e.hi; }
    // output q of the round sits in the q-th freed slot: A's ring first (iend of them), then B's
    __device__ __forceinline__ u32 oslot(u32 q) const { return q < iend ? ra(ia + q) : rb(ib + (q - iend)); }
    __device__ __forceinline__ bool more() const { return ia < cs || ib < co; }
    __device__ __forceinline__ void stage() {
        const u32 tid = threadIdx.x;
        na = cs - ia < T ? cs - ia : T; nb = co - ib < T ? co - ib : T; nout = na + nb < T ? na + nb : T;
        for (u32 g = ia + ha + tid; g < ia + na; g += UNI_THREADS) {
            if constexpr (WS) { s_in[ra(g)] = A[g]; s_inh[ra(g)] = Ah[g] & mask; }
            else s_in[ra(g)] = A[g] & mask;
        }
        for (u32 g = ib + hb + tid; g < ib + nb; g += UNI_THREADS) {
            if constexpr (WS) { s_in[rb(g)] = B[g]; s_inh[rb(g)] = Bh[g] & mask; }
            else s_in[rb(g)] = B[g] & mask;
        }
        __syncthreads();
    }
    // co-rank of the end of this thread's outputs — how many of the first d1 outputs come from A — by a binary search on the round's diagonal; its
    // start comes from the neighbour
    __device__ __forceinline__ void split() {
        const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
        const u32 d1 = (tid + 1) * UNI_ITEMS < nout ? (tid + 1) * UNI_ITEMS : nout;
        u32 lo = d1 > nb ? d1 - nb : 0u, hi = d1 < na ? d1 : na;
        while (lo < hi) {
            const u32 mid = (lo + hi) >> 1;
            if (!uni_lt<WS>(get(rb(ib + d1 - 1 - mid)), get(ra(ia + mid)))) lo = mid + 1; else hi = mid;  // A[mid] <= B[d1 - 1 - mid]: ties take A's copy first
        }
        i1 = lo;
        if (lane == 63) s_split[w + 1] = i1;
        if (tid == 0) s_split[0] = 0;
        __syncthreads();
        i0 = __shfl_up(i1, 1, 64);
        if (lane == 0) i0 = s_split[w];
        iend = s_split[NW];  // co-rank of nout (the last thread's end)
    }
    // the thread's UNI_ITEMS outputs o[], merged from its candidates a[] (A from i0 on, kept for the caller) and B's from d0 - i0 on with a fixed
    // network: min(a[k], b[n-1-k]) leaves the n smallest as a bitonic sequence, log2 n compare-exchange stages sort it
    __device__ __forceinline__ void merge(E (&a)[UNI_ITEMS], E (&o)[UNI_ITEMS]) const {
        const u32 tid = threadIdx.x;
        const u32 d0 = tid * UNI_ITEMS < nout ? tid * UNI_ITEMS : nout, j0 = d0 - i0;
        E b[UNI_ITEMS];
#pragma unroll
        for (int k = 0; k < UNI_ITEMS; ++k) {
            const u32 x = i0 + k, y = j0 + k;
            a[k] = uni_sel<WS>(x < na, get(ra(ia + (x < na ? x : 0u))), uni_inf<WS>());
            b[k] = uni_sel<WS>(y < nb, get(rb(ib + (y < nb ? y : 0u))), uni_inf<WS>());
        }
#pragma unroll
        for (int k = 0; k < UNI_ITEMS; ++k) o[k] = uni_sel<WS>(uni_lt<WS>(a[k], b[UNI_ITEMS - 1 - k]), a[k], b[UNI_ITEMS - 1 - k]);
#pragma unroll
        for (int st = UNI_ITEMS / 2; st >= 1; st >>= 1)
#pragma unroll
            for (int k = 0; k < UNI_ITEMS; ++k)
                if ((k & st) == 0) uni_cmpx<WS>(o[k], o[k + st]);
    }
    // the outputs take the place of what the round consumed (the caller synchronises before it reads them)
    __device__ __forceinline__ void write_back(const E (&o)[UNI_ITEMS]) const {
        __syncthreads();  // every read of the chunks is done
#pragma unroll
        for (int k = 0; k < UNI_ITEMS; ++k) {
            const u32 q = threadIdx.x * UNI_ITEMS + k;
            if (q < nout) put(oslot(q), o[k]);  // (nothing past nout: those slots hold words of the next round)
        }
    }
    // end of a round that wrote `tot` words and whose last output was `last`: the co-rank of that output says how far either list was consumed
    __device__ __forceinline__ void advance(u32 tot, const E& last) {
        carry = last;
        have_carry = true;
        written += tot;
        ha = na - iend;
        hb = nb - (nout - iend);
        ia += iend;
        ib += nout - iend;
        __syncthreads();  // the next round refills the freed slots and rewrites the split table
    }
};
template <bool WS>
__global__ __launch_bounds__(UNI_THREADS) void k_bucket_union(const BDesc* __restrict__ list, const u32* __restrict__ list_n, const u32* __restrict__ m_cs,
                                                              const u64* __restrict__ m_sstart, const u64* __restrict__ m_ostart, const u64* __restrict__ s_lo,
                                                              const u64* __restrict__ s_hi, const u64* __restrict__ o_lo, const u64* __restrict__ o_hi,
                                                              u64* __restrict__ out_lo, u64* __restrict__ out_hi, u32 SB, u32* __restrict__ out_count,
                                                              u8* __restrict__ out_kind) {
    typedef UniE<WS> E;
    typedef UniRounds<WS> R;
    constexpr int NW = R::NW;
    __shared__ u64 s_in[R::SLOTS];
    __shared__ u64 s_inh[WS ? R::SLOTS : 1];  // (wide suffixes: the high halves, same slots)
    __shared__ u32 s_split[NW + 1];
    __shared__ u32 s_wtot[NW + 1];
    if (blockIdx.x >= *list_n) return;
    const BDesc dsc = list[blockIdx.x];
    const u32 r = dsc.r, c = dsc.c & BDESC_LEN_MASK, cs = m_cs[r];
    const u64 a_self = m_sstart[r], a_oth = m_ostart[r];
    u64* __restrict__ dst = out_lo + dsc.start;
    u64* __restrict__ dsth = WS ? out_hi + dsc.start : nullptr;
    const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    R m{s_in, s_inh, s_split, s_lo + a_self, o_lo + a_oth, WS ? s_hi + a_self : nullptr, WS ? o_hi + a_oth : nullptr, suffix_mask<WS>(SB), cs, c - cs};
    while (m.more()) {
        m.stage();
        m.split();
        E a[UNI_ITEMS], o[UNI_ITEMS];
        m.merge(a, o);
        m.write_back(o);
        __syncthreads();
        // ordered compaction of the outputs that differ from their predecessor (equal = other's copy of a word self holds: dropped)
        E v[UNI_ITEMS];
        bool head[UNI_ITEMS];
#pragma unroll
        for (int j = 0; j < UNI_ITEMS; ++j) {
            const u32 p = w * (64 * UNI_ITEMS) + j * 64 + lane;
            const bool live = p < m.nout;
            v[j] = m.get(m.oslot(live ? p : 0u));
            const E u = m.get(m.oslot((live && p) ? p - 1 : 0u));
            head[j] = live && (p ? !uni_eq<WS>(v[j], u) : (!m.have_carry || !uni_eq<WS>(v[j], m.carry)));
        }
        const E last = m.get(m.oslot(m.nout - 1));
        u32 before[UNI_ITEMS];
        const u32 tot = count_before<NW, UNI_ITEMS>(head, s_wtot, before);
#pragma unroll
        for (int j = 0; j < UNI_ITEMS; ++j)
            if (head[j]) {
                dst[m.written + before[j]] = v[j].lo;
                if constexpr (WS) dsth[m.written + before[j]] = v[j].hi;
            }
        m.advance(tot, last);
    }
    if (tid == 0) { out_count[r] = m.written; out_kind[r] = KIND_TRIE; }
}

// ---- `&mut a OP &mut b` into a new index (cblx_set_op; /root/reference/src/wordset/set_ops.rs:78-121, 159-190, 241-279, 319-364 walk the
// two prefix bitvectors, src/trievec/set_ops.rs:5-41, 73-99, 131-161, 189-224 the buckets): a bucket only one side holds is cloned as
// stored, a bucket both hold becomes TrieOrVec::Vec(sorted OP of the two sorted iterators) — always a Vec, ascending, dropped when empty;
// iter_sorted leaves the Vec buckets of either operand sorted on the prefixes both hold. --------------------------------------------------
// One thread per candidate prefix, after k_merge_table (cap = cs + co on entry): the run capacity becomes the op's upper bound, a one-sided bucket
// gets its final count and kind (it is cloned as stored), a both-sided one joins the `both` list, and each of its Vec sides of two words or more
// joins the list of the sorting class of its length ([side][0]: one workgroup's LDS radix sort, [side][1]: the general kernel) with the run in the
// OPERAND's arena as its descriptor — sorted in place there, which is the side effect the reference has.
// ASSIGN (`a &= &mut b`, `a -= &mut b`, `a ^= &mut b`): a both-sided bucket keeps a's kind and joins the list of its kernel — [0] a's side a Trie
// (k_bucket_setop), [1] a's side a Vec of up to SA_LDS words (k_bucket_setop_assign, tables in LDS), [2] a longer Vec (tables in `scratch`, 3 cs + 1
// words from BDesc.start on; the sum of those goes to scratch_n, which the other form never touches).
static const u32 SETOP_SORT_LDS = 512 * MED_ITEMS;  // k_bucket_medium<512>'s capacity
static const int SA_THREADS = 256;
static const u32 SA_LDS = 1024;
template <bool ASSIGN>
__global__ __launch_bounds__(CLASSIFY_THREADS) void k_setop_plan(u64 nb, u32 op, u32* __restrict__ cap, const u32* __restrict__ m_cs, u32* __restrict__ m_co,
                                                                  const u64* __restrict__ m_sstart, const u64* __restrict__ m_ostart, const u8* __restrict__ m_skind,
                                                                  const u8* __restrict__ m_okind, u32* __restrict__ out_count, u8* __restrict__ out_kind,
                                                                  BDesc* __restrict__ sort_lists /* [2 sides][2 classes][nb] */,
                                                                  BDesc* __restrict__ both_lists /* [NBOTH][nb] */, u32* __restrict__ list_n /* [4] sort lists, [NBOTH] both */,
                                                                  unsigned long long* __restrict__ scratch_n /* ASSIGN only */) {
    constexpr int NBOTH = ASSIGN ? 3 : 1;
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    int cls_a = -1, cls_b = -1, cls_both = -1;
    u32 cs = 0, co = 0;
    u64 off = 0;
    if (r < nb) {
        cs = m_cs[r];
        co = cap[r] - cs;
        m_co[r] = co;
        if (cs != 0 && co != 0) {
            cap[r] = op == SETOP_AND ? (cs < co ? cs : co) : op == SETOP_SUB ? cs : cs + co;
            out_count[r] = 0;  // (written by the bucket's kernel)
            if constexpr (ASSIGN) {
                out_kind[r] = m_skind[r];
                cls_both = m_skind[r] == KIND_TRIE ? 0 : cs <= SA_LDS ? 1 : 2;
                if (cls_both == 2) off = atomicAdd(scratch_n, 3ull * cs + 1ull);  // (long Vecs are rare: one atomic each)
            } else {
                out_kind[r] = KIND_VEC;
                cls_both = 0;
            }
            if (m_skind[r] == KIND_VEC && cs > 1) cls_a = cs <= SETOP_SORT_LDS ? 0 : 1;
            if (m_okind[r] == KIND_VEC && co > 1) cls_b = co <= SETOP_SORT_LDS ? 0 : 1;
        } else {  // one-sided (never for AND, never b's side for SUB: such prefixes are no candidates): cloned as stored
            cap[r] = cs + co;
            out_count[r] = cs + co;
            out_kind[r] = cs ? m_skind[r] : m_okind[r];
        }
    }
    const u32 slot_a = block_append<CLASSIFY_THREADS, 2>(cls_a, list_n);
    if (cls_a >= 0) sort_lists[(u64)cls_a * nb + slot_a] = BDesc{m_sstart[r], cs | BDESC_TRIE, (u32)r};  // (TRIE: the kernel leaves the run sorted)
    __syncthreads();  // block_append's tables are reused
    const u32 slot_b = block_append<CLASSIFY_THREADS, 2>(cls_b, list_n + 2);
    if (cls_b >= 0) sort_lists[(u64)(2 + cls_b) * nb + slot_b] = BDesc{m_ostart[r], co | BDESC_TRIE, (u32)r};
    const u32 slot = block_append<CLASSIFY_THREADS, NBOTH>(cls_both, list_n + 4);
    if (cls_both >= 0) both_lists[(u64)cls_both * nb + slot] = BDesc{off, 0, (u32)r};
}
// LPB lanes per candidate: a one-sided bucket is copied into its run as stored
template <bool WS, int LPB>
__global__ __launch_bounds__(256) void k_setop_gather(u64 nb, const u64* __restrict__ start, const u32* __restrict__ m_cs, const u32* __restrict__ m_co,
                                                      const u64* __restrict__ m_sstart, const u64* __restrict__ m_ostart, const u64* __restrict__ s_lo,
                                                      const u64* __restrict__ s_hi, const u64* __restrict__ o_lo, const u64* __restrict__ o_hi,
                                                      u64* __restrict__ out_lo, u64* __restrict__ out_hi) {
    const u64 r = ((u64)blockIdx.x * 256 + threadIdx.x) / LPB;
    if (r >= nb) return;
    const u32 lane = threadIdx.x & (LPB - 1);
    const u32 cs = m_cs[r], co = m_co[r];
    if (cs != 0 && co != 0) return;
    const u64 d0 = start[r], src = cs ? m_sstart[r] : m_ostart[r];
    const u64* __restrict__ lo = cs ? s_lo : o_lo;
    const u64* __restrict__ hi = cs ? s_hi : o_hi;
    for (u32 j = lane; j < cs + co; j += LPB) {
        out_lo[d0 + j] = lo[src + j];
        if constexpr (WS) out_hi[d0 + j] = hi[src + j];
    }
}
// Both-sided buckets: k_bucket_union's rounds (two staging rings, co-rank on the round's diagonal, register merge network, ordered compaction by
// ballot) with another keep-predicate. Both lists are duplicate-free, so a value occurs once or twice in the merged sequence, a's copy first:
//   OR keeps what differs from its predecessor, AND what equals it (the second of a pair), XOR what differs from both neighbours, SUB what
//   differs from both neighbours and came from a.
// ORIGIN (SUB): the merge network loses it. No tag bit is used — a bit above the suffix is free below 64 bits and in the high half of a wide
// suffix, but not at SUFFIX_BITS = 64, and a tagged all-ones suffix would have to be kept apart from the network's padding value. Instead the
// thread that merged an output knows how many of its outputs came from a (the difference of its two co-ranks) and still holds exactly those
// candidates in registers: an output that equals none of them came from b. (One that equals one of them is a's copy or b's copy of a PAIR, which SUB
// drops on its neighbours alone, so the answer is exact wherever it is used.) The same code serves every suffix width; the flags travel to the
// compaction through one LDS word per thread.
// ROUND EDGES: a's copy of a pair may be the last output of a round and b's copy the first of the next. The last output of every round is therefore
// HELD BACK — its value, whether it equals its predecessor and where it came from stay in registers — and is decided as the first element of the
// next round, when its successor is known; after the last round it has no successor. A round thus emits [held-back value, outputs 0 .. nout-2].
template <bool WS, u32 OP>
__global__ __launch_bounds__(UNI_THREADS) void k_bucket_setop(const BDesc* __restrict__ list, const u32* __restrict__ list_n, const u32* __restrict__ m_cs,
                                                              const u32* __restrict__ m_co, const u64* __restrict__ m_sstart, const u64* __restrict__ m_ostart,
                                                              const u64* __restrict__ s_lo, const u64* __restrict__ s_hi, const u64* __restrict__ o_lo,
                                                              const u64* __restrict__ o_hi, const u64* __restrict__ run_start, u64* __restrict__ out_lo,
                                                              u64* __restrict__ out_hi, u32 SB, u32* __restrict__ out_count, u8* __restrict__ out_kind) {
    typedef UniE<WS> E;
    typedef UniRounds<WS> R;
    constexpr int NW = R::NW;
    static_assert(UNI_ITEMS <= 32, "one origin bit per output in a 32-bit word");
    __shared__ u64 s_in[R::SLOTS];
    __shared__ u64 s_inh[WS ? R::SLOTS : 1];
    __shared__ u32 s_org[OP == SETOP_SUB ? UNI_THREADS : 1];  // bit k of word t: output t * UNI_ITEMS + k of the round came from a
    __shared__ u32 s_split[NW + 1];
    __shared__ u32 s_wtot[NW + 1];
    if (blockIdx.x >= *list_n) return;
    const u32 r = list[blockIdx.x].r, cs = m_cs[r], co = m_co[r];
    const u64 a_self = m_sstart[r], a_oth = m_ostart[r], d_run = run_start[r];
    u64* __restrict__ dst = out_lo + d_run;
    u64* __restrict__ dsth = WS ? out_hi + d_run : nullptr;
    const u32 tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    auto keep_rule = [](bool eqp, bool eqn, bool from_a) {
        return OP == SETOP_OR ? !eqp : OP == SETOP_AND ? eqp : OP == SETOP_XOR ? (!eqp && !eqn) : (from_a && !eqp && !eqn);
    };
    R m{s_in, s_inh, s_split, s_lo + a_self, o_lo + a_oth, WS ? s_hi + a_self : nullptr, WS ? o_hi + a_oth : nullptr, suffix_mask<WS>(SB), cs, co};
    bool carry_eqp = false, carry_a = false;  // of m.carry, the held-back output
    while (m.more()) {
        m.stage();
        m.split();
        E a[UNI_ITEMS], o[UNI_ITEMS];
        m.merge(a, o);
        u32 org = 0;
        if constexpr (OP == SETOP_SUB) {
            const u32 from_a = m.i1 - m.i0;  // a[0 .. from_a) are the thread's outputs that came from a
#pragma unroll
            for (int k = 0; k < UNI_ITEMS; ++k) {
                bool fa = false;
#pragma unroll
                for (int j = 0; j < UNI_ITEMS; ++j) fa = fa || ((u32)j < from_a && uni_eq<WS>(o[k], a[j]));
                org |= fa ? 1u << k : 0u;
            }
        }
        m.write_back(o);
        if constexpr (OP == SETOP_SUB) s_org[tid] = org;
        __syncthreads();
        auto org_of = [&](u32 q) { return OP == SETOP_SUB ? ((s_org[q / UNI_ITEMS] >> (q % UNI_ITEMS)) & 1u) != 0 : false; };
        const u32 nout = m.nout;
        // emit slot e of the round holds output e - 1 (slot 0: the value held back); its successor is output e
        E v[UNI_ITEMS];
        bool keep[UNI_ITEMS];
#pragma unroll
        for (int j = 0; j < UNI_ITEMS; ++j) {
            const u32 e = w * (64 * UNI_ITEMS) + j * 64 + lane;
            const bool in = e < nout;
            const E succ = m.get(m.oslot(in ? e : 0u));
            const E x1 = m.get(m.oslot(in && e >= 1 ? e - 1 : 0u)), x2 = m.get(m.oslot(in && e >= 2 ? e - 2 : 0u));
            v[j] = uni_sel<WS>(e >= 1, x1, m.carry);
            const E pred = uni_sel<WS>(e >= 2, x2, m.carry);
            const bool eqp = e == 0 ? carry_eqp : ((e >= 2 || m.have_carry) && uni_eq<WS>(v[j], pred));
            const bool from_a = e == 0 ? carry_a : org_of(in && e >= 1 ? e - 1 : 0u);
            keep[j] = in && (e >= 1 || m.have_carry) && keep_rule(eqp, uni_eq<WS>(v[j], succ), from_a);
        }
        // the round's last output is held back
        const E last = m.get(m.oslot(nout - 1));
        const E before_last = uni_sel<WS>(nout >= 2, m.get(m.oslot(nout >= 2 ? nout - 2 : 0u)), m.carry);
        const bool last_eqp = (nout >= 2 || m.have_carry) && uni_eq<WS>(last, before_last);
        const bool last_a = org_of(nout - 1);
        u32 before[UNI_ITEMS];
        const u32 tot = count_before<NW, UNI_ITEMS>(keep, s_wtot, before);
#pragma unroll
        for (int j = 0; j < UNI_ITEMS; ++j)
            if (keep[j]) {
                dst[m.written + before[j]] = v[j].lo;
                if constexpr (WS) dsth[m.written + before[j]] = v[j].hi;
            }
        carry_eqp = last_eqp;
        carry_a = last_a;
        m.advance(tot, last);
    }
    if (tid == 0) {
        u32 written = m.written;
        if (m.have_carry && keep_rule(carry_eqp, false, carry_a)) {  // the last value of the merged sequence has no successor
            dst[written] = m.carry.lo;
            if constexpr (WS) dsth[written] = m.carry.hi;
            ++written;
        }
        out_count[r] = written;
        if (out_kind) out_kind[r] = KIND_VEC;  // (null: the bucket keeps the kind the plan gave it)
    }
}
// the candidates that keep at least one word stay in the directory
__global__ void k_setop_live(u64 nb, const u32* __restrict__ cnt, u32* __restrict__ live) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r < nb) live[r] = cnt[r] != 0 ? 1u : 0u;
}
// ... and move to their new rank (ascending prefixes stay ascending); their bits make up the result's bitvector (zeroed by the caller)
__global__ void k_setop_compact(u64 nb, const u32* __restrict__ cnt, const u64* __restrict__ new_rank, const u32* __restrict__ prefix, const u64* __restrict__ start,
                                const u8* __restrict__ kind, u32* __restrict__ o_prefix, u64* __restrict__ o_start, u32* __restrict__ o_cnt, u8* __restrict__ o_kind,
                                u64* __restrict__ bv) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nb || cnt[r] == 0) return;
    const u64 n = new_rank[r];
    const u32 p = prefix[r];
    o_prefix[n] = p;
    o_start[n] = start[r];
    o_cnt[n] = cnt[r];
    o_kind[n] = kind[r];
    atomicOr((unsigned long long*)&bv[p >> 6], 1ull << (p & 63));
}

// ---- CBL::merge / CBL::intersect of n operands (cblx_set_op_many; /root/reference/src/cbl.rs:106-124 -> src/wordset/set_ops.rs:11-42, 49-75) ----------
// Per distinct prefix the reference gets the operands that hold it. merge: one holder -> cloned as stored; two or more -> every holder's Vec is sorted
// (iter_sorted) and the result is Vec(ascending union), whatever its length. intersect: only prefixes ALL operands hold; every holder's Vec is sorted, the
// result is Vec(ascending intersection), dropped when empty — also for n = 1, which turns every bucket into an ascending Vec.
// A candidate bucket carries a 64-bit holder mask (hence at most 64 operands); nothing of size [buckets][operands] exists: a holder's rank in its own
// directory is rank_dir[word] + popc(bits below), recomputed where its run is needed.
static const u32 MANY_MAX = 64;  // = CBLX_SETOP_MAX_OPERANDS
// words of all holders of a bucket that k_bucket_setop_many stages in LDS: up to MANY_SMALL one wave and 2 KB (4 KB wide), up to MANY_LDS four waves and
// 24 KB (40 KB wide: 6 / 4 workgroups per CU); longer buckets are folded pairwise by k_bucket_setop (tests/test_gpu_setops_many.py mirrors both)
static const u32 MANY_SMALL = 256, MANY_LDS = 2048;
struct ManyOp { DirView d; const u64* lo; const u64* hi; };  // one operand: its directory and its arena

__global__ void k_many_bv(u64 nwords, const ManyOp* __restrict__ ops, u32 n, u32 op, u64* __restrict__ out, u32* __restrict__ popc) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    u64 v = ops[0].d.bv[w];
    for (u32 i = 1; i < n; ++i) { const u64 x = ops[i].d.bv[w]; v = op == SETOP_AND ? (v & x) : (v | x); }
    out[w] = v;
    popc[w] = (u32)__builtin_popcountll(v);
}
// One thread per prefix slot of the candidate bitvector: holder mask, run capacity (merge: sum of the holders' counts, intersect: the smallest) and the
// bucket's fate — a merge bucket with one holder gets its final count and kind (k_many_gather clones it), every other one joins the list of its route:
// [0] up to MANY_SMALL words of all holders, [1] up to MANY_LDS, [2] longer. BDesc.c = words of all holders.
__global__ __launch_bounds__(CLASSIFY_THREADS) void k_many_table(u64 nprefix, const u64* __restrict__ bv, const u64* __restrict__ rank_dir, const ManyOp* __restrict__ ops, u32 n,
                                                                  u32 op, u64 nb, u32* __restrict__ bucket_prefix, u64* __restrict__ hmask, u32* __restrict__ cap,
                                                                  u32* __restrict__ out_count, u8* __restrict__ out_kind, BDesc* __restrict__ lists /* [3][nb] */,
                                                                  u32* __restrict__ list_n) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    int cls = -1;
    u64 r = 0;
    u32 sum = 0;
    if (p < nprefix) {
        const u64 w = bv[p >> 6];
        if ((w >> (p & 63)) & 1ull) {
            r = rank_dir[p >> 6] + (u64)__builtin_popcountll(w & ((1ull << (p & 63)) - 1ull));
            u64 mask = 0;
            u32 mn = 0xFFFFFFFFu;
            u8 k0 = KIND_VEC;
            for (u32 i = 0; i < n; ++i) {
                u64 rank;
                if (!dir_lookup(ops[i].d, (u32)p, rank)) continue;
                const u32 c = ops[i].d.count[rank];
                if (!mask) k0 = ops[i].d.kind[rank];
                mask |= 1ull << i;
                sum += c;
                mn = c < mn ? c : mn;
            }
            bucket_prefix[r] = (u32)p;
            hmask[r] = mask;
            if (op == SETOP_OR && (mask & (mask - 1ull)) == 0) {
                cap[r] = sum;
                out_count[r] = sum;
                out_kind[r] = k0;
            } else {
                cap[r] = op == SETOP_AND ? mn : sum;
                out_count[r] = 0;  // (written by the bucket's kernel)
                out_kind[r] = KIND_VEC;
                cls = sum <= MANY_SMALL ? 0 : sum <= MANY_LDS ? 1 : 2;
            }
        }
    }
    const u32 slot = block_append<CLASSIFY_THREADS, 3>(cls, list_n);
    if (cls >= 0) lists[(u64)cls * nb + slot] = BDesc{0, sum, (u32)r};
}
// LPB lanes per candidate (merge): a bucket one operand holds is copied into its run as stored — k_setop_gather's n-ary twin
template <bool WS, int LPB>
__global__ __launch_bounds__(256) void k_many_gather(u64 nb, const u64* __restrict__ start, const u32* __restrict__ bucket_prefix, const u64* __restrict__ hmask,
                                                     const ManyOp* __restrict__ ops, u64* __restrict__ out_lo, u64* __restrict__ out_hi) {
    const u64 r = ((u64)blockIdx.x * 256 + threadIdx.x) / LPB;
    if (r >= nb) return;
    const u32 lane = threadIdx.x & (LPB - 1);
    const u64 mask = hmask[r];
    if (mask & (mask - 1ull)) return;
    const ManyOp o = ops[__builtin_ctzll(mask)];
    u64 rank;
    if (!dir_lookup(o.d, bucket_prefix[r], rank)) return;
    const u64 d0 = start[r], src = o.d.start[rank];
    const u32 c = o.d.count[rank];
    for (u32 j = lane; j < c; j += LPB) {
        out_lo[d0 + j] = o.lo[src + j];
        if constexpr (WS) out_hi[d0 + j] = o.hi[src + j];
    }
}
// One thread per candidate, once per operand: the operand's Vec bucket of two words or more on a prefix the reference visits with iter_sorted (merge: two
// holders or more; intersect: every candidate) joins the list of its sorting class, with the run in the OPERAND's arena as descriptor (as k_setop_plan)
__global__ __launch_bounds__(CLASSIFY_THREADS) void k_many_sortplan(u64 nb, const u32* __restrict__ bucket_prefix, const u64* __restrict__ hmask, u32 op,
                                                                     const ManyOp* __restrict__ ops, u32 i, BDesc* __restrict__ sort_lists /* [2][nb] */,
                                                                     u32* __restrict__ list_n) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    int cls = -1;
    u64 st = 0;
    u32 c = 0;
    if (r < nb) {
        const u64 mask = hmask[r];
        u64 rank;
        if (((mask >> i) & 1ull) && (op == SETOP_AND || (mask & (mask - 1ull)) != 0) && dir_lookup(ops[i].d, bucket_prefix[r], rank)) {
            c = ops[i].d.count[rank];
            st = ops[i].d.start[rank];
            if (ops[i].d.kind[rank] == KIND_VEC && c > 1) cls = c <= SETOP_SORT_LDS ? 0 : 1;
        }
    }
    const u32 slot = block_append<CLASSIFY_THREADS, 2>(cls, list_n);
    if (cls >= 0) sort_lists[(u64)cls * nb + slot] = BDesc{st, c | BDESC_TRIE, (u32)r};  // (TRIE: the kernel leaves the run sorted)
}
// One workgroup per bucket of up to CAP words over all its m holders, whose runs are ascending and duplicate-free by now. The runs are staged back to back
// in LDS (lane t of the first wave looks up operand t; a wave scan of the counts gives the offsets).
//   OR: every element finds its position in the merged multiset by one binary search per other run — runs of lower index count their elements <= it, runs of
//       higher index those < it, so the lowest holder's copy of a value comes first — and the searches in the lower runs also say whether one of them holds
//       the value: then this copy is not kept. (element index, kept) goes to the merged position; an ordered compaction by ballot / mbcnt / wave totals writes
//       the kept ones out. No tag bit in the suffix and no padding value: SUFFIX_BITS = 64 has no free bit and all-ones is a legal suffix.
//   AND: the elements of the shortest holder (the lowest one on ties) are searched in every other run and kept when all hold them; same compaction.
template <bool WS, u32 OP, u32 CAP, int THREADS>
__global__ __launch_bounds__(THREADS) void k_bucket_setop_many(const BDesc* __restrict__ list, const u32* __restrict__ list_n, const u32* __restrict__ bucket_prefix,
                                                               const u64* __restrict__ hmask, const ManyOp* __restrict__ ops, const u64* __restrict__ run_start,
                                                               u64* __restrict__ out_lo, u64* __restrict__ out_hi, u32 SB, u32* __restrict__ out_count) {
    typedef UniE<WS> E;
    static_assert(OP == SETOP_OR || OP == SETOP_AND, "the reference has no n-ary SUB / XOR");
    static_assert(THREADS % 64 == 0, "whole waves");
    constexpr int NW = THREADS / 64;
    __shared__ u64 s_lo[CAP];
    __shared__ u64 s_hi[WS ? CAP : 1];
    __shared__ u32 s_perm[OP == SETOP_OR ? CAP : 1];  // merged position -> element | kept << 31
    __shared__ u64 s_src[MANY_MAX];                    // holder k: first arena slot of its run,
    __shared__ u32 s_opi[MANY_MAX];                    // its operand,
    __shared__ u32 s_off[MANY_MAX + 1];                // and where its run starts in s_lo; [m] = words of all holders
    __shared__ u32 s_wtot[NW];
    if (blockIdx.x >= *list_n) return;
    const u32 r = list[blockIdx.x].r;
    const u64 holders = hmask[r];
    const u32 p = bucket_prefix[r], m = (u32)__builtin_popcountll(holders);
    const u64 mask = suffix_mask<WS>(SB);
    const u32 tid = threadIdx.x, lane = tid & 63;
    if (tid < 64) {
        const bool holds = ((holders >> tid) & 1ull) != 0;
        u32 c = 0;
        u64 st = 0, rank;
        if (holds && dir_lookup(ops[tid].d, p, rank)) { c = ops[tid].d.count[rank]; st = ops[tid].d.start[rank]; }
        u32 inc = c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) { const u32 t = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += t; }
        if (holds) {
            const u32 k = (u32)__builtin_popcountll(holders & ((1ull << tid) - 1ull));
            s_off[k] = inc - c;
            s_src[k] = st;
            s_opi[k] = tid;
        }
        if (tid == 63) s_off[m] = inc;
    }
    __syncthreads();
    const u32 total = s_off[m] < CAP ? s_off[m] : CAP;  // (the list's class says total <= CAP)
    auto run_of = [&](u32 e) { u32 k = 0; while (k + 1 < m && s_off[k + 1] <= e) ++k; return k; };
    auto get = [&](u32 i) { E e; e.lo = s_lo[i]; if constexpr (WS) e.hi = s_hi[i]; return e; };
    for (u32 e = tid; e < total; e += THREADS) {
        const u32 k = run_of(e);
        const ManyOp& o = ops[s_opi[k]];
        const u64 g = s_src[k] + (e - s_off[k]);
        if constexpr (WS) { s_lo[e] = o.lo[g]; s_hi[e] = o.hi[g] & mask; }
        else s_lo[e] = o.lo[g] & mask;
        if constexpr (OP == SETOP_OR) s_perm[e] = 0;
    }
    __syncthreads();
    u64* __restrict__ dst = out_lo + run_start[r];
    u64* __restrict__ dsth = WS ? out_hi + run_start[r] : nullptr;
    // first index in [a, b) whose element is not below v (UPPER: is above v)
    auto bound = [&](u32 a, u32 b, const E& v, bool upper) {
        while (a < b) {
            const u32 mid = (a + b) >> 1;
            const E x = get(mid);
            if (upper ? !uni_lt<WS>(v, x) : uni_lt<WS>(x, v)) a = mid + 1; else b = mid;
        }
        return a;
    };
    u32 ks = 0, len = total;
    if constexpr (OP == SETOP_OR) {
        for (u32 e = tid; e < total; e += THREADS) {
            const u32 k = run_of(e);
            const E v = get(e);
            u32 pos = e - s_off[k];
            bool dup = false;
            for (u32 kk = 0; kk < m; ++kk) {
                if (kk == k) continue;
                const u32 a = s_off[kk], at = bound(a, s_off[kk + 1] < total ? s_off[kk + 1] : total, v, kk < k);
                pos += at - a;
                if (kk < k && at > a && uni_eq<WS>(get(at - 1), v)) dup = true;
            }
            if (pos < total) s_perm[pos] = e | (dup ? 0u : 0x80000000u);
        }
        __syncthreads();
    } else {
        len = s_off[1] - s_off[0];
        for (u32 k = 1; k < m; ++k) { const u32 c = s_off[k + 1] - s_off[k]; if (c < len) { len = c; ks = k; } }
        if (s_off[ks] + len > total) len = 0;
    }
    u32 written = 0;
    for (u32 base = 0; base < len; base += THREADS) {
        const u32 q = base + tid;
        bool keep = q < len;
        u32 src = 0;
        if constexpr (OP == SETOP_OR) {
            const u32 pe = keep ? s_perm[q] : 0u;
            keep = (pe >> 31) != 0;
            src = pe & 0x7FFFFFFFu;
        } else if (keep) {
            src = s_off[ks] + q;
            const E v = get(src);
            for (u32 kk = 0; kk < m && keep; ++kk) {
                if (kk == ks) continue;
                const u32 b = s_off[kk + 1] < total ? s_off[kk + 1] : total, at = bound(s_off[kk], b, v, false);
                keep = at < b && uni_eq<WS>(get(at), v);
            }
        }
        u32 before;
        const u32 tot = count_before<NW>(keep, s_wtot, before);
        if (keep) {
            dst[written + before] = s_lo[src];
            if constexpr (WS) dsth[written + before] = s_hi[src];
        }
        written += tot;
        __syncthreads();  // s_wtot is rewritten
    }
    if (tid == 0) out_count[r] = written;
}
// ---- the long route: a bucket whose holders have more than MANY_LDS words is folded holder by holder with k_bucket_setop over two scratch runs of
// sum-of-counts words each (X at sc_start[q], Y at S + sc_start[q]; q = the bucket's place in the long list). acc_side[q] says which one holds the
// accumulator: a step whose operand does not hold the bucket leaves it where it is.
// the accumulator starts as the lowest holder's run (ascending by now), suffix bits only
template <bool WS>
__global__ __launch_bounds__(256) void k_many_long_init(const BDesc* __restrict__ list, u32 nlong, const u32* __restrict__ bucket_prefix, const u64* __restrict__ hmask,
                                                        const ManyOp* __restrict__ ops, const u64* __restrict__ sc_start, u64* __restrict__ sc_lo, u64* __restrict__ sc_hi,
                                                        u32 SB, u32* __restrict__ acc_cnt, u8* __restrict__ acc_side) {
    const u32 q = blockIdx.x;
    if (q >= nlong) return;
    const u32 r = list[q].r;
    const ManyOp o = ops[__builtin_ctzll(hmask[r])];
    u64 rank;
    if (!dir_lookup(o.d, bucket_prefix[r], rank)) return;
    const u64 mask = suffix_mask<WS>(SB);
    const u64 src = o.d.start[rank], d0 = sc_start[q];
    const u32 c = o.d.count[rank];
    for (u32 j = threadIdx.x; j < c; j += 256) {
        if constexpr (WS) { sc_lo[d0 + j] = o.lo[src + j]; sc_hi[d0 + j] = o.hi[src + j] & mask; }
        else sc_lo[d0 + j] = o.lo[src + j] & mask;
    }
    if (threadIdx.x == 0) { acc_cnt[q] = c; acc_side[q] = 0; }
}
__global__ void k_many_long_words(const BDesc* __restrict__ list, u32 nlong, u32* __restrict__ words) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < nlong) words[q] = list[q].c;
}
// step i of the fold: the long buckets operand i holds (beyond their first holder, and unless an intersection is empty already) get k_bucket_setop's
// tables — a = the accumulator, b = operand i's run, output = the other scratch run — and change sides
__global__ __launch_bounds__(CLASSIFY_THREADS) void k_many_long_plan(const BDesc* __restrict__ list, u32 nlong, const u32* __restrict__ bucket_prefix,
                                                                      const u64* __restrict__ hmask, const ManyOp* __restrict__ ops, u32 i, u32 op,
                                                                      const u64* __restrict__ sc_start, u64 S, const u32* __restrict__ acc_cnt, u8* __restrict__ acc_side,
                                                                      u32* __restrict__ t_cs, u32* __restrict__ t_co, u64* __restrict__ t_sstart, u64* __restrict__ t_ostart,
                                                                      u64* __restrict__ t_run, BDesc* __restrict__ step_list, u32* __restrict__ step_n) {
    const u32 q = blockIdx.x * blockDim.x + threadIdx.x;
    int cls = -1;
    if (q < nlong) {
        const u32 r = list[q].r;
        const u64 mask = hmask[r];
        u64 rank;
        if (((mask >> i) & 1ull) && (u32)__builtin_ctzll(mask) != i && !(op == SETOP_AND && acc_cnt[q] == 0) && dir_lookup(ops[i].d, bucket_prefix[r], rank)) {
            const u8 side = acc_side[q];
            t_cs[q] = acc_cnt[q];
            t_co[q] = ops[i].d.count[rank];
            t_sstart[q] = sc_start[q] + (side ? S : 0ull);
            t_ostart[q] = ops[i].d.start[rank];
            t_run[q] = sc_start[q] + (side ? 0ull : S);
            acc_side[q] = side ^ 1;
            cls = 0;
        }
    }
    const u32 slot = block_append<CLASSIFY_THREADS, 1>(cls, step_n);
    if (cls >= 0) step_list[slot] = BDesc{0, 0, q};
}
// the accumulator becomes the result bucket
template <bool WS>
__global__ __launch_bounds__(256) void k_many_long_finish(const BDesc* __restrict__ list, u32 nlong, const u64* __restrict__ sc_start, u64 S, const u64* __restrict__ sc_lo,
                                                          const u64* __restrict__ sc_hi, const u32* __restrict__ acc_cnt, const u8* __restrict__ acc_side,
                                                          const u64* __restrict__ run_start, const u32* __restrict__ cap, u64* __restrict__ out_lo, u64* __restrict__ out_hi,
                                                          u32* __restrict__ out_count) {
    const u32 q = blockIdx.x;
    if (q >= nlong) return;
    const u32 r = list[q].r;
    const u32 c = acc_cnt[q] < cap[r] ? acc_cnt[q] : cap[r];  // (an intersection is no longer than its shortest holder, a union than all of them)
    const u64 src = sc_start[q] + (acc_side[q] ? S : 0ull), d0 = run_start[r];
    for (u32 j = threadIdx.x; j < c; j += 256) {
        out_lo[d0 + j] = sc_lo[src + j];
        if constexpr (WS) out_hi[d0 + j] = sc_hi[src + j];
    }
    if (threadIdx.x == 0) out_count[r] = c;
}

// ---- k-mers at least t of n operands hold, and how many k-mers exactly j hold (cblx_set_at_least / cblx_occupancy_counts) --------
// Ours, not the reference's. A prefix m operands hold is visited when m >= t (t >= 2; t = 1 is cblx_set_op_many's merge): every holder's Vec is sorted, the
// result is Vec(ascending {v : t holders or more hold v}), dropped when empty. The occupancy count visits what a merge visits, sorts what a merge sorts and
// writes no index: a one-holder bucket adds its length to hist[1] from the directory, a multi-held one tallies the holders of every distinct value.
// The candidates: per 64 prefixes a vertical counter over the n bitvector words — seven bit planes, a ripple-carry add per operand — compared with t
// bit-sliced from the lowest plane up (ge = the planes so far are >= t's bits so far).
__global__ void k_thresh_bv(u64 nwords, const ManyOp* __restrict__ ops, u32 n, u32 t, u64* __restrict__ out, u32* __restrict__ popc) {
    const u64 w = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwords) return;
    u64 c0 = 0, c1 = 0, c2 = 0, c3 = 0, c4 = 0, c5 = 0, c6 = 0;
    for (u32 i = 0; i < n; ++i) {
        u64 carry = ops[i].d.bv ? ops[i].d.bv[w] : 0ull, x;
        x = c0 & carry; c0 ^= carry; carry = x;
        x = c1 & carry; c1 ^= carry; carry = x;
        x = c2 & carry; c2 ^= carry; carry = x;
        x = c3 & carry; c3 ^= carry; carry = x;
        x = c4 & carry; c4 ^= carry; carry = x;
        x = c5 & carry; c5 ^= carry; carry = x;
        c6 ^= carry;  // (n <= 64: the count fits seven planes)
    }
    u64 ge = ~0ull;
    ge = (t & 1u) ? (c0 & ge) : (c0 | ge);
    ge = (t & 2u) ? (c1 & ge) : (c1 | ge);
    ge = (t & 4u) ? (c2 & ge) : (c2 | ge);
    ge = (t & 8u) ? (c3 & ge) : (c3 | ge);
    ge = (t & 16u) ? (c4 & ge) : (c4 | ge);
    ge = (t & 32u) ? (c5 & ge) : (c5 | ge);
    ge = (t & 64u) ? (c6 & ge) : (c6 | ge);
    out[w] = ge;
    popc[w] = (u32)__builtin_popcountll(ge);
}
// k_many_table's twin, one thread per prefix slot of the candidate bitvector: holder mask and the list of the bucket's route by the words of all holders.
// t >= 2 (`single` null): every candidate has t holders or more; its run takes sum / t words, since every output consumes t staged words or more.
// Counting (`single` given, t = 1): nothing has a run; a one-holder bucket leaves its length in single[r] and joins no list.
__global__ __launch_bounds__(CLASSIFY_THREADS) void k_thresh_table(u64 nprefix, const u64* __restrict__ bv, const u64* __restrict__ rank_dir, const ManyOp* __restrict__ ops, u32 n,
                                                                    u32 t, u64 nb, u32* __restrict__ bucket_prefix, u64* __restrict__ hmask, u32* __restrict__ cap,
                                                                    u32* __restrict__ out_count, u8* __restrict__ out_kind, BDesc* __restrict__ lists /* [3][nb] */,
                                                                    u32* __restrict__ list_n, u32* __restrict__ single) {
    const u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    int cls = -1;
    u64 r = 0;
    u32 sum = 0;
    if (p < nprefix) {
        const u64 w = bv[p >> 6];
        if ((w >> (p & 63)) & 1ull) {
            r = rank_dir[p >> 6] + (u64)__builtin_popcountll(w & ((1ull << (p & 63)) - 1ull));
            u64 mask = 0;
            for (u32 i = 0; i < n; ++i) {
                u64 rank;
                if (!dir_lookup(ops[i].d, (u32)p, rank)) continue;
                mask |= 1ull << i;
                sum += ops[i].d.count[rank];
            }
            bucket_prefix[r] = (u32)p;
            hmask[r] = mask;
            const bool one = (mask & (mask - 1ull)) == 0;
            if (single) single[r] = one ? sum : 0u;
            else {
                cap[r] = sum / t;
                out_count[r] = 0;  // (written by the bucket's kernel)
                out_kind[r] = KIND_VEC;
            }
            if (!(single && one)) cls = sum <= MANY_SMALL ? 0 : sum <= MANY_LDS ? 1 : 2;
        }
    }
    const u32 slot = block_append<CLASSIFY_THREADS, 3>(cls, list_n);
    if (cls >= 0) lists[(u64)cls * nb + slot] = BDesc{0, sum, (u32)r};
}
// One tally per holder count in LDS: the lanes of a wave that saw the same count h (0: nothing to tally) add their number with one LDS atomic. Every lane
// of the wave must call it.
__device__ __forceinline__ void tally_holders(u32 h, unsigned long long* s_tally) {
    const u32 lane = threadIdx.x & 63;
    u64 todo = __ballot(h != 0);
    while (todo) {
        const u32 leader = (u32)__builtin_ctzll(todo);
        const u32 hv = (u32)__shfl((int)h, (int)leader, 64);
        const u64 same = __ballot(h == hv);
        if (lane == leader) atomicAdd(&s_tally[hv], (unsigned long long)__builtin_popcountll(same));
        todo &= ~same;
    }
}
// the tallies of one workgroup become its row of `tally` ([gridDim.x][MANY_MAX + 1]); k_tally_sum adds the rows up
template <int THREADS> __device__ __forceinline__ void tally_flush(const unsigned long long* s_tally, u64* __restrict__ tally) {
    __syncthreads();
    for (u32 j = threadIdx.x; j <= MANY_MAX; j += THREADS) tally[(u64)blockIdx.x * (MANY_MAX + 1) + j] = s_tally[j];
}
// One round over the words staged in LDS, shared by the short routes and the long one. s_lo / s_hi hold m ascending, duplicate-free windows back to
// back, window k at [s_off[k], s_off[k + 1]), `total` words in all. It is k_bucket_setop_many's OR path — position search, (element, kept) to the merged
// position, ordered compaction by ballot / mbcnt / wave totals — plus a holder count per element: the search in a lower window (upper bound) says whether
// that window holds the value, as there; the search in a higher window (lower bound) needs one comparison at the bound. An element is kept when it is the
// lowest holder's copy and t windows or more hold it. ROUNDS: only the first s_act[k] elements of window k take part (`active` in all): they are the
// elements up to a value every window reaches, so every copy of them is staged and they stand at the merged positions 0 .. active - 1.
// COUNT: nothing is written but the tallies — the holders of every lowest copy. Otherwise the kept elements go to dst[written ...) below `room`; returns
// how many. Every thread of the workgroup must call it; s_perm and s_wtot are free again when it returns.
template <bool WS, bool COUNT, bool ROUNDS, int THREADS>
__device__ __forceinline__ u32 atleast_round(const u64* s_lo, const u64* s_hi, u32* s_perm, const u32* s_off, const u32* s_act, u32 m, u32 total, u32 active, u32 t,
                                             u32* s_wtot, unsigned long long* s_tally, u64* __restrict__ dst, u64* __restrict__ dsth, u32 written, u32 room) {
    typedef UniE<WS> E;
    constexpr int NW = THREADS / 64;
    const u32 tid = threadIdx.x;
    auto run_of = [&](u32 e) { u32 k = 0; while (k + 1 < m && s_off[k + 1] <= e) ++k; return k; };
    auto get = [&](u32 i) { E e; e.lo = s_lo[i]; if constexpr (WS) e.hi = s_hi[i]; return e; };
    // first index in [a, b) whose element is not below v (UPPER: is above v)
    auto bound = [&](u32 a, u32 b, const E& v, bool upper) {
        while (a < b) {
            const u32 mid = (a + b) >> 1;
            const E x = get(mid);
            if (upper ? !uni_lt<WS>(v, x) : uni_lt<WS>(x, v)) a = mid + 1; else b = mid;
        }
        return a;
    };
    for (u32 base = 0; base < total; base += THREADS) {  // (whole waves: tally_holders is called by every lane)
        const u32 e = base + tid;
        u32 h = 0;
        if (e < total) {
            const u32 k = run_of(e);
            u32 pos = e - s_off[k];
            bool live = true;
            if constexpr (ROUNDS) live = pos < s_act[k];
            if (live) {
                const E v = get(e);
                bool dup = false;
                h = 1;
                for (u32 kk = 0; kk < m; ++kk) {
                    if (kk == k) continue;
                    const u32 a = s_off[kk], end = s_off[kk + 1], at = bound(a, end, v, kk < k);
                    pos += at - a;
                    if (kk < k) { if (at > a && uni_eq<WS>(get(at - 1), v)) { dup = true; ++h; } }
                    else if (at < end && uni_eq<WS>(get(at), v)) ++h;
                }
                if constexpr (!COUNT) { if (pos < active) s_perm[pos] = e | (!dup && h >= t ? 0x80000000u : 0u); }
                if (dup) h = 0;
            }
        }
        if constexpr (COUNT) tally_holders(h, s_tally);
    }
    u32 kept = 0;
    if constexpr (!COUNT) {
        __syncthreads();
        for (u32 base = 0; base < active; base += THREADS) {
            const u32 q = base + tid;
            const u32 pe = q < active ? s_perm[q] : 0u;
            const bool keep = (pe >> 31) != 0;
            const u32 src = pe & 0x7FFFFFFFu;
            u32 before;
            const u32 tot = count_before<NW>(keep, s_wtot, before);
            const u32 at = written + kept + before;
            if (keep && at < room) {
                dst[at] = s_lo[src];
                if constexpr (WS) dsth[at] = s_hi[src];
            }
            kept += tot;
            __syncthreads();  // s_wtot is rewritten
        }
    }
    return kept;
}
// The short routes: one workgroup per bucket of up to CAP words over all its m holders, whose runs are ascending and duplicate-free by now, staged back to
// back in LDS exactly as k_bucket_setop_many stages them; one round over all of them. COUNT: a workgroup takes the buckets blockIdx.x, + gridDim.x, ...
// of its list and leaves one row of tallies.
template <bool WS, u32 CAP, int THREADS, bool COUNT>
__global__ __launch_bounds__(THREADS) void k_bucket_atleast(const BDesc* __restrict__ list, const u32* __restrict__ list_n, const u32* __restrict__ bucket_prefix,
                                                            const u64* __restrict__ hmask, const ManyOp* __restrict__ ops, const u64* __restrict__ run_start,
                                                            const u32* __restrict__ cap, u64* __restrict__ out_lo, u64* __restrict__ out_hi, u32 SB,
                                                            u32* __restrict__ out_count, u32 t, u64* __restrict__ tally) {
    static_assert(THREADS % 64 == 0, "whole waves");
    constexpr int NW = THREADS / 64;
    __shared__ u64 s_lo[CAP];
    __shared__ u64 s_hi[WS ? CAP : 1];
    __shared__ u32 s_perm[COUNT ? 1 : CAP];  // merged position -> element | kept << 31
    __shared__ u64 s_src[MANY_MAX];           // holder k: first arena slot of its run,
    __shared__ u32 s_opi[MANY_MAX];           // its operand,
    __shared__ u32 s_off[MANY_MAX + 1];       // and where its run starts in s_lo; [m] = words of all holders
    __shared__ u32 s_wtot[NW];
    __shared__ unsigned long long s_tally[COUNT ? MANY_MAX + 1 : 1];
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u64 mask = suffix_mask<WS>(SB);
    const u32 nlist = *list_n;
    if constexpr (COUNT) {
        for (u32 j = tid; j <= MANY_MAX; j += THREADS) s_tally[j] = 0ull;
    }
    for (u32 b = blockIdx.x; b < nlist; b += gridDim.x) {
        __syncthreads();  // the tables of the bucket before are rewritten (and s_tally is cleared)
        const u32 r = list[b].r;
        const u64 holders = hmask[r];
        const u32 p = bucket_prefix[r], m = (u32)__builtin_popcountll(holders);
        if (tid < 64) {
            const bool holds = ((holders >> tid) & 1ull) != 0;
            u32 c = 0;
            u64 st = 0, rank;
            if (holds && dir_lookup(ops[tid].d, p, rank)) { c = ops[tid].d.count[rank]; st = ops[tid].d.start[rank]; }
            u32 inc = c;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) { const u32 up = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += up; }
            if (holds) {
                const u32 k = (u32)__builtin_popcountll(holders & ((1ull << tid) - 1ull));
                s_off[k] = inc - c < CAP ? inc - c : CAP;  // (the list's class says words of all holders <= CAP)
                s_src[k] = st;
                s_opi[k] = tid;
            }
            if (tid == 63) s_off[m] = inc < CAP ? inc : CAP;
        }
        __syncthreads();
        const u32 total = s_off[m];
        for (u32 e = tid; e < total; e += THREADS) {
            u32 k = 0;
            while (k + 1 < m && s_off[k + 1] <= e) ++k;
            const ManyOp& o = ops[s_opi[k]];
            const u64 g = s_src[k] + (e - s_off[k]);
            if constexpr (WS) { s_lo[e] = o.lo[g]; s_hi[e] = o.hi[g] & mask; }
            else s_lo[e] = o.lo[g] & mask;
            if constexpr (!COUNT) s_perm[e] = 0;
        }
        __syncthreads();
        const u64 d0 = COUNT ? 0ull : run_start[r];
        const u32 kept = atleast_round<WS, COUNT, false, THREADS>(s_lo, s_hi, s_perm, s_off, nullptr, m, total, total, t, s_wtot, s_tally, out_lo + d0, WS ? out_hi + d0 : nullptr, 0u,
                                                                  COUNT ? 0u : cap[r]);
        if constexpr (!COUNT) { if (tid == 0) out_count[r] = kept < cap[r] ? kept : cap[r]; }
    }
    if constexpr (COUNT) tally_flush<THREADS>(s_tally, tally);
}
// The long route: a bucket whose holders have more than MANY_LDS words, exact at any length with the LDS of the workgroup route. One workgroup walks the
// holders' ascending, duplicate-free runs where they lie in the operands' arenas, in rounds. A round stages the next MANY_LDS / (runs with words left)
// words of every run. `limit` = the smallest last staged word among the runs that have words beyond their window: every run reaches it, so every copy of a
// value <= limit is staged, and the elements <= limit — the first s_act[k] of window k, found by one search per window — are settled by atleast_round as
// on the short routes; the others are staged again in the next round. With no run beyond its window the round takes everything and is the last. The run
// that sets the limit gives up its whole window, so every round but the last settles MANY_LDS / 64 words or more. Rounds cover ascending ranges of values:
// appended one after the other, the kept elements of the bucket come out ascending, with no table in global memory.
// COUNT: the tallies only; a workgroup takes the buckets blockIdx.x, + gridDim.x, ... of the list.
template <bool WS, bool COUNT>
__global__ __launch_bounds__(256) void k_bucket_atleast_long(const BDesc* __restrict__ list, u32 nlong, const u32* __restrict__ bucket_prefix, const u64* __restrict__ hmask,
                                                             const ManyOp* __restrict__ ops, const u64* __restrict__ run_start, const u32* __restrict__ cap,
                                                             u64* __restrict__ out_lo, u64* __restrict__ out_hi, u32 SB, u32* __restrict__ out_count, u32 t,
                                                             u64* __restrict__ tally) {
    typedef UniE<WS> E;
    constexpr int THREADS = 256, NW = THREADS / 64;
    constexpr u32 CAP = MANY_LDS;
    __shared__ u64 s_lo[CAP];
    __shared__ u64 s_hi[WS ? CAP : 1];
    __shared__ u32 s_perm[COUNT ? 1 : CAP];
    __shared__ const u64* s_plo[MANY_MAX];  // holder k: its run in its operand's arena,
    __shared__ const u64* s_phi[MANY_MAX];
    __shared__ u32 s_cnt[MANY_MAX];         // its length,
    __shared__ u32 s_pos[MANY_MAX];         // how much of it is settled,
    __shared__ u32 s_act[MANY_MAX];         // how much of its window this round settles,
    __shared__ u32 s_off[MANY_MAX + 1];     // and where its window starts in s_lo; [m] = staged words
    __shared__ u32 s_active;                // the sum of s_act
    __shared__ u32 s_wtot[NW];
    __shared__ unsigned long long s_tally[COUNT ? MANY_MAX + 1 : 1];
    const u32 tid = threadIdx.x, lane = tid & 63;
    const u64 mask = suffix_mask<WS>(SB);
    if constexpr (COUNT) {
        for (u32 j = tid; j <= MANY_MAX; j += THREADS) s_tally[j] = 0ull;
    }
    for (u32 q = blockIdx.x; q < nlong; q += gridDim.x) {
        __syncthreads();  // the tables of the bucket before are rewritten (and s_tally is cleared)
        const u32 r = list[q].r;
        const u64 holders = hmask[r];
        const u32 p = bucket_prefix[r], m = (u32)__builtin_popcountll(holders);
        if (tid < 64 && ((holders >> tid) & 1ull)) {
            const u32 k = (u32)__builtin_popcountll(holders & ((1ull << tid) - 1ull));
            u32 c = 0;
            u64 st = 0, rank;
            if (dir_lookup(ops[tid].d, p, rank)) { c = ops[tid].d.count[rank]; st = ops[tid].d.start[rank]; }
            s_cnt[k] = c;
            s_pos[k] = 0;
            s_plo[k] = ops[tid].lo + st;
            s_phi[k] = WS ? ops[tid].hi + st : nullptr;
        }
        const u64 d0 = COUNT ? 0ull : run_start[r];
        const u32 room = COUNT ? 0u : cap[r];
        u32 written = 0;
        for (;;) {
            __syncthreads();  // s_pos is settled; the windows of the round before are rewritten
            if (tid < 64) {   // the windows of this round
                const u32 rem = tid < m ? s_cnt[tid] - s_pos[tid] : 0u;
                const u32 left = (u32)__builtin_popcountll(__ballot(rem != 0));
                const u32 per = left ? CAP / left : 0u;
                const u32 take = rem < per ? rem : per;
                u32 inc = take;
#pragma unroll
                for (int d = 1; d < 64; d <<= 1) { const u32 up = __shfl_up(inc, d, 64); if ((int)lane >= d) inc += up; }
                if (tid < m) s_off[tid] = inc - take;
                if (tid == 63) s_off[m] = inc;
            }
            __syncthreads();
            const u32 total = s_off[m];  // <= CAP
            if (total == 0) break;       // every run is settled
            for (u32 e = tid; e < total; e += THREADS) {
                u32 k = 0;
                while (k + 1 < m && s_off[k + 1] <= e) ++k;
                const u32 i = s_pos[k] + (e - s_off[k]);
                if constexpr (WS) { s_lo[e] = s_plo[k][i]; s_hi[e] = s_phi[k][i] & mask; }
                else s_lo[e] = s_plo[k][i] & mask;
                if constexpr (!COUNT) s_perm[e] = 0;
            }
            __syncthreads();
            if (tid < 64) {  // the limit, and what every window settles
                const u32 a = tid < m ? s_off[tid] : 0u, end = tid < m ? s_off[tid + 1] : 0u;
                bool has = tid < m && end > a && s_pos[tid] + (end - a) < s_cnt[tid];  // words beyond the window
                E x;
                x.lo = has ? s_lo[end - 1] : 0ull;
                if constexpr (WS) x.hi = has ? s_hi[end - 1] : 0ull;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) {
                    E o;
                    o.lo = __shfl_xor(x.lo, d, 64);
                    if constexpr (WS) o.hi = __shfl_xor(x.hi, d, 64);
                    const bool ohas = __shfl_xor((int)has, d, 64) != 0;
                    if (ohas && (!has || uni_lt<WS>(o, x))) { x = o; has = true; }
                }
                u32 act = end - a;
                if (has) {  // the elements of the window that are not above the limit
                    u32 lo = a, hi = end;
                    while (lo < hi) {
                        const u32 mid = (lo + hi) >> 1;
                        E y;
                        y.lo = s_lo[mid];
                        if constexpr (WS) y.hi = s_hi[mid];
                        if (!uni_lt<WS>(x, y)) lo = mid + 1; else hi = mid;
                    }
                    act = lo - a;
                }
                if (tid < m) s_act[tid] = act;
                u32 sum = act;
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
                if (tid == 0) s_active = sum;
            }
            __syncthreads();
            written += atleast_round<WS, COUNT, true, THREADS>(s_lo, s_hi, s_perm, s_off, s_act, m, total, s_active, t, s_wtot, s_tally, out_lo + d0, WS ? out_hi + d0 : nullptr,
                                                               written, room);
            __syncthreads();  // every lane has read s_act and s_pos
            if (tid < m) s_pos[tid] += s_act[tid];
        }
        if constexpr (!COUNT) { if (tid == 0) out_count[r] = written < room ? written : room; }
    }
    if constexpr (COUNT) tally_flush<THREADS>(s_tally, tally);
}
// hist[j] = the sum of column j over the `rows` rows of `tally`, plus the words of the one-holder buckets for j = 1; one workgroup per j (no atomics: exact
// integers, the same on every run)
__global__ __launch_bounds__(256) void k_tally_sum(const u64* __restrict__ tally, u32 rows, const u64* __restrict__ single_total, u64* __restrict__ hist) {
    __shared__ u64 s_w[4];
    const u32 j = blockIdx.x;
    u64 s = 0;
    for (u32 i = threadIdx.x; i < rows; i += 256) s += tally[(u64)i * (MANY_MAX + 1) + j];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) hist[j] = s_w[0] + s_w[1] + s_w[2] + s_w[3] + (j == 1 ? *single_total : 0ull);
}

// ---- `a &= &mut b`, `a -= &mut b`, `a ^= &mut b` (cblx_set_op_assign; src/wordset/set_ops.rs:192-239, 281-317, 366-410 walk the prefixes,
// src/trievec/set_ops.rs:101-129, 163-187, 226-257 the buckets). A bucket both hold keeps a's KIND. A Trie is the ascending result (Trie::remove
// prunes empty nodes, so the trie is a function of its set): k_bucket_setop's output. A Vec is sorted by iter_sorted, takes the ascending words
// only b holds at its end (`^=`: insert_sorted_iter) and loses its deletions through remove_sorted_iter: swap_remove on ascending indices in
// reverse (src/trievec/mod.rs:146-168). With v the Vec remove_sorted_iter scans, n = len(v), D the deleted indices (all inside sorted a),
// m = |D|, L = n - m and dl(p) the number of deleted indices below p, the result r of length L is
//     r[i] = v[i]                       for i < L outside D
//     r[h] = v[s], s = next*(L + dl(h)) for a hole h < L in D, with next(p) = p outside D and L + dl(p) inside D, followed to its fixed point
// (L + dl(p) = n - |{d in D: d >= p}|: where the last word stood when index p was removed). Chains live in [L, n) and can be as long as m, so
// they are settled by pointer doubling (next = next o next until nothing moves), never walked by one lane. (The lists: k_setop_plan<true>.)
template <bool WS> __device__ __forceinline__ UniE<WS> sa_load(const u64* __restrict__ lo, const u64* __restrict__ hi, u32 i, u64 mask) {
    UniE<WS> e;
    if constexpr (WS) { e.lo = lo[i]; e.hi = hi[i] & mask; }
    else e.lo = lo[i] & mask;
    return e;
}
// is x one of the n ascending words of (lo, hi)?
template <bool WS> __device__ __forceinline__ bool sa_member(const u64* __restrict__ lo, const u64* __restrict__ hi, u32 n, u64 mask, const UniE<WS>& x) {
    u32 l = 0, h = n;
    while (l < h) {
        const u32 mid = l + ((h - l) >> 1);
        if (uni_lt<WS>(sa_load<WS>(lo, hi, mid, mask), x)) l = mid + 1; else h = mid;
    }
    return l < n && uni_eq<WS>(sa_load<WS>(lo, hi, l, mask), x);
}
// One workgroup per both-sided bucket whose a side is a Vec; both runs are ascending in their arenas (a's was sorted there, as b's if it is a Vec).
//   1. every word of a is looked up in b by binary search — its index in sorted a is the index remove_sorted_iter finds, so no merge has to carry
//      it: deleted = absent (AND) / present (SUB, XOR); an ordered count of the flags gives dl[0 .. cs], dl[cs] = m;
//   2. XOR: the words of b that a lacks, in order, go to dst[cs ..) — the places insert_sorted_iter pushes them to;
//   3. next[] over the tail [L, cs) of sorted a (beyond cs nothing is deleted: a fixed point), doubled until no entry moves;
//   4. dst[i], i < min(L, cs): a[i] if it stays, else v[next*(L + dl(i))], read from a below cs and from the pushed words (dst itself, at or
//      beyond cs, where step 4 writes nothing) above.
// BIG: dl and the two copies of next[] sit in global memory instead of LDS; the steps are the same.
template <bool WS, u32 OP, bool BIG>
__global__ __launch_bounds__(SA_THREADS) void k_bucket_setop_assign(const BDesc* __restrict__ list, const u32* __restrict__ list_n, const u32* __restrict__ m_cs,
                                                                    const u32* __restrict__ m_co, const u64* __restrict__ m_sstart, const u64* __restrict__ m_ostart,
                                                                    const u64* __restrict__ s_lo, const u64* __restrict__ s_hi, const u64* __restrict__ o_lo,
                                                                    const u64* __restrict__ o_hi, const u64* __restrict__ run_start, u64* out_lo, u64* out_hi, u32 SB,
                                                                    u32* __restrict__ out_count, u8* __restrict__ out_kind, u32* scratch) {
    typedef UniE<WS> E;
    static_assert(OP == SETOP_AND || OP == SETOP_SUB || OP == SETOP_XOR, "`|=` is cblx_merge_assign");
    constexpr int NW = SA_THREADS / 64;
    __shared__ u32 s_dl[BIG ? 1 : SA_LDS + 1];
    __shared__ u32 s_nx[BIG ? 1 : 2 * SA_LDS];
    __shared__ u32 s_wtot[NW];
    if (blockIdx.x >= *list_n) return;
    const BDesc dsc = list[blockIdx.x];
    const u32 r = dsc.r, cs = m_cs[r], co = m_co[r];
    const u64 a_self = m_sstart[r], a_oth = m_ostart[r], d_run = run_start[r];
    const u64* __restrict__ A = s_lo + a_self;
    const u64* __restrict__ B = o_lo + a_oth;
    const u64* __restrict__ Ah = WS ? s_hi + a_self : nullptr;
    const u64* __restrict__ Bh = WS ? o_hi + a_oth : nullptr;
    u64* dst = out_lo + d_run;
    u64* dsth = WS ? out_hi + d_run : nullptr;
    const u64 mask = suffix_mask<WS>(SB);
    const u32 tid = threadIdx.x;
    u32 *dl, *nx0, *nx1;
    if constexpr (BIG) { dl = scratch + dsc.start; nx0 = dl + cs + 1; nx1 = nx0 + cs; }
    else { dl = s_dl; nx0 = s_nx; nx1 = s_nx + SA_LDS; }
    u32 m = 0;
    for (u32 base = 0; base < cs; base += SA_THREADS) {
        const u32 i = base + tid;
        bool del = false;
        if (i < cs) del = sa_member<WS>(B, Bh, co, mask, sa_load<WS>(A, Ah, i, mask)) != (OP == SETOP_AND);
        u32 before;
        const u32 tot = count_before<NW>(del, s_wtot, before);
        __syncthreads();  // s_wtot is rewritten by the next call
        if (i < cs) dl[i] = m + before;
        m += tot;
    }
    if (tid == 0) dl[cs] = m;
    u32 ins = 0;
    if constexpr (OP == SETOP_XOR) {
        for (u32 base = 0; base < co; base += SA_THREADS) {
            const u32 j = base + tid;
            E y = uni_inf<WS>();
            bool push = false;
            if (j < co) { y = sa_load<WS>(B, Bh, j, mask); push = !sa_member<WS>(A, Ah, cs, mask, y); }
            u32 before;
            const u32 tot = count_before<NW>(push, s_wtot, before);
            __syncthreads();  // s_wtot is rewritten by the next call
            if (push) {
                dst[cs + ins + before] = y.lo;
                if constexpr (WS) dsth[cs + ins + before] = y.hi;
            }
            ins += tot;
        }
    }
    const u32 L = cs + ins - m, low = L < cs ? L : cs;
    __syncthreads();
    u32* cur = nx0;
    if (L < cs) {
        const u32 T = cs - L;
        for (u32 q = tid; q < T; q += SA_THREADS) {
            const u32 p = L + q, d0 = dl[p];
            nx0[q] = dl[p + 1] != d0 ? L + d0 : p;
        }
        __syncthreads();
        u32* nxt = nx1;
        for (;;) {
            bool moved = false;
            for (u32 q = tid; q < T; q += SA_THREADS) {
                const u32 v = cur[q], v2 = v < cs ? cur[v - L] : v;
                nxt[q] = v2;
                moved = moved || v2 != v;
            }
            u32* const t = cur; cur = nxt; nxt = t;
            if (!__syncthreads_or(moved)) break;
        }
    }
    for (u32 i = tid; i < low; i += SA_THREADS) {
        const u32 d0 = dl[i];
        u32 s = i;
        if (dl[i + 1] != d0) { s = L + d0; if (s < cs) s = cur[s - L]; }
        E e;
        if (s < cs) e = sa_load<WS>(A, Ah, s, mask);
        else { e.lo = dst[s]; if constexpr (WS) e.hi = dsth[s]; }
        dst[i] = e.lo;
        if constexpr (WS) dsth[i] = e.hi;
    }
    if (tid == 0) { out_count[r] = L; out_kind[r] = KIND_VEC; }
}

// ---- |a AND b| alone (cblx_intersection_count): one u32 per bucket both hold, nothing else is written and nothing is sorted ----
// To intersect two duplicate-free lists neither has to be ascending: the shorter (STAGED) side goes into LDS as stored, masked to the suffix, under an
// open-addressing table of u32 entries — index + 1, 0 = empty, twice as many slots as the side may have words, filled by atomicCAS on a mixed hash of the
// suffix with linear probing — and every word of the other (PROBE) side is looked up: the hits are the intersection. The table holds INDICES, so no suffix
// value is set apart as "empty": SUFFIX_BITS = 64 has no spare bit and the all-ones suffix is legal. No kind is consulted; common_route (common_route.hpp)
// picks the kernel by the two lengths, and by the kinds only where two Tries longer than a table can be merged instead.
// The lists of a route are walked by a grid-stride loop over *list_n, so the host launches all four kernels before it has read a single list length.
static const u32 COMMON_WAVE_CAP = COMMON_SMALL / 2;  // the staged side of a bucket of the wave route
static const int COMMON_THREADS = 256;
// murmur3's 64-bit finaliser over lo ^ hi * phi: consecutive suffixes, multiples of a power of two and values that differ in their top bits alone all spread
__device__ __forceinline__ u32 common_hash(u64 lo, u64 hi) {
    u64 x = lo ^ (hi * 0x9E3779B97F4A7C15ull);
    x ^= x >> 33; x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33; x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return (u32)x;
}
// The staged words and their table; the LDS arrays belong to the kernel (CAP words, CAP high halves when wide, 2 * CAP entries).
template <bool WS, u32 CAP> struct CommonTable {
    static_assert((CAP & (CAP - 1)) == 0, "the table indexes by hash mod 2 CAP");
    static constexpr u32 SLOTS = 2 * CAP, M = SLOTS - 1;
    u64 *s_lo, *s_hi;
    u32* s_tab;
    // n <= CAP words from (lo, hi), by all THREADS threads of the workgroup; the table can be probed when it returns. The caller synchronises
    // before it fills again.
    template <int THREADS> __device__ __forceinline__ void fill(const u64* __restrict__ lo, const u64* __restrict__ hi, u32 n, u64 mask) const {
        for (u32 i = threadIdx.x; i < SLOTS; i += THREADS) s_tab[i] = 0u;
        for (u32 i = threadIdx.x; i < n; i += THREADS) {
            if constexpr (WS) { s_lo[i] = lo[i]; s_hi[i] = hi[i] & mask; }
            else s_lo[i] = lo[i] & mask;
        }
        __syncthreads();
        for (u32 i = threadIdx.x; i < n; i += THREADS) {
            u32 h = common_hash(s_lo[i], WS ? s_hi[i] : 0ull) & M;
            while (atomicCAS(&s_tab[h], 0u, i + 1u) != 0u) h = (h + 1u) & M;  // (n <= CAP < SLOTS: a free slot exists)
        }
        __syncthreads();
    }
    // is the masked suffix (lo, hi) one of the staged words? (an empty slot ends every probe sequence: the table is never more than half full)
    __device__ __forceinline__ bool holds(u64 lo, u64 hi) const {
        u32 h = common_hash(lo, WS ? hi : 0ull) & M;
        for (;;) {
            const u32 e = s_tab[h];
            if (e == 0u) return false;
            if (s_lo[e - 1u] == lo && (!WS || s_hi[e - 1u] == hi)) return true;
            h = (h + 1u) & M;
        }
    }
};
// one thread per candidate (every candidate of a.bv & b.bv is held by both): b's count, and the bucket joins the list of its route
__global__ __launch_bounds__(CLASSIFY_THREADS) void k_common_plan(u64 nb, const u32* __restrict__ raw_cnt, const u32* __restrict__ m_cs, u32* __restrict__ m_co,
                                                                   const u8* __restrict__ m_skind, const u8* __restrict__ m_okind,
                                                                   BDesc* __restrict__ lists /* [COMMON_ROUTES][nb] */, u32* __restrict__ list_n) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    int cls = -1;
    if (r < nb) {
        const u32 cs = m_cs[r], co = raw_cnt[r] - cs;
        m_co[r] = co;
        if (cs != 0 && co != 0) cls = common_route(cs, co, m_skind[r] == KIND_TRIE, m_okind[r] == KIND_TRIE);
    }
    const u32 slot = block_append<CLASSIFY_THREADS, COMMON_ROUTES>(cls, list_n);
    if (cls >= 0) lists[(u64)cls * nb + slot] = BDesc{0, 0, (u32)r};
}
// what the four kernels are given: the route's list, the tables of k_merge_table / k_common_plan, the two arenas, the counters
struct CommonArgs {
    const BDesc* list; const u32* list_n;
    const u32 *cs, *co;
    const u64 *sstart, *ostart;
    const u64 *a_lo, *a_hi, *b_lo, *b_hi;
    u32 SB;
    u32* common;
};
// the sum of a workgroup's per-thread counts, valid in thread 0; `s_w`: one word per wave, the caller synchronises before it is used again
template <int NW> __device__ __forceinline__ u32 common_block_sum(u32 v, u32* s_w) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_down(v, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    u32 tot = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) tot += s_w[w];
    return tot;
}
// Route 1, ca + cb <= COMMON_SMALL: one wave per bucket (a workgroup IS one wave, so its barriers are wave-level: no other wave waits at them). The
// staged side is at most 128 words; the probe side is read 64 words per step, coalesced, the hits counted by ballot.
template <bool WS>
__global__ __launch_bounds__(64) void k_common_wave(const CommonArgs g) {
    __shared__ u64 s_lo[COMMON_WAVE_CAP];
    __shared__ u64 s_hi[WS ? COMMON_WAVE_CAP : 1];
    __shared__ u32 s_tab[2 * COMMON_WAVE_CAP];
    const CommonTable<WS, COMMON_WAVE_CAP> t{s_lo, s_hi, s_tab};
    const u64 mask = suffix_mask<WS>(g.SB);
    const u32 lane = threadIdx.x, n = *g.list_n;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        const u32 r = g.list[i].r, ca = g.cs[r], cb = g.co[r];
        const bool sa = common_stage_a(ca, cb);
        const u64 s0 = sa ? g.sstart[r] : g.ostart[r], p0 = sa ? g.ostart[r] : g.sstart[r];
        const u64* __restrict__ S = (sa ? g.a_lo : g.b_lo) + s0;
        const u64* __restrict__ Sh = WS ? (sa ? g.a_hi : g.b_hi) + s0 : nullptr;
        const u64* __restrict__ Q = (sa ? g.b_lo : g.a_lo) + p0;
        const u64* __restrict__ Qh = WS ? (sa ? g.b_hi : g.a_hi) + p0 : nullptr;
        const u32 ns0 = sa ? ca : cb, ns = ns0 < COMMON_WAVE_CAP ? ns0 : COMMON_WAVE_CAP, np = sa ? cb : ca;  // (the route says ns0 <= the table's capacity)
        t.template fill<64>(S, Sh, ns, mask);
        u32 hits = 0;
        for (u32 j0 = 0; j0 < np; j0 += 64) {
            const u32 j = j0 + lane;
            bool hit = false;
            if (j < np) hit = WS ? t.holds(Q[j], Qh[j] & mask) : t.holds(Q[j] & mask, 0ull);
            hits += (u32)__builtin_popcountll(__ballot(hit));
        }
        if (lane == 0) g.common[r] = hits;
        __syncthreads();  // the table is rewritten
    }
}
// Routes 2 and 4: 256 threads per bucket. The staged side goes through the table in slices of COMMON_LDS words — ONE slice on route 2, whose staged side is
// that short — and the probe side, of any length, is streamed from HBM once per slice, two words per 16-byte load where the run starts on a 16-byte
// boundary (one word in front of the pairs where it does not). LDS: 16 KB, 24 KB wide.
template <bool WS, bool SLICED>
__device__ __forceinline__ void common_lds_run(const CommonArgs& g) {
    constexpr int NW = COMMON_THREADS / 64;
    __shared__ u64 s_lo[COMMON_LDS];
    __shared__ u64 s_hi[WS ? COMMON_LDS : 1];
    __shared__ u32 s_tab[2 * COMMON_LDS];
    __shared__ u32 s_w[NW];
    const CommonTable<WS, COMMON_LDS> t{s_lo, s_hi, s_tab};
    const u64 mask = suffix_mask<WS>(g.SB);
    const u32 tid = threadIdx.x, n = *g.list_n;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        const u32 r = g.list[i].r, ca = g.cs[r], cb = g.co[r];
        const bool sa = common_stage_a(ca, cb);
        const u64 s0 = sa ? g.sstart[r] : g.ostart[r], p0 = sa ? g.ostart[r] : g.sstart[r];
        const u64* __restrict__ S = (sa ? g.a_lo : g.b_lo) + s0;
        const u64* __restrict__ Sh = WS ? (sa ? g.a_hi : g.b_hi) + s0 : nullptr;
        const u64* __restrict__ Q = (sa ? g.b_lo : g.a_lo) + p0;
        const u64* __restrict__ Qh = WS ? (sa ? g.b_hi : g.a_hi) + p0 : nullptr;
        const u32 ns0 = sa ? ca : cb, ns = SLICED || ns0 < COMMON_LDS ? ns0 : COMMON_LDS, np = sa ? cb : ca;  // (route 2 says ns0 <= COMMON_LDS)
        // the probe run as [head words one by one][pairs][tail words one by one]
        const bool odd = ((uintptr_t)Q & 8u) != 0;
        const bool paired = !WS || (((uintptr_t)Qh & 8u) != 0) == odd;  // (both halves start on the same side of a 16-byte boundary: always, with the pool's arenas)
        const u32 head = !paired ? np : (odd && np ? 1u : 0u), npair = (np - head) >> 1, tail = head + 2u * npair;
        const ulonglong2* __restrict__ Q2 = (const ulonglong2*)(Q + head);
        const ulonglong2* __restrict__ Q2h = WS ? (const ulonglong2*)(Qh + head) : nullptr;
        auto one = [&](u32 j) { return (WS ? t.holds(Q[j], Qh[j] & mask) : t.holds(Q[j] & mask, 0ull)) ? 1u : 0u; };
        u32 hits = 0;
        for (u32 sl = 0; sl < ns; sl += COMMON_LDS) {
            const u32 n1 = ns - sl < COMMON_LDS ? ns - sl : COMMON_LDS;
            t.template fill<COMMON_THREADS>(S + sl, WS ? Sh + sl : nullptr, n1, mask);
            for (u32 j = tid; j < head; j += COMMON_THREADS) hits += one(j);
            for (u32 q = tid; q < npair; q += COMMON_THREADS) {
                const ulonglong2 v = Q2[q];
                if constexpr (WS) {
                    const ulonglong2 vh = Q2h[q];
                    hits += (t.holds(v.x, vh.x & mask) ? 1u : 0u) + (t.holds(v.y, vh.y & mask) ? 1u : 0u);
                } else hits += (t.holds(v.x & mask, 0ull) ? 1u : 0u) + (t.holds(v.y & mask, 0ull) ? 1u : 0u);
            }
            for (u32 j = tail + tid; j < np; j += COMMON_THREADS) hits += one(j);
            __syncthreads();  // the table is rewritten
        }
        const u32 tot = common_block_sum<NW>(hits, s_w);
        if (tid == 0) g.common[r] = tot;
    }
}
template <bool WS>
__global__ __launch_bounds__(COMMON_THREADS) void k_common_lds(const CommonArgs g) { common_lds_run<WS, false>(g); }
// Route 4: both sides are longer than COMMON_LDS words and at least one of them is a Vec — only set operations and `|=` leave such Vecs behind. QUADRATIC BY
// DESIGN: ceil(staged / COMMON_LDS) passes over the probe side. It is rare, it is correct at any length, and it keeps the operands unsorted; sorting the Vec
// in its arena, which is what makes `&` linear here, is exactly what a comparison must not do.
template <bool WS>
__global__ __launch_bounds__(COMMON_THREADS) void k_common_sliced(const CommonArgs g) { common_lds_run<WS, true>(g); }
// Route 3, two Tries of any length: UniRounds as k_bucket_union drives it, with AND's predicate — an output that equals its predecessor is b's copy of a word a
// holds — counted in a register instead of compacted; nothing is written back to the rings. The outputs stay in the registers that merged them: a thread
// compares its own four in place and gets the predecessor of its first from its neighbour through one LDS word per thread. Across a round edge only the VALUE
// of the last output is carried (UniRounds::carry): its pair partner can only be the first output of the next round.
template <bool WS>
__global__ __launch_bounds__(UNI_THREADS) void k_common_merge(const CommonArgs g) {
    typedef UniE<WS> E;
    typedef UniRounds<WS> R;
    constexpr int NW = R::NW;
    __shared__ u64 s_in[R::SLOTS];
    __shared__ u64 s_inh[WS ? R::SLOTS : 1];
    __shared__ u32 s_split[NW + 1];
    __shared__ u64 s_edge[UNI_THREADS + 1];  // [t]: thread t's last output; [UNI_THREADS]: the round's last output
    __shared__ u64 s_edgeh[WS ? UNI_THREADS + 1 : 1];
    __shared__ u32 s_w[NW];
    const u64 mask = suffix_mask<WS>(g.SB);
    const u32 tid = threadIdx.x, n = *g.list_n;
    for (u32 i = blockIdx.x; i < n; i += gridDim.x) {
        const u32 r = g.list[i].r;
        const u64 a0 = g.sstart[r], b0 = g.ostart[r];
        R m{s_in, s_inh, s_split, g.a_lo + a0, g.b_lo + b0, WS ? g.a_hi + a0 : nullptr, WS ? g.b_hi + b0 : nullptr, mask, g.cs[r], g.co[r]};
        u32 cnt = 0;
        while (m.more()) {
            m.stage();
            m.split();
            E a[UNI_ITEMS], o[UNI_ITEMS];
            m.merge(a, o);
            const u32 q0 = tid * UNI_ITEMS, nout = m.nout;
            s_edge[tid] = o[UNI_ITEMS - 1].lo;
            if constexpr (WS) s_edgeh[tid] = o[UNI_ITEMS - 1].hi;
#pragma unroll
            for (int k = 0; k < UNI_ITEMS; ++k)
                if (q0 + k + 1 == nout) {
                    s_edge[UNI_THREADS] = o[k].lo;
                    if constexpr (WS) s_edgeh[UNI_THREADS] = o[k].hi;
                }
            __syncthreads();
            E pred = m.carry, last;
            bool have = m.have_carry;
            if (tid) {  // (thread tid - 1's outputs all lie below nout wherever this thread's first one does)
                pred.lo = s_edge[tid - 1];
                if constexpr (WS) pred.hi = s_edgeh[tid - 1];
                have = true;
            }
#pragma unroll
            for (int k = 0; k < UNI_ITEMS; ++k) {
                cnt += (q0 + k < nout && have && uni_eq<WS>(o[k], pred)) ? 1u : 0u;
                pred = o[k];
                have = true;
            }
            last.lo = s_edge[UNI_THREADS];
            if constexpr (WS) last.hi = s_edgeh[UNI_THREADS];
            m.advance(0, last);
        }
        const u32 tot = common_block_sum<NW>(cnt, s_w);
        if (tid == 0) g.common[r] = tot;
        __syncthreads();  // s_w and the rings are rewritten
    }
}
// The sum of n counters, one u64 per workgroup (no atomics: the order of an integer sum does not matter, and the result is the same on every run). Run twice:
// over the buckets into up to COMMON_SUM_GROUPS partial sums, then over those by one workgroup.
static const u32 COMMON_SUM_GROUPS = 1024;
template <typename T>
__global__ __launch_bounds__(256) void k_common_sum(const T* __restrict__ v, u64 n, u64* __restrict__ out) {
    __shared__ u64 s_w[4];
    u64 s = 0;
    for (u64 i = (u64)blockIdx.x * 256 + threadIdx.x; i < n; i += (u64)gridDim.x * 256) s += v[i];
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

}  // namespace cblx
