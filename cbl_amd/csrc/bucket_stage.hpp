// bucket_stage.hpp — the driver of the per-bucket kernels (KRN-3) over the runs of a directory: the length classes of the one-workgroup kernels and the
// one launcher of their run sorts (sort_rule, launch_run_sort), the long-run paths (big_stage on a twin buffer, huge_stage, long_runs_stage, finish_twin)
// and bucket_stage itself. pipeline.hpp runs it behind the partition, setops.hpp's merge_direct builds on its parts. Kernels: kernels_bucket.hpp.
// Included by cblx.cpp only.
#pragma once
#include "ctx.hpp"

namespace {

// general kernel for runs of any length (and the fallback of the big path): one workgroup per run, LSD radix in global scratch
template <typename C> void huge_stage(cblx_ctx* c, const BDesc* d_list, const u32* d_list_n, u32 nh, u64* a_lo, typename C::HiT* a_hi, Resident& nr, const MergeArgs& ma) {
    typedef typename C::HiT HiT;
    if (nh == 0) return;
    StageTimer t(c, ST_BHUGE);
    std::vector<BDesc> hl = d2h_vec<BDesc>(c, d_list, nh);
    std::vector<u64> so(nh);
    u64 tot = 0;
    for (u32 i = 0; i < nh; ++i) { so[i] = tot; tot += hl[i].c & ~BDESC_TRIE; }
    Buf<u64> d_so(c->pool, nh), s_alo(c->pool, tot), s_blo(c->pool, tot), s_ahi(c->pool, C::WS ? tot : 1), s_bhi(c->pool, C::WS ? tot : 1);
    Buf<u32> s_aidx(c->pool, tot), s_bidx(c->pool, tot);
    h2d(c, d_so.get(), so.data(), nh);
    hipLaunchKernelGGL((k_bucket_huge<C::WS, HiT>), dim3(nh), dim3(256), 0, c->stream, d_list, d_list_n, d_so.get(), a_lo, a_hi, c->P.SB, s_alo.get(), s_ahi.get(),
                       s_aidx.get(), s_blo.get(), s_bhi.get(), s_bidx.get(), nr.cnt.get(), nr.kind.get(), ma);
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));
}
// lanes per bucket of the per-bucket copy kernels, from the average run length (words / buckets)
template <typename F> void with_lpb(u64 words, u64 buckets, F&& f) {
    const u64 avg = buckets ? words / buckets : 0;
    if (avg >= 48) f(std::integral_constant<int, 64>());
    else if (avg >= 12) f(std::integral_constant<int, 16>());
    else f(std::integral_constant<int, 4>());
}
inline dim3 lpb_grid(u64 buckets, int lpb) { return dim3((unsigned)std::max<u64>(1, ceil_div(buckets * (u64)lpb, 256))); }

// The length classes of the one-workgroup bucket kernels (k_bucket_msd, k_bucket_sorted, k_bucket_claim): a run of up to `cap` words takes a workgroup of
// `threads` — cap / 8 per lane, the two shortest on one wave of two / four slots per lane (kernels_bucket.hpp: CLS_M32).
struct LenClass { int cls, threads, cap; };
constexpr int N_LEN_CLASSES = 6;
constexpr LenClass LEN_CLASSES[N_LEN_CLASSES] = {{CLS_M16, 64, 128}, {CLS_M32, 64, 256}, {CLS_M64, 64, 512}, {CLS_M128, 128, 1024}, {CLS_M256, 256, 2048}, {CLS_M512, 512, 4096}};
constexpr int len_class_of(u32 cap) {  // entry of that capacity
    for (int k = 0; k < N_LEN_CLASSES; ++k) if ((u32)LEN_CLASSES[k].cap == cap) return k;
    return -1;
}
// Entry K as an argument: in f(len_class<K>) the entry LEN_CLASSES[decltype(k)::value] is a constant expression. each_len_class visits all in order.
template <int K> constexpr std::integral_constant<int, K> len_class{};
template <int K = 0, typename F> void each_len_class(const F& f) {
    if constexpr (K < N_LEN_CLASSES) { f(len_class<K>); each_len_class<K + 1>(f); }
}
// ---- the run sorts of one workgroup: the walk kernel (k_bucket_sorted) or the counting sort (k_bucket_msd), chosen and launched in one place ----------
// where a sort kernel reports the runs it gives up on: the `retry` list (counter retry_n), or a mark on their list entry in `bail` and the word `bail_any`
struct SortOut { BDesc* retry = nullptr; u32* retry_n = nullptr; u8* bail = nullptr; u32* bail_any = nullptr; };
// what the caller wants: a build's first kernel (runs that stay Vecs need no order) | the sorted list | `self |= other` of both-sided buckets (merge_direct)
enum SortMode { SORT_BUILD, SORT_SORTED, SORT_MERGE };
struct SortRule { bool walk, merge; };  // the walk kernel runs (else the counting sort); the MERGE argument of the one that runs
// Elements that carry their stream index — PACKED narrow suffixes (`pk`), wide ones (`ws`) — take the walk kernel (round 6); in a build only the runs of more
// than VEC_THRESHOLD words, which end up sorted (or give up: repeats). Unpacked narrow suffixes take the counting sort. Asked for the sorted list of up to 1024
// words (big_stage: sub-ranges on the 128-thread workgroup) that is its `self |= other` instantiation without merge arguments: that one keeps the top-bit
// sub-bucket limit (the build's 1024-word class assumes hashed sub-buckets).
constexpr SortRule sort_rule(SortMode m, bool pk, bool ws, int cap) {
    const bool walk = (pk || ws) && (m != SORT_BUILD || cap > (int)VEC_THRESHOLD);
    return {walk, m == SORT_MERGE || (m == SORT_SORTED && !walk && cap <= 1024)};
}
// The rule as the five launch sites spelled it before they shared it, {walk, MERGE} for packed narrow | unpacked narrow (SB = 64) | wide suffixes at a capacity
constexpr bool operator==(SortRule a, SortRule b) { return a.walk == b.walk && a.merge == b.merge; }
constexpr bool rule_is(SortMode m, int cap, SortRule packed, SortRule unpacked, SortRule wide) {
    return sort_rule(m, true, false, cap) == packed && sort_rule(m, false, false, cap) == unpacked && sort_rule(m, false, true, cap) == wide;
}
static_assert(rule_is(SORT_BUILD, 128, {0, 0}, {0, 0}, {0, 0}) && rule_is(SORT_BUILD, 1024, {0, 0}, {0, 0}, {0, 0}) && rule_is(SORT_BUILD, 2048, {1, 0}, {0, 0}, {1, 0}) &&
              rule_is(SORT_BUILD, 4096, {1, 0}, {0, 0}, {1, 0}), "bucket_stage, a class's first kernel: the walk kernel iff (PK || WS) && CAP > VEC_THRESHOLD, MERGE = false");
static_assert(rule_is(SORT_SORTED, 4096, {1, 0}, {0, 0}, {1, 0}), "bucket_stage, behind the claim tables (512 / 4096): the walk kernel iff PK || WS, MERGE = false");
static_assert(rule_is(SORT_SORTED, 2048, {1, 0}, {0, 0}, {1, 0}), "bucket_stage, behind the long runs' pre-pass (256 / 2048; narrow only, wide never gets there): the walk kernel iff PK");
static_assert(rule_is(SORT_SORTED, BIG_SUB, {1, 0}, {0, 1}, {1, 0}) && rule_is(SORT_SORTED, BIG_VCAP, {1, 0}, {0, 0}, {1, 0}),
              "big_stage, sub-ranges (BIG_SUB = 1024, BIG_VCAP = 2048): the walk kernel iff PK || WS with MERGE = false, else the counting sort with MERGE = (CAP <= 1024)");
static_assert(rule_is(SORT_MERGE, 128, {1, 1}, {0, 1}, {1, 1}) && rule_is(SORT_MERGE, 4096, {1, 1}, {0, 1}, {1, 1}), "merge_direct: the walk kernel iff PK || WS, MERGE = true for both kernels");
// The one launch of a run sort, the only place that knows the two kernels' argument orders: `n` runs of length class K from `list` (counter list_n) in lo / hi
template <typename C, SortMode M, bool PK, int K>
void launch_run_sort(cblx_ctx* c, std::integral_constant<int, K>, const BDesc* list, const u32* list_n, u32 n, u64* lo, typename C::HiT* hi, u32* cnt, u8* kind, const SortOut& o,
                     const MergeArgs& ma = MergeArgs{}) {
    typedef typename C::HiT HiT;
    constexpr int T = LEN_CLASSES[K].threads, CAP = LEN_CLASSES[K].cap;
    constexpr SortRule R = sort_rule(M, PK, C::WS, CAP);
    if constexpr (R.walk)
        hipLaunchKernelGGL((k_bucket_sorted<T, CAP, C::WS, HiT, R.merge>), dim3(n), dim3(T), 0, c->stream, list, list_n, lo, hi, c->P.SB, cnt, kind, o.retry, o.retry_n, o.bail, o.bail_any, ma);
    else
        hipLaunchKernelGGL((k_bucket_msd<T, CAP, PK, C::WS, HiT, R.merge>), dim3(n), dim3(T), 0, c->stream, list, list_n, lo, hi, c->P.SB, cnt, kind, o.retry, o.retry_n, ma, o.bail, o.bail_any);
}
// f(std::true_type) where the elements are PACKED (kernels_bucket.hpp: a narrow suffix that leaves PK_BITS of a u64 to the stream index), else f(std::false_type)
template <typename C, typename F> void with_packed(const Consts& P, F&& f) {
    if constexpr (!C::WS) { if (P.SB + PK_BITS <= 64) return f(std::true_type()); }
    f(std::false_type());
}
// suffixes too wide for the counting-sort kernel's 16-byte elements (!msd_takes — SUFFIX_BITS > 116: K >= 57 with a handful of prefix bits): every counting-sort
// class of the class lists takes the LDS radix kernel, on the runs in nr's arena
template <typename C> void radix_only_classes(cblx_ctx* c, const BDesc* lists, const u32* list_n, const std::vector<u32>& ln, u64 nb, Resident& nr, const MergeArgs& ma) {
    typedef typename C::HiT HiT;
    for (const LenClass& lc : LEN_CLASSES)
        if (ln[lc.cls])
            hipLaunchKernelGGL((k_bucket_medium<512, C::WS, HiT>), dim3(ln[lc.cls]), dim3(512), 0, c->stream, lists + (size_t)lc.cls * nb, list_n + lc.cls, nr.a_lo.get(),
                               C::WS ? (HiT*)nr.a_hi.get() : (HiT*)nullptr, c->P.SB, nr.cnt.get(), nr.kind.get(), ma);
}
// nr.count = the words of all buckets
inline void count_words(cblx_ctx* c, Resident& nr) {
    Buf<u64> total(c->pool, 1);
    CBLX_HIP(hipMemsetAsync(total.get(), 0, 8, c->stream));
    hipLaunchKernelGGL(k_sum_u32, dim3((unsigned)std::min<u64>(2048, std::max<u64>(1, ceil_div(nr.nb, 256)))), dim3(256), 0, c->stream, nr.cnt.get(), nr.nb, total.get());
    nr.count = d2h<u64>(c, total.get());
}

__global__ void k_sum_bdesc_len(const BDesc* __restrict__ list, u32 n, u64* __restrict__ out) {
    u64 s = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += list[i].c & ~BDESC_TRIE;
    s = wave_reduce_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)out, (unsigned long long)s);
}
// (profiling) sum of the final counts of the buckets of a list
__global__ void k_sum_list_counts(const BDesc* __restrict__ list, u32 n, const u32* __restrict__ cnt, u64* __restrict__ out) {
    u64 s = 0;
    for (u32 i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) s += cnt[list[i].r];
    s = wave_reduce_sum(s);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd((unsigned long long*)out, (unsigned long long)s);
}
// runs of 4097 .. BIG_MAX words (kernels_bucket.hpp: k_big_*): one more partition pass on the top suffix bits with the runs as
// segments, out of the arena into a twin buffer at the same positions; sub-ranges sorted + deduplicated in place there by
// k_bucket_msd; what cannot be finished that way takes the general kernel on the (untouched) arena run. The finished runs stay
// in the twin: finish_twin decides which buffer becomes the arena.
struct Twin {
    Buf<u64> lo, hi;   // same positions as the arena; hi only for suffixes wider than 64 bits
    Buf<u8> in_twin;   // per bucket rank: 1 = its final words are in the twin
    u64 arrivals = 0;  // words of the runs that went through the twin
    u64 runs = 0;      // ... and their number
    bool used() const { return lo.get() != nullptr; }
};
__global__ void k_set_u32(u32* p, u32 v) { *p = v; }
template <typename C> void big_stage(cblx_ctx* c, const BDesc* d_list, const u32* d_list_n, u32 nbig, Resident& nr, const MergeArgs& ma, Twin& tw) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    typedef typename std::conditional<WS, u64, NoHi>::type AH;  // hi part of an arena element as the partition kernels see it
    if (nbig == 0) return;
    const Consts& P = c->P;
    u64* a_lo = nr.a_lo.get();
    HiT* a_hi = WS ? (HiT*)nr.a_hi.get() : (HiT*)nullptr;
    if (!tw.used()) {
        const u64 T = d2h<u64>(c, nr.start.get() + nr.nb);  // every run position lies below the total arrival count
        try {
            tw.lo = Buf<u64>(c->pool, T + 2);
            if (WS) tw.hi = Buf<u64>(c->pool, T + 2);
            tw.in_twin = Buf<u8>(c->pool, nr.nb + 1);
        } catch (const Error& e) {
            // no room for a second arena (an index that fills most of the HBM): the long runs take the general kernel, whose
            // scratch is only as large as the runs themselves
            if (e.code != CBLX_ENOMEM) throw;
            tw = Twin();
            huge_stage<C>(c, d_list, d_list_n, nbig, a_lo, a_hi, nr, ma);
            return;
        }
        CBLX_HIP(hipMemsetAsync(tw.in_twin.get(), 0, nr.nb + 1, c->stream));
    }
    Buf<BDesc> fb(c->pool, nbig);
    Buf<u32> fb_n(c->pool, 1);
    {
        StageTimer t(c, ST_BBIG);
        Buf<u32> ntile(c->pool, nbig), nv(c->pool, nbig), tile_first(c->pool, nbig + 1);
        Buf<u64> vb(c->pool, nbig + 1), run_start(c->pool, nbig);
        hipLaunchKernelGGL(k_big_plan, grid1(nbig, 256), dim3(256), 0, c->stream, d_list, nbig, P.SB, ntile.get(), nv.get());
        const u64 nt64 = exclusive_scan<u32>(c, ntile.get(), nbig, tile_first.get());
        const u64 vtot = exclusive_scan<u64>(c, nv.get(), nbig, vb.get());
        if (nt64 >= 0xFFFFFF00ull / 256) throw Error(CBLX_ERANGE, "too many tiles in the long runs of one batch");
        const u32 nt = (u32)nt64;
        hipLaunchKernelGGL(k_set_u32, dim3(1), dim3(1), 0, c->stream, tile_first.get() + nbig, nt);
        Buf<u64> t_start(c->pool, nt);
        Buf<u32> t_count(c->pool, nt), t_seg(c->pool, nt), counts(c->pool, (size_t)256 * nt), colpre(c->pool, (size_t)256 * nt), scratch, coltot(c->pool, 256),
            adj(c->pool, (size_t)256 * nbig), rel(c->pool, (size_t)256 * nbig);
        hipLaunchKernelGGL(k_big_tile_table, grid1(std::max<u64>(nt, nbig), 256), dim3(256), 0, c->stream, d_list, nbig, tile_first.get(), t_start.get(), t_count.get(), t_seg.get(),
                           run_start.get());
        TileView tv{nullptr, t_count.get(), nullptr, nullptr, nt, 0};
        tv.start64 = t_start.get();
        tv.seg32 = t_seg.get();
        const u32 DB = big_digit_bits(P.SB);
        const DigitBits dfn{P.SB - DB, DB};
        const AH* in_hi = (const AH*)a_hi;
        AH* out_hi = (AH*)tw.hi.get();
        hipLaunchKernelGGL((k_radix_hist<AH, DigitBits>), dim3(xcd_grid(nt)), dim3(RDX_THREADS), 0, c->stream, (const u64*)a_lo, in_hi, tv, dfn, counts.get());
        colscan(c, counts.get(), nullptr, nt, colpre.get(), coltot.get(), scratch);
        hipLaunchKernelGGL(k_seg_adjust, dim3(nbig), dim3(256), 0, c->stream, colpre.get(), coltot.get(), (const u32*)tile_first.get(), (const u32*)nullptr, (const u32*)nullptr, nt, nbig,
                           adj.get(), rel.get());
        hipLaunchKernelGGL((k_radix_scatter<AH, AH, DigitBits>), dim3(xcd_grid(nt)), dim3(RDX_THREADS), 0, c->stream, (const u64*)a_lo, in_hi, tv, dfn, (const u32*)colpre.get(),
                           (const u32*)adj.get(), tw.lo.get(), out_hi, DigitBits{0, 0}, (u8*)nullptr, (u32*)nullptr, 0u, 0u, 0u, (u32*)nullptr, 0u,
                           OwnWindow{0, 0, nullptr, nullptr, nullptr}, (const u64*)run_start.get());
        Buf<BDesc> vlist(c->pool, vtot), cls_lists(c->pool, 2 * vtot);
        Buf<u32> v_count(c->pool, vtot + 1), cls_n(c->pool, 2);
        Buf<u8> v_kind(c->pool, vtot + 1);
        Buf<BDesc> retry(c->pool, vtot);  // sub-ranges the sort gives up on (crowded sub-bucket): their runs fall back as a whole
        Buf<u32> retry_n(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(retry_n.get(), 0, 4, c->stream));
        CBLX_HIP(hipMemsetAsync(cls_n.get(), 0, 8, c->stream));
        CBLX_HIP(hipMemsetAsync(fb_n.get(), 0, 4, c->stream));
        hipLaunchKernelGGL(k_big_vlist, dim3((nbig + BIG_VLIST_RUNS - 1) / BIG_VLIST_RUNS), dim3(256), 0, c->stream, d_list, nbig, vb.get(), rel.get(), P.SB, vlist.get(), v_count.get(), cls_lists.get(), cls_n.get(), vtot);
        const std::vector<u32> cn = d2h_vec<u32>(c, cls_n.get(), 2);
        HiT* th = WS ? (HiT*)tw.hi.get() : (HiT*)nullptr;
        // sub-ranges are always asked for the sorted list (sort_rule: those of up to 1024 words take the 128-thread workgroup)
        with_packed<C>(P, [&](auto pk) {
            auto sub = [&](auto kc, u32 i) {  // list i of the sub-ranges, by the kernel of length class kc
                if (cn[i])
                    launch_run_sort<C, SORT_SORTED, decltype(pk)::value>(c, kc, cls_lists.get() + (size_t)i * vtot, cls_n.get() + i, cn[i], tw.lo.get(), th, v_count.get(), v_kind.get(),
                                                                         SortOut{retry.get(), retry_n.get()});
            };
            sub(len_class<len_class_of(BIG_SUB)>, 0);
            sub(len_class<len_class_of(BIG_VCAP)>, 1);
        });
        hipLaunchKernelGGL((k_big_finish<WS>), dim3(nbig), dim3(256), 0, c->stream, d_list, d_list_n, vb.get(), vlist.get(), v_count.get(), P.SB, tw.lo.get(), tw.hi.get(), nr.cnt.get(),
                           nr.kind.get(), tw.in_twin.get(), fb.get(), fb_n.get());
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the pass tables die here
    }
    {   // arrivals of the runs that went through the twin = their lengths (the fallback runs are few)
        Buf<u64> tot(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(tot.get(), 0, 8, c->stream));
        hipLaunchKernelGGL(k_sum_bdesc_len, dim3((unsigned)std::min<u64>(1024, ceil_div(nbig, 256))), dim3(256), 0, c->stream, d_list, nbig, tot.get());
        tw.arrivals += d2h<u64>(c, tot.get());
    }
    const u32 nfb = d2h<u32>(c, fb_n.get());
    tw.runs += nbig - nfb;
    huge_stage<C>(c, fb.get(), fb_n.get(), nfb, a_lo, a_hi, nr, ma);
}
// the runs too long for one workgroup's sort (CLS_BIG, CLS_HUGE of the class lists): the twin path where the counting sort takes the suffixes, else the general kernel
template <typename C> void long_runs_stage(cblx_ctx* c, const BDesc* lists, const u32* list_n, const std::vector<u32>& ln, u64 nb, Resident& nr, const MergeArgs& ma, Twin& tw) {
    typedef typename C::HiT HiT;
    u64* a_lo = nr.a_lo.get();
    HiT* a_hi = C::WS ? (HiT*)nr.a_hi.get() : (HiT*)nullptr;
    if (msd_takes<C::WS>(c->P.SB)) big_stage<C>(c, lists + (size_t)CLS_BIG * nb, list_n + CLS_BIG, ln[CLS_BIG], nr, ma, tw);
    else huge_stage<C>(c, lists + (size_t)CLS_BIG * nb, list_n + CLS_BIG, ln[CLS_BIG], a_lo, a_hi, nr, ma);
    huge_stage<C>(c, lists + (size_t)CLS_HUGE * nb, list_n + CLS_HUGE, ln[CLS_HUGE], a_lo, a_hi, nr, ma);
}
// After every bucket kernel of the stage: the finished long runs sit in the twin, everything else in the arena. The buffer that
// holds more words becomes the arena; the other side's buckets are copied over (count[r] words at the same positions).
// `force`: -1 = the rule above; 0 / 1 = the result must end up in the arena / in the twin (a group of the grouped receiver, whose
// two buffers are a slot of the final arena and a scratch area: pipeline_group)
template <typename C> void finish_twin(cblx_ctx* c, Resident& nr, Twin& tw, int force = -1) {
    constexpr bool WS = C::WS;
    if (!tw.used()) return;
    if (force == 0 && tw.runs == 0) { tw = Twin(); return; }  // a preset twin nothing went through
    StageTimer t(c, ST_BBIG);
    const u64 T = d2h<u64>(c, nr.start.get() + nr.nb);
    const bool to_twin = force < 0 ? tw.arrivals * 2 > T : force == 1;
    const u64* src_lo = to_twin ? nr.a_lo.get() : tw.lo.get();
    const u64* src_hi = to_twin ? nr.a_hi.get() : tw.hi.get();
    u64* dst_lo = to_twin ? tw.lo.get() : nr.a_lo.get();
    u64* dst_hi = to_twin ? tw.hi.get() : nr.a_hi.get();
    // lanes per bucket: the long runs take a wave each; the others follow the average bucket length
    auto copy = [&](auto lpb) {
        constexpr int LPB = decltype(lpb)::value;
        hipLaunchKernelGGL((k_copy_buckets<WS, LPB>), lpb_grid(nr.nb, LPB), dim3(256), 0, c->stream, nr.nb, nr.start.get(), nr.cnt.get(), tw.in_twin.get(), to_twin ? 0u : 1u, src_lo, src_hi,
                           dst_lo, dst_hi);
    };
    if (to_twin) with_lpb(T - tw.arrivals, nr.nb - std::min<u64>(tw.runs, nr.nb), copy); else copy(std::integral_constant<int, 64>());
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));
    if (to_twin) {
        nr.a_lo = std::move(tw.lo);
        if (WS) nr.a_hi = std::move(tw.hi);
    }
    tw = Twin();
}

// KRN-3 over the runs of `nr` (run of a prefix = [its resident suffixes as stored][the new words in stream order]) in the
// arena a_lo / a_hi: per-bucket dedup / sort by size class; fills nr.cnt, nr.kind, nr.count. `old` = the resident index
// the runs were built against (tells which buckets are untouched and which are Tries already).
// `preset` (optional): the twin buffer of the long-run path, supplied by the caller (lo / hi set, same positions as the arena) instead of
// allocated here; `force`: see finish_twin
template <typename C> void bucket_stage(cblx_ctx* c, Resident& nr, const DirView& old, Twin* preset = nullptr, int force = -1) {
    typedef typename C::HiT HiT;
    const Consts& P = c->P;
    u64* a_lo = nr.a_lo.get();  // the arena (the long runs may move it to a twin buffer at the end: finish_twin)
    HiT* a_hi = C::WS ? (HiT*)nr.a_hi.get() : (HiT*)nullptr;
    Twin tw;
    if (preset) {
        tw = std::move(*preset);
        tw.in_twin = Buf<u8>(c->pool, nr.nb + 1);
        CBLX_HIP(hipMemsetAsync(tw.in_twin.get(), 0, nr.nb + 1, c->stream));
    }
    {
    const u64 nb = nr.nb;
    Buf<BDesc> lists(c->pool, (size_t)CLS_N * std::max<u64>(nb, 1));
    Buf<u32> list_n(c->pool, CLS_N);
    Buf<u32> res_count(c->pool, nb + 1);
    Buf<u8> res_kind(c->pool, nb + 1);
    CBLX_HIP(hipMemsetAsync(list_n.get(), 0, CLS_N * 4, c->stream));
    // (suffixes wider than 64 bits: an element takes 18 bytes of LDS, the 4096-word workgroup 82 KB = one per CU, and the Trie
    // classes cost 60 ps per word on 2000-word buckets against 10 on short ones. Sending runs over 2048 / 1024 words down the
    // long-run path instead was measured and is slower: 134 -> 143 / 165 ms per 1.2 G words at K = 59, the cost is the ranking
    // inside clusters of up to K mates, whatever the workgroup — so k_classify's `lds_max` is 4096 for every suffix width)
    hipLaunchKernelGGL(k_classify, grid1(nb, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nb, 4096u, nr.prefix.get(), nr.start.get(), old,
                       res_count.get(), res_kind.get(), nr.cnt.get(), nr.kind.get(), lists.get(), list_n.get());
    std::vector<u32> ln = d2h_vec<u32>(c, list_n.get(), CLS_N);
    if (ln[CLS_S32] | ln[CLS_S16]) {
        StageTimer t(c, ST_BSMALL);
        if (ln[CLS_S16])
            hipLaunchKernelGGL((k_bucket_small<16, C::WS, HiT>), grid1((u64)ln[CLS_S16] * 16, 256), dim3(256), 0, c->stream,
                               lists.get() + (size_t)CLS_S16 * nb, list_n.get() + CLS_S16, a_lo, a_hi, P.SB, nr.cnt.get(), nr.kind.get());
        if (ln[CLS_S32])
            hipLaunchKernelGGL((k_bucket_small<32, C::WS, HiT>), grid1((u64)ln[CLS_S32] * 32, 256), dim3(256), 0, c->stream,
                               lists.get() + (size_t)CLS_S32 * nb, list_n.get() + CLS_S32, a_lo, a_hi, P.SB, nr.cnt.get(), nr.kind.get());
    }
    // whether the batch looks like one full of repeats: some shorter run gave up in the counting sort (unknown = yes when
    // there are no shorter runs at all). Long runs of distinct words — the receiving side of a many-GPU build — then skip
    // the pre-pass below altogether.
    bool saw_repeats = true;
    {
        StageTimer t(c, ST_BMED);
        // fast path (counting sort on the top suffix bits + in-sub-bucket ranking); a run with a crowded sub-bucket marks its
        // list entry and takes the claim-table kernel of its length class (runs full of repeats); what needs the sorted layout
        // after that goes to the LDS radix sort
        constexpr int NM = N_LEN_CLASSES;
        u64 roff[NM + 1] = {0};
        for (int k = 0; k < NM; ++k) roff[k + 1] = roff[k] + ln[LEN_CLASSES[k].cls];
        Buf<u8> bail(c->pool, roff[NM] + 8);
        Buf<u32> bail_any(c->pool, NM + 1);  // one word per class, then the radix kernel's list counter
        Buf<BDesc> retry2(c->pool, std::max<u64>(roff[NM], 1));
        CBLX_HIP(hipMemsetAsync(bail.get(), 0, roff[NM] + 8, c->stream));
        CBLX_HIP(hipMemsetAsync(bail_any.get(), 0, (NM + 1) * 4, c->stream));
        u32* r2n = bail_any.get() + NM;
        // The classes up to 1024 words (hashed sub-buckets) never give up without repeats in the batch: once one of them did
        // — the shortest is asked first — the classes after it start with the claim table (`repeat_mode`) instead of a
        // counting sort that is going to give up.
        bool repeat_mode = false;
        std::vector<u32> any(NM, 0u);
        bool used_msd[NM] = {false};
        auto any_of = [&](const std::vector<u32>& v) { u32 a = 0; for (u32 x : v) a |= x; return a != 0; };
        const bool radix_only = !msd_takes<C::WS>(P.SB);
        if (radix_only) {
            radix_only_classes<C>(c, lists.get(), list_n.get(), ln, nb, nr, MergeArgs{});
            CBLX_HIP(hipGetLastError());
        }
        with_packed<C>(P, [&](auto packed_tag) {
            constexpr bool PK = decltype(packed_tag)::value;
            if (radix_only) return;
            auto go = [&](auto kc) {
                constexpr int k = decltype(kc)::value, T = LEN_CLASSES[k].threads, CAPV = LEN_CLASSES[k].cap, cls = LEN_CLASSES[k].cls;
                if (!ln[cls]) return;
                // (the claim table as FIRST kernel of every run <= 1024 words, measured: cfg 2, no repeats, +0.25 ms; the 30x-coverage workload -2.4 ms)
                if (repeat_mode) {
                    hipLaunchKernelGGL((k_bucket_claim<T, CAPV, C::WS, HiT>), dim3(ln[cls]), dim3(T), 0, c->stream, lists.get() + (size_t)cls * nb, list_n.get() + cls, a_lo, a_hi, P.SB,
                                       nr.cnt.get(), nr.kind.get(), retry2.get(), r2n, (const u8*)nullptr);
                    return;
                }
                used_msd[k] = true;
                launch_run_sort<C, SORT_BUILD, PK>(c, kc, lists.get() + (size_t)cls * nb, list_n.get() + cls, ln[cls], a_lo, a_hi, nr.cnt.get(), nr.kind.get(),
                                                   SortOut{nullptr, nullptr, bail.get() + roff[k], bail_any.get() + k});
            };
            go(len_class<0>);
            if (used_msd[0] && (ln[CLS_M32] | ln[CLS_M64] | ln[CLS_M128] | ln[CLS_M256] | ln[CLS_M512]))  // the shortest class is the cheapest witness
                repeat_mode = d2h<u32>(c, bail_any.get() + 0) != 0;
            go(len_class<1>);
            go(len_class<2>);
            go(len_class<3>);
            if (!repeat_mode && (ln[CLS_M256] | ln[CLS_M512]) && (used_msd[1] | used_msd[2] | used_msd[3]))
                repeat_mode = any_of(d2h_vec<u32>(c, bail_any.get(), 4));
            go(len_class<4>);
            go(len_class<5>);
            if (!roff[NM]) return;
            any = d2h_vec<u32>(c, bail_any.get(), NM);
            each_len_class([&](auto kc) {
                constexpr int k = decltype(kc)::value, T = LEN_CLASSES[k].threads, CAPV = LEN_CLASSES[k].cap, cls = LEN_CLASSES[k].cls;
                if (!used_msd[k] || !any[k]) return;
                hipLaunchKernelGGL((k_bucket_claim<T, CAPV, C::WS, HiT>), dim3((ln[cls] + 63) / 64), dim3(T), 0, c->stream, lists.get() + (size_t)cls * nb, list_n.get() + cls, a_lo, a_hi,
                                   P.SB, nr.cnt.get(), nr.kind.get(), retry2.get(), r2n, (const u8*)(bail.get() + roff[k]));
            });
            if (repeat_mode || any_of(any)) {
                // what the claim tables left for the sorted layout: distinct words now, at most 4096 per run
                const u32 n2 = d2h<u32>(c, r2n);
                if (n2) {
                    Buf<BDesc> retry3(c->pool, n2);
                    Buf<u32> r3n(c->pool, 1);
                    CBLX_HIP(hipMemsetAsync(r3n.get(), 0, 4, c->stream));
                    launch_run_sort<C, SORT_SORTED, PK>(c, len_class<len_class_of(4096)>, retry2.get(), r2n, n2, a_lo, a_hi, nr.cnt.get(), nr.kind.get(), SortOut{retry3.get(), r3n.get()});
                    const u32 n3 = d2h<u32>(c, r3n.get());
                    if (n3)
                        hipLaunchKernelGGL((k_bucket_medium<512, C::WS, HiT>), dim3(n3), dim3(512), 0, c->stream, retry3.get(), r3n.get(), a_lo, a_hi, P.SB, nr.cnt.get(), nr.kind.get(), MergeArgs{});
                    CBLX_HIP(hipStreamSynchronize(c->stream));  // retry3 dies here
                }
            }
        });
        saw_repeats = roff[NM] ? repeat_mode : true;  // no shorter runs at all: unknown = yes
        if (roff[NM] && !repeat_mode && (ln[CLS_BIG] | ln[CLS_HUGE]) && any_of(any)) {
            // no shorter hashed runs to tell: a sizeable share of the runs that went through the counting sort must have given up
            // (a few do without a single repeat — necklace clusters)
            Buf<u64> nbail(c->pool, 1);
            CBLX_HIP(hipMemsetAsync(nbail.get(), 0, 8, c->stream));
            hipLaunchKernelGGL(k_sum_u8, dim3((unsigned)std::min<u64>(1024, ceil_div(roff[NM], 256))), dim3(256), 0, c->stream, bail.get(), roff[NM], nbail.get());
            saw_repeats = d2h<u64>(c, nbail.get()) * 8 >= roff[NM];
        }
        CBLX_HIP(hipStreamSynchronize(c->stream));  // retry buffers die here
    }
    bool long_done = false;
    if constexpr (!C::WS) {
        if (P.SB < 64 && ln[CLS_BIG] + ln[CLS_HUGE] > 0 && saw_repeats) {
            // runs too long for one workgroup's sort: first the pre-pass that shrinks the ones full of repeats to their first
            // occurrences (k_big_claim); what it passes on takes the paths below, what it shrank to more than 1024 distinct
            // words is sorted by one workgroup
            const u32 nbig = ln[CLS_BIG], nhuge = ln[CLS_HUGE];
            Buf<BDesc> next_big(c->pool, std::max<u32>(nbig, 1)), next_huge(c->pool, std::max<u32>(nhuge, 1)), srt(c->pool, (size_t)nbig + nhuge), retry(c->pool, (size_t)nbig + nhuge);
            Buf<u32> cnts(c->pool, 4);  // next_big, next_huge, sorted, retry
            std::vector<u32> cn;
            {
            StageTimer t(c, ST_BBIG);
            CBLX_HIP(hipMemsetAsync(cnts.get(), 0, 16, c->stream));
            if (nbig)
                hipLaunchKernelGGL((k_big_claim<HiT>), dim3(nbig), dim3(BCL_THREADS), 0, c->stream, lists.get() + (size_t)CLS_BIG * nb, list_n.get() + CLS_BIG, a_lo, P.SB, nr.cnt.get(),
                                   nr.kind.get(), next_big.get(), cnts.get() + 0, srt.get(), cnts.get() + 2);
            if (nhuge)
                hipLaunchKernelGGL((k_big_claim<HiT>), dim3(nhuge), dim3(BCL_THREADS), 0, c->stream, lists.get() + (size_t)CLS_HUGE * nb, list_n.get() + CLS_HUGE, a_lo, P.SB, nr.cnt.get(),
                                   nr.kind.get(), next_huge.get(), cnts.get() + 1, srt.get(), cnts.get() + 2);
            cn = d2h_vec<u32>(c, cnts.get(), 3);
            if (cn[2]) {
                with_packed<C>(P, [&](auto pk) {
                    launch_run_sort<C, SORT_SORTED, decltype(pk)::value>(c, len_class<len_class_of(2048)>, srt.get(), cnts.get() + 2, cn[2], a_lo, a_hi, nr.cnt.get(), nr.kind.get(),
                                                                         SortOut{retry.get(), cnts.get() + 3});
                });
                const u32 nre = d2h<u32>(c, cnts.get() + 3);
                if (nre)
                    hipLaunchKernelGGL((k_bucket_medium<512, false, HiT>), dim3(nre), dim3(512), 0, c->stream, retry.get(), cnts.get() + 3, a_lo, a_hi, P.SB, nr.cnt.get(), nr.kind.get(), MergeArgs{});
            }
            CBLX_HIP(hipGetLastError());
            }
            big_stage<C>(c, next_big.get(), cnts.get() + 0, cn[0], nr, MergeArgs{}, tw);
            huge_stage<C>(c, next_huge.get(), cnts.get() + 1, cn[1], a_lo, a_hi, nr, MergeArgs{});
            CBLX_HIP(hipStreamSynchronize(c->stream));  // the lists die here
            long_done = true;
        }
    }
    if (!long_done) long_runs_stage<C>(c, lists.get(), list_n.get(), ln, nb, nr, MergeArgs{}, tw);
    }
    CBLX_HIP(hipGetLastError());
    finish_twin<C>(c, nr, tw, force);
    count_words(c, nr);
}

}  // namespace
