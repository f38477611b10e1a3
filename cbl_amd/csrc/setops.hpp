// setops.hpp — set algebra between resident indexes and k-mer removal, on the host: `self |= other` (merge_direct), `a OP b` into a new index and the
// assigning forms (set_op_build), CBL::merge / CBL::intersect of n operands (set_op_many_build), the k-mers at least t of n hold and the occupancy histogram (at_least_build), |a AND b| alone (intersection_count), WordSet::remove_batch (remove_words). They share the
// bucket stages of bucket_stage.hpp and the end of a result (set_op_tail). Kernels: kernels_setops.hpp, kernels_remove.hpp. Included by cblx.cpp only.
#pragma once
#include "kernels_remove.hpp"
#include "kernels_setops.hpp"
#include "pipeline.hpp"

namespace {

// ---- pieces the set-algebra drivers below share ------------------------------------------------------------------
// the per-bucket rows of a directory of nr.nb buckets (one spare entry each: start[nb] is the arena's length)
inline void alloc_dir_rows(cblx_ctx* c, Resident& nr) {
    nr.prefix = Buf<u32>(c->pool, nr.nb + 1);
    nr.start = Buf<u64>(c->pool, nr.nb + 1);
    nr.cnt = Buf<u32>(c->pool, nr.nb + 1);
    nr.kind = Buf<u8>(c->pool, nr.nb + 1);
}
// The runs are sealed — start[] = the scan of their capacities `cap`, start[nb] = the sum N — and an arena of N words is allocated. Returns N.
template <bool WS> u64 seal_runs(cblx_ctx* c, Resident& nr, const u32* cap) {
    const u64 N = exclusive_scan<u64>(c, cap, nr.nb, nr.start.get());
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, nr.start.get() + nr.nb, N);
    CBLX_HIP(hipGetLastError());
    nr.a_lo = Buf<u64>(c->pool, N + 2);
    if (WS) nr.a_hi = Buf<u64>(c->pool, N + 2);
    return N;
}
// f(OP) with the operation as a compile-time constant
template <typename F> void with_setop(u32 op, F&& f) {
    if (op == SETOP_OR) f(std::integral_constant<u32, SETOP_OR>());
    else if (op == SETOP_AND) f(std::integral_constant<u32, SETOP_AND>());
    else if (op == SETOP_SUB) f(std::integral_constant<u32, SETOP_SUB>());
    else f(std::integral_constant<u32, SETOP_XOR>());
}

// ---- `self |= other`, both resident on this device (src/cbl.rs:433-449 -> src/wordset/set_ops.rs:123-157) ---------
// `s`: self's index (c->res for `c |= o`; another context's for cblx_merge_from, which leaves it untouched); the result becomes c->res
template <typename C> void merge_direct(cblx_ctx* c, const Resident& s, const Resident& o) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    Resident nr;
    Buf<u32> raw, m_cs;
    Buf<u64> m_sstart, m_ostart;
    Buf<u8> m_skind, m_okind;
    u64 N = 0;
    {
        StageTimer t(c, ST_DIR);
        Buf<u32> popc(c->pool, nwords);
        nr.bv = Buf<u64>(c->pool, nwords);
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        hipLaunchKernelGGL(k_setop_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, s.bv.get(), o.bv.get(), SETOP_OR, nr.bv.get(), popc.get());
        nr.nb = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
        const u64 nb = nr.nb;
        alloc_dir_rows(c, nr);
        raw = Buf<u32>(c->pool, nb + 1);
        m_cs = Buf<u32>(c->pool, nb + 1);
        m_sstart = Buf<u64>(c->pool, nb + 1);
        m_ostart = Buf<u64>(c->pool, nb + 1);
        m_skind = Buf<u8>(c->pool, nb + 1);
        m_okind = Buf<u8>(c->pool, nb + 1);
        hipLaunchKernelGGL(k_merge_table, grid1(nprefix, 256), dim3(256), 0, c->stream, nprefix, nr.bv.get(), nr.rank_dir.get(), s.view(), o.view(), nr.prefix.get(),
                           raw.get(), m_cs.get(), m_sstart.get(), m_ostart.get(), m_skind.get(), m_okind.get());
        N = seal_runs<WS>(c, nr, raw.get());
    }
    if (N != s.count + o.count) throw Error(CBLX_EDEVICE, "merge: run lengths do not match the two indexes (internal error)");
    const u64 nb = nr.nb;
    // Trie |= Trie (both lists ascending): merged by k_bucket_union straight from the two arenas — not gathered, not sorted again
    // (wide suffixes too since round 5: two-word elements). CBLX_MERGE_UNION=0 keeps the counting-sort route (tests compare the two)
    const char* union_env = std::getenv("CBLX_MERGE_UNION");  // (read per call: tests switch it)
    const bool union_path = !(union_env && union_env[0] == '0');
    // both-sided buckets of up to 4096 words (the counting-sort classes) are read where they are stored: their kernel loads self's part from
    // self's arena and other's from other's, and only the result is written — the gather moved 16 bytes per word for nothing.
    // CBLX_MERGE_DIRECT=0 gathers them as before
    const char* direct_env = std::getenv("CBLX_MERGE_DIRECT");
    const bool direct = msd_takes<WS>(P.SB) && !(direct_env && direct_env[0] == '0');
    const u32 direct_upto = direct ? 512u * MED_ITEMS : 0u;
    {
        StageTimer t(c, ST_EXPAND);
        with_lpb(N, nb, [&](auto lpb) {
            constexpr int LPB = decltype(lpb)::value;
            hipLaunchKernelGGL((k_merge_gather<WS, LPB>), lpb_grid(nb, LPB), dim3(256), 0, c->stream, nb, nr.start.get(), m_cs.get(), m_sstart.get(), m_ostart.get(),
                               s.a_lo.get(), s.a_hi.get(), o.a_lo.get(), o.a_hi.get(), nr.a_lo.get(), nr.a_hi.get(), union_path ? m_skind.get() : (const u8*)nullptr,
                               union_path ? m_okind.get() : (const u8*)nullptr, direct_upto);
        });
    }
    Buf<BDesc> lists(c->pool, (size_t)CLS_N * std::max<u64>(nb, 1));
    Buf<u32> list_n(c->pool, CLS_N);
    CBLX_HIP(hipMemsetAsync(list_n.get(), 0, CLS_N * 4, c->stream));
    const bool prof = (c->flags & CBLX_FLAG_PROFILE) != 0;
    Buf<unsigned long long> cls_words;
    if (prof) { cls_words = Buf<unsigned long long>(c->pool, CLS_N + 2); CBLX_HIP(hipMemsetAsync(cls_words.get(), 0, (CLS_N + 2) * 8, c->stream)); }
    hipLaunchKernelGGL(k_classify_merge, grid1(nb, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nb, WS ? 512u : 1024u, nr.start.get(), m_cs.get(), m_skind.get(), m_okind.get(),
                       nr.cnt.get(), nr.kind.get(), lists.get(), list_n.get(), union_path, cls_words.get());
    CBLX_HIP(hipGetLastError());
    std::vector<u32> ln = d2h_vec<u32>(c, list_n.get(), CLS_N);
    std::vector<unsigned long long> cw;
    if (prof) cw = d2h_vec<unsigned long long>(c, cls_words.get(), CLS_N + 1);
    const MergeArgs ma{m_cs.get(), m_ostart.get(), m_okind.get(), o.a_lo.get(), o.a_hi.get()};  // (kernels that work on the gathered run)
    MergeArgs ma_msd = ma;                                                                       // (the counting-sort classes: in place)
    if (direct) { ma_msd.s_lo = s.a_lo.get(); ma_msd.s_hi = s.a_hi.get(); ma_msd.sstart = m_sstart.get(); }
    u64* a_lo = nr.a_lo.get();
    HiT* a_hi = WS ? (HiT*)nr.a_hi.get() : (HiT*)nullptr;
    // (Round 5 measured the unions on a second stream beside the counting-sort classes — launched first they take every wave slot and the two run one
    //  after the other, launched second they share the chip and the pair takes exactly the sum of the two: 10.10 against 10.06 ms. One stream it stays.)
    if (ln[CLS_UNION]) {
        StageTimer t(c, ST_BBIG);
        hipLaunchKernelGGL((k_bucket_union<WS>), dim3(ln[CLS_UNION]), dim3(UNI_THREADS), 0, c->stream, lists.get() + (size_t)CLS_UNION * nb, list_n.get() + CLS_UNION, m_cs.get(), m_sstart.get(),
                           m_ostart.get(), (const u64*)s.a_lo.get(), (const u64*)s.a_hi.get(), (const u64*)o.a_lo.get(), (const u64*)o.a_hi.get(), a_lo, (u64*)nr.a_hi.get(), P.SB,
                           nr.cnt.get(), nr.kind.get());
        CBLX_HIP(hipGetLastError());
    }
    {
        StageTimer t(c, ST_BMED);
        // both-sided buckets: counting sort on the top suffix bits + ranking inside the sub-buckets (k_bucket_msd in its
        // merge mode); a bucket with a crowded sub-bucket comes back through `retry` and takes the LDS radix sort
        Buf<BDesc> retry(c->pool, std::max<u64>(nb, 1));
        Buf<u32> retry_n(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(retry_n.get(), 0, 4, c->stream));
        if (!msd_takes<WS>(P.SB)) radix_only_classes<C>(c, lists.get(), list_n.get(), ln, nb, nr, ma);
        else
            with_packed<C>(P, [&](auto pk) {
                each_len_class([&](auto kc) {
                    constexpr int cls = LEN_CLASSES[decltype(kc)::value].cls;
                    if constexpr (cls != CLS_M32)  // (k_classify_merge has no such class)
                        if (ln[cls])
                            launch_run_sort<C, SORT_MERGE, decltype(pk)::value>(c, kc, lists.get() + (size_t)cls * nb, list_n.get() + cls, ln[cls], a_lo, a_hi, nr.cnt.get(), nr.kind.get(),
                                                                                SortOut{retry.get(), retry_n.get()}, ma_msd);
                });
            });
        const u32 nretry = (ln[CLS_M16] || ln[CLS_M64] || ln[CLS_M128] || ln[CLS_M256] || ln[CLS_M512]) ? d2h<u32>(c, retry_n.get()) : 0u;
        if (nretry) {
            if (direct)  // (these buckets were not gathered: the radix kernel works on the run)
                hipLaunchKernelGGL((k_merge_gather_list<WS>), dim3(nretry), dim3(256), 0, c->stream, retry.get(), retry_n.get(), m_cs.get(), m_sstart.get(), m_ostart.get(), s.a_lo.get(),
                                   s.a_hi.get(), (const u64*)o.a_lo.get(), (const u64*)o.a_hi.get(), nr.a_lo.get(), nr.a_hi.get());
            hipLaunchKernelGGL((k_bucket_medium<512, WS, HiT>), dim3(nretry), dim3(512), 0, c->stream, retry.get(), retry_n.get(), a_lo, a_hi, P.SB, nr.cnt.get(), nr.kind.get(), ma);
        }
        if constexpr (!WS) if (ln[CLS_M1024])
            hipLaunchKernelGGL((k_bucket_medium<1024, WS, HiT>), dim3(ln[CLS_M1024]), dim3(1024), 0, c->stream, lists.get() + (size_t)CLS_M1024 * nb,
                               list_n.get() + CLS_M1024, a_lo, a_hi, P.SB, nr.cnt.get(), nr.kind.get(), ma);
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // retry buffers die here
    }
    {
        Twin tw;
        long_runs_stage<C>(c, lists.get(), list_n.get(), ln, nb, nr, ma, tw);
        finish_twin<C>(c, nr, tw);
    }
    count_words(c, nr);
    if (prof) {
        // words every stage's kernels were given (cblx_stage_units): the gather copies the one-sided buckets and the both-sided ones their
        // kernel does not read in place; the unions are priced on what they WRITE (2 BYTES read + BYTES written per output)
        u64 msd = 0, gathered = cw[CLS_N];
        for (int cls : {CLS_M16, CLS_M64, CLS_M128, CLS_M256, CLS_M512}) msd += cw[cls];
        if (!direct) gathered += msd;
        gathered += cw[CLS_M1024] + cw[CLS_HUGE] + cw[CLS_BIG];
        c->stages[ST_EXPAND].units += gathered;
        c->stages[ST_BMED].units += msd + cw[CLS_M1024];
        c->stages[ST_BHUGE].units += cw[CLS_HUGE];
        u64 uni_out = 0;
        if (ln[CLS_UNION]) {
            Buf<u64> tot(c->pool, 1);
            CBLX_HIP(hipMemsetAsync(tot.get(), 0, 8, c->stream));
            hipLaunchKernelGGL(k_sum_list_counts, dim3((unsigned)std::min<u64>(1024, ceil_div(ln[CLS_UNION], 256))), dim3(256), 0, c->stream, lists.get() + (size_t)CLS_UNION * nb, ln[CLS_UNION],
                               (const u32*)nr.cnt.get(), tot.get());
            uni_out = d2h<u64>(c, tot.get());
        }
        c->stages[ST_BBIG].units += uni_out + cw[CLS_BIG];
    }
    c->res = std::move(nr);
}

// The Vec buckets of one operand that a set operation visits with iter_sorted, sorted where they are stored: runs of up to 4096 words (`l_lds`, list_n[0]) take
// the LDS radix sort, longer ones (`l_gen`, list_n[1]) the general kernel; `junk` takes the counts and kinds they report.
template <typename C> void sort_vec_sides(cblx_ctx* c, Resident& x, const BDesc* l_lds, const BDesc* l_gen, const u32* list_n, u32 n_lds, u32 n_gen, Resident& junk) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    u64* x_lo = x.a_lo.get();
    HiT* x_hi = WS ? (HiT*)x.a_hi.get() : (HiT*)nullptr;
    if (n_lds) {
        StageTimer t(c, ST_BMED);
        hipLaunchKernelGGL((k_bucket_medium<512, WS, HiT>), dim3(n_lds), dim3(512), 0, c->stream, l_lds, list_n, x_lo, x_hi, c->P.SB, junk.cnt.get(), junk.kind.get(), MergeArgs{});
        CBLX_HIP(hipGetLastError());
    }
    huge_stage<C>(c, l_gen, list_n + 1, n_gen, x_lo, x_hi, junk, MergeArgs{});
}
// The end of a set operation into a new index: candidates that came out empty leave the directory, the k-mers are counted. `popc` is scratch of nwords
// counters, N the arena's length. false: nothing is left (the result is the empty index).
inline bool set_op_tail(cblx_ctx* c, Resident& nr, Buf<u32>& popc, u64 nwords, u64 N) {
    const u64 nb = nr.nb;
    {
        // buckets that came out empty leave the directory (never for OR)
        StageTimer t(c, ST_DIR);
        Buf<u32> live(c->pool, nb);
        Buf<u64> new_rank(c->pool, nb);
        hipLaunchKernelGGL(k_setop_live, grid1(nb, 256), dim3(256), 0, c->stream, nb, nr.cnt.get(), live.get());
        const u64 kept = exclusive_scan<u64>(c, live.get(), nb, new_rank.get());
        if (kept == 0) { CBLX_HIP(hipStreamSynchronize(c->stream)); return false; }
        if (kept != nb) {
            Resident cr;
            cr.nb = kept;
            cr.bv = Buf<u64>(c->pool, nwords);
            cr.rank_dir = Buf<u64>(c->pool, nwords + 1);
            alloc_dir_rows(c, cr);
            CBLX_HIP(hipMemsetAsync(cr.bv.get(), 0, nwords * 8, c->stream));
            hipLaunchKernelGGL(k_setop_compact, grid1(nb, 256), dim3(256), 0, c->stream, nb, nr.cnt.get(), new_rank.get(), nr.prefix.get(), nr.start.get(), nr.kind.get(),
                               cr.prefix.get(), cr.start.get(), cr.cnt.get(), cr.kind.get(), cr.bv.get());
            hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, cr.start.get() + kept, N);
            hipLaunchKernelGGL(k_popc_words, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, cr.bv.get(), popc.get());
            CBLX_HIP(hipGetLastError());
            if (exclusive_scan<u64>(c, popc.get(), nwords, cr.rank_dir.get()) != kept) throw Error(CBLX_EDEVICE, "set_op: the compacted directory does not match its bitvector (internal error)");
            cr.a_lo = std::move(nr.a_lo);
            cr.a_hi = std::move(nr.a_hi);
            CBLX_HIP(hipStreamSynchronize(c->stream));  // the old tables die here
            nr = std::move(cr);
        }
    }
    count_words(c, nr);
    return true;
}

// ---- `&mut a OP &mut b` into a new index, all three resident on this device (src/cbl.rs:411-431, 451-471, 491-511, 531-551 -> src/wordset/set_ops.rs) ----
// The result becomes c->res. `a` and `b` keep their sets; their Vec buckets on the prefixes both hold are sorted in their own arenas (iter_sorted's side
// effect). Both operands are non-empty (the caller answers the other cases with a clone or an empty index).
// The arena keeps slack inside the runs of the both-sided buckets (a run is as long as the op's upper bound), as the results of `|=` do: the serializer,
// cblx_validate and the queries read start[r] and cnt[r] only.
// `assign`: the layout of the ASSIGNING forms `a &= &mut b`, `a -= &mut b`, `a ^= &mut b` (src/cbl.rs:473-489, 513-529, 553-569 -> src/wordset/set_ops.rs:192-239,
// 281-317, 366-410 -> src/trievec/set_ops.rs:101-129, 163-187, 226-257): same candidates, same one-sided buckets, same sorts, but a both-sided bucket keeps a's kind
// — a Trie is the ascending result, a Vec is what remove_sorted_iter's swap_remove leaves (k_bucket_setop_assign). The file holds neither container ids nor the
// tiered vector nor empty_containers, so the result is this per-bucket function of the operands.
template <typename C> Resident set_op_build(cblx_ctx* c, Resident& a, Resident& b, u32 op, bool assign) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    Resident nr;
    Buf<u32> cap, m_cs, m_co, popc(c->pool, nwords);
    Buf<u64> m_sstart, m_ostart;
    Buf<u8> m_skind, m_okind;
    Buf<BDesc> sort_lists, both_list;  // both_list: [1][nb], or [3][nb] by the kernel that takes the bucket (assign)
    Buf<u32> list_n(c->pool, 7);
    Buf<unsigned long long> scratch_n(c->pool, 1);  // (assign) words of global tables the long Vec buckets need
    u64 N = 0;
    {
        StageTimer t(c, ST_DIR);
        nr.bv = Buf<u64>(c->pool, nwords);
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        hipLaunchKernelGGL(k_setop_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, a.bv.get(), b.bv.get(), op, nr.bv.get(), popc.get());
        nr.nb = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
        if (nr.nb == 0) return Resident();  // (AND of indexes that share no prefix)
        const u64 nb = nr.nb;
        alloc_dir_rows(c, nr);
        cap = Buf<u32>(c->pool, nb + 1);
        m_cs = Buf<u32>(c->pool, nb + 1);
        m_co = Buf<u32>(c->pool, nb + 1);
        m_sstart = Buf<u64>(c->pool, nb + 1);
        m_ostart = Buf<u64>(c->pool, nb + 1);
        m_skind = Buf<u8>(c->pool, nb + 1);
        m_okind = Buf<u8>(c->pool, nb + 1);
        sort_lists = Buf<BDesc>(c->pool, 4 * nb);
        both_list = Buf<BDesc>(c->pool, (assign ? 3 : 1) * nb);
        CBLX_HIP(hipMemsetAsync(list_n.get(), 0, 7 * 4, c->stream));
        CBLX_HIP(hipMemsetAsync(scratch_n.get(), 0, 8, c->stream));
        hipLaunchKernelGGL(k_merge_table, grid1(nprefix, 256), dim3(256), 0, c->stream, nprefix, nr.bv.get(), nr.rank_dir.get(), a.view(), b.view(), nr.prefix.get(),
                           cap.get(), m_cs.get(), m_sstart.get(), m_ostart.get(), m_skind.get(), m_okind.get());
        hipLaunchKernelGGL(assign ? k_setop_plan<true> : k_setop_plan<false>, grid1(nb, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nb, op, cap.get(), m_cs.get(), m_co.get(),
                           m_sstart.get(), m_ostart.get(), m_skind.get(), m_okind.get(), nr.cnt.get(), nr.kind.get(), sort_lists.get(), both_list.get(), list_n.get(), scratch_n.get());
        N = seal_runs<WS>(c, nr, cap.get());
    }
    const u64 nb = nr.nb;
    {
        StageTimer t(c, ST_EXPAND);
        with_lpb(N, nb, [&](auto lpb) {
            constexpr int LPB = decltype(lpb)::value;
            hipLaunchKernelGGL((k_setop_gather<WS, LPB>), lpb_grid(nb, LPB), dim3(256), 0, c->stream, nb, nr.start.get(), m_cs.get(), m_co.get(), m_sstart.get(), m_ostart.get(),
                               (const u64*)a.a_lo.get(), (const u64*)a.a_hi.get(), (const u64*)b.a_lo.get(), (const u64*)b.a_hi.get(), nr.a_lo.get(), nr.a_hi.get());
        });
        CBLX_HIP(hipGetLastError());
    }
    const std::vector<u32> ln = d2h_vec<u32>(c, list_n.get(), 7);
    {
        // step 1: the Vec sides of the both-sided buckets, sorted where they are stored. Runs of up to 4096 words take the LDS radix sort, longer ones (a Vec
        // left by an earlier `|=` or set operation has no length limit) the general kernel; both are asked for the sorted layout and write the count and
        // kind they find — the operand's own, unchanged: its words are distinct — into a table nobody reads.
        Resident junk;
        junk.cnt = Buf<u32>(c->pool, nb + 1);
        junk.kind = Buf<u8>(c->pool, nb + 1);
        for (int side = 0; side < 2; ++side)
            sort_vec_sides<C>(c, side ? b : a, sort_lists.get() + (size_t)(2 * side) * nb, sort_lists.get() + (size_t)(2 * side + 1) * nb, list_n.get() + 2 * side, ln[2 * side],
                              ln[2 * side + 1], junk);
        CBLX_HIP(hipStreamSynchronize(c->stream));  // `junk` dies here
    }
    if (ln[4]) {
        // step 2: both lists ascending now, whatever their kinds
        StageTimer t(c, ST_BBIG);
        with_setop(op, [&](auto opc) {
            constexpr u32 OP = decltype(opc)::value;
            hipLaunchKernelGGL((k_bucket_setop<WS, OP>), dim3(ln[4]), dim3(UNI_THREADS), 0, c->stream, both_list.get(), list_n.get() + 4, m_cs.get(), m_co.get(), m_sstart.get(),
                               m_ostart.get(), (const u64*)a.a_lo.get(), (const u64*)a.a_hi.get(), (const u64*)b.a_lo.get(), (const u64*)b.a_hi.get(), (const u64*)nr.start.get(),
                               nr.a_lo.get(), nr.a_hi.get(), P.SB, nr.cnt.get(), assign ? (u8*)nullptr : nr.kind.get());  // (assign: a's side is a Trie and stays one)
        });
        CBLX_HIP(hipGetLastError());
    }
    Buf<u32> scratch;
    if (assign && (ln[5] || ln[6])) {
        // step 2, a's side a Vec: membership, the pushed words of `^=` and the swap_remove layout in one kernel; tables in LDS up to SA_LDS words, else in `scratch`
        StageTimer t(c, ST_BSMALL);
        if (ln[6]) scratch = Buf<u32>(c->pool, d2h<unsigned long long>(c, scratch_n.get()) + 1);
        auto go = [&](auto opc, auto big) {
            constexpr u32 OP = decltype(opc)::value;
            constexpr bool BIG = decltype(big)::value;
            const u32 n = ln[BIG ? 6 : 5];
            if (n)
                hipLaunchKernelGGL((k_bucket_setop_assign<WS, OP, BIG>), dim3(n), dim3(SA_THREADS), 0, c->stream, both_list.get() + (size_t)(BIG ? 2 : 1) * nb, list_n.get() + (BIG ? 6 : 5),
                                   m_cs.get(), m_co.get(), m_sstart.get(), m_ostart.get(), (const u64*)a.a_lo.get(), (const u64*)a.a_hi.get(), (const u64*)b.a_lo.get(),
                                   (const u64*)b.a_hi.get(), (const u64*)nr.start.get(), nr.a_lo.get(), nr.a_hi.get(), P.SB, nr.cnt.get(), nr.kind.get(), scratch.get());
        };
        with_setop(op, [&](auto opc) {
            if constexpr (decltype(opc)::value != SETOP_OR) { go(opc, std::false_type()); go(opc, std::true_type()); }  // (`|=` is merge_direct)
        });
        CBLX_HIP(hipGetLastError());
    }
    if (!set_op_tail(c, nr, popc, nwords, N)) return Resident();
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the lists and tables of this call die here
    return nr;
}
// The Vec sides of an n-ary operation, one operand after the other through the same two lists (the launches of one operand are behind it when its counts are
// read). `op` is k_many_sortplan's rule: SETOP_OR — candidates two or more hold; SETOP_AND — every candidate the operand holds.
template <typename C> void sort_many_sides(cblx_ctx* c, const std::vector<Resident*>& xs, const ManyOp* ops, u64 nb, const u32* prefix, const u64* hmask, u32 op) {
    Resident junk;
    junk.cnt = Buf<u32>(c->pool, nb + 1);
    junk.kind = Buf<u8>(c->pool, nb + 1);
    Buf<BDesc> sort_lists(c->pool, 2 * nb);
    Buf<u32> sort_n(c->pool, 2);
    for (u32 i = 0; i < (u32)xs.size(); ++i) {
        CBLX_HIP(hipMemsetAsync(sort_n.get(), 0, 2 * 4, c->stream));
        hipLaunchKernelGGL(k_many_sortplan, grid1(nb, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nb, prefix, hmask, op, ops, i, sort_lists.get(), sort_n.get());
        CBLX_HIP(hipGetLastError());
        const std::vector<u32> sn = d2h_vec<u32>(c, sort_n.get(), 2);
        sort_vec_sides<C>(c, *xs[i], sort_lists.get(), sort_lists.get() + nb, sort_n.get(), sn[0], sn[1], junk);
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the lists are rewritten for the next operand
    }
}
// ---- CBL::merge / CBL::intersect of n operands into a new index (src/cbl.rs:106-124 -> src/wordset/set_ops.rs:11-42, 49-75), all resident on this device ----
// `xs`: 1 .. 64 non-empty operands in the caller's order (an empty one contributes nothing to a merge and empties an intersection: the caller's business).
// op: SETOP_OR (merge) | SETOP_AND (intersect). Every operand keeps its set; its Vec buckets on the prefixes the reference visits with iter_sorted — merge:
// two holders or more, intersect: held by all — are sorted in its own arena. The rules per bucket are at k_many_table / k_bucket_setop_many.
template <typename C> Resident set_op_many_build(cblx_ctx* c, const std::vector<Resident*>& xs, u32 op) {
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    const u32 n = (u32)xs.size();
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    std::vector<ManyOp> h_ops(n);
    for (u32 i = 0; i < n; ++i) h_ops[i] = ManyOp{xs[i]->view(), xs[i]->a_lo.get(), xs[i]->a_hi.get()};
    Buf<ManyOp> ops(c->pool, n);
    h2d(c, ops.get(), h_ops.data(), n);
    Resident nr;
    Buf<u32> cap, popc(c->pool, nwords), list_n(c->pool, 3);
    Buf<u64> hmask;
    Buf<BDesc> lists;  // [3][nb]: the multi-held buckets by route
    u64 N = 0;
    {
        StageTimer t(c, ST_DIR);
        nr.bv = Buf<u64>(c->pool, nwords);
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        hipLaunchKernelGGL(k_many_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, (const ManyOp*)ops.get(), n, op, nr.bv.get(), popc.get());
        nr.nb = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
        if (nr.nb == 0) { CBLX_HIP(hipStreamSynchronize(c->stream)); return Resident(); }  // (intersect of indexes that share no prefix)
        const u64 nb = nr.nb;
        alloc_dir_rows(c, nr);
        cap = Buf<u32>(c->pool, nb + 1);
        hmask = Buf<u64>(c->pool, nb + 1);
        lists = Buf<BDesc>(c->pool, 3 * nb);
        CBLX_HIP(hipMemsetAsync(list_n.get(), 0, 3 * 4, c->stream));
        hipLaunchKernelGGL(k_many_table, grid1(nprefix, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nprefix, (const u64*)nr.bv.get(), (const u64*)nr.rank_dir.get(),
                           (const ManyOp*)ops.get(), n, op, nb, nr.prefix.get(), hmask.get(), cap.get(), nr.cnt.get(), nr.kind.get(), lists.get(), list_n.get());
        N = seal_runs<WS>(c, nr, cap.get());
    }
    const u64 nb = nr.nb;
    if (op == SETOP_OR) {
        StageTimer t(c, ST_EXPAND);
        with_lpb(N, nb, [&](auto lpb) {
            constexpr int LPB = decltype(lpb)::value;
            hipLaunchKernelGGL((k_many_gather<WS, LPB>), lpb_grid(nb, LPB), dim3(256), 0, c->stream, nb, (const u64*)nr.start.get(), (const u32*)nr.prefix.get(), (const u64*)hmask.get(),
                               (const ManyOp*)ops.get(), nr.a_lo.get(), nr.a_hi.get());
        });
        CBLX_HIP(hipGetLastError());
    }
    const std::vector<u32> ln = d2h_vec<u32>(c, list_n.get(), 3);
    if (ln[0] || ln[1] || ln[2]) sort_many_sides<C>(c, xs, ops.get(), nb, nr.prefix.get(), hmask.get(), op);
    if (ln[0] || ln[1]) {
        StageTimer t(c, ST_BBIG);
        with_setop(op, [&](auto opc) {
            constexpr u32 OP = decltype(opc)::value;
            if constexpr (OP == SETOP_OR || OP == SETOP_AND) {  // (the only n-ary operations)
            if (ln[0])
                hipLaunchKernelGGL((k_bucket_setop_many<WS, OP, MANY_SMALL, 64>), dim3(ln[0]), dim3(64), 0, c->stream, (const BDesc*)lists.get(), (const u32*)list_n.get(),
                                   (const u32*)nr.prefix.get(), (const u64*)hmask.get(), (const ManyOp*)ops.get(), (const u64*)nr.start.get(), nr.a_lo.get(), nr.a_hi.get(), P.SB,
                                   nr.cnt.get());
            if (ln[1])
                hipLaunchKernelGGL((k_bucket_setop_many<WS, OP, MANY_LDS, 256>), dim3(ln[1]), dim3(256), 0, c->stream, (const BDesc*)lists.get() + nb, (const u32*)list_n.get() + 1,
                                   (const u32*)nr.prefix.get(), (const u64*)hmask.get(), (const ManyOp*)ops.get(), (const u64*)nr.start.get(), nr.a_lo.get(), nr.a_hi.get(), P.SB,
                                   nr.cnt.get());
            }
        });
        CBLX_HIP(hipGetLastError());
    }
    if (ln[2]) {
        // the long route: correct at any length, not fast — one k_bucket_setop launch per operand over the long buckets it holds
        StageTimer t(c, ST_BBIG);
        const u32 nl = ln[2];
        const BDesc* ll = lists.get() + 2 * nb;
        Buf<u32> words(c->pool, nl), acc_cnt(c->pool, nl), t_cs(c->pool, nl), t_co(c->pool, nl), step_n(c->pool, 1);
        Buf<u64> sc_start(c->pool, nl + 1), t_sstart(c->pool, nl), t_ostart(c->pool, nl), t_run(c->pool, nl);
        Buf<u8> acc_side(c->pool, nl);
        Buf<BDesc> step_list(c->pool, nl);
        hipLaunchKernelGGL(k_many_long_words, grid1(nl, 256), dim3(256), 0, c->stream, ll, nl, words.get());
        const u64 S = exclusive_scan<u64>(c, words.get(), nl, sc_start.get());
        Buf<u64> sc_lo(c->pool, 2 * S + 2), sc_hi(c->pool, WS ? 2 * S + 2 : 1);
        hipLaunchKernelGGL((k_many_long_init<WS>), dim3(nl), dim3(256), 0, c->stream, ll, nl, (const u32*)nr.prefix.get(), (const u64*)hmask.get(), (const ManyOp*)ops.get(),
                           (const u64*)sc_start.get(), sc_lo.get(), sc_hi.get(), P.SB, acc_cnt.get(), acc_side.get());
        for (u32 i = 0; i < n; ++i) {
            CBLX_HIP(hipMemsetAsync(step_n.get(), 0, 4, c->stream));
            hipLaunchKernelGGL(k_many_long_plan, grid1(nl, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, ll, nl, (const u32*)nr.prefix.get(), (const u64*)hmask.get(),
                               (const ManyOp*)ops.get(), i, op, (const u64*)sc_start.get(), S, (const u32*)acc_cnt.get(), acc_side.get(), t_cs.get(), t_co.get(), t_sstart.get(),
                               t_ostart.get(), t_run.get(), step_list.get(), step_n.get());
            with_setop(op, [&](auto opc) {
                constexpr u32 OP = decltype(opc)::value;
                hipLaunchKernelGGL((k_bucket_setop<WS, OP>), dim3(nl), dim3(UNI_THREADS), 0, c->stream, (const BDesc*)step_list.get(), (const u32*)step_n.get(), (const u32*)t_cs.get(),
                                   (const u32*)t_co.get(), (const u64*)t_sstart.get(), (const u64*)t_ostart.get(), (const u64*)sc_lo.get(), (const u64*)sc_hi.get(),
                                   (const u64*)xs[i]->a_lo.get(), (const u64*)xs[i]->a_hi.get(), (const u64*)t_run.get(), sc_lo.get(), sc_hi.get(), P.SB, acc_cnt.get(), (u8*)nullptr);
            });
        }
        hipLaunchKernelGGL((k_many_long_finish<WS>), dim3(nl), dim3(256), 0, c->stream, ll, nl, (const u64*)sc_start.get(), S, (const u64*)sc_lo.get(), (const u64*)sc_hi.get(),
                           (const u32*)acc_cnt.get(), (const u8*)acc_side.get(), (const u64*)nr.start.get(), (const u32*)cap.get(), nr.a_lo.get(), nr.a_hi.get(), nr.cnt.get());
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the scratch runs die here
    }
    if (!set_op_tail(c, nr, popc, nwords, N)) return Resident();
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the lists and tables of this call die here
    return nr;
}
template <typename C> void set_op_many_direct(cblx_ctx* c, const std::vector<Resident*>& xs, u32 op) { c->res = set_op_many_build<C>(c, xs, op); }

// ---- k-mers at least t of the n operands hold into a new index, or the occupancy histogram alone (cblx_set_at_least / cblx_occupancy_counts) ----
// `xs`: 2 .. 64 non-empty operands, all resident on this device. hist == null: 2 <= t <= n, the result is returned (t = 1 is set_op_many_build's merge, the
// caller's business). hist given (n + 1 entries): t must be 1 — a merge's visit in a count-only mode: no arena, no output runs, no gather; hist[j] = distinct
// k-mers exactly j operands hold, read back once through the mailbox; the returned index is empty. Either way the Vec buckets of every operand on the visited
// prefixes — m >= max(t, 2) holders — are sorted in its own arena.
template <typename C> Resident at_least_build(cblx_ctx* c, const std::vector<Resident*>& xs, u32 t, u64* hist) {
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    const u32 n = (u32)xs.size();
    const bool count_only = hist != nullptr;
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    if (count_only) for (u32 j = 0; j <= n; ++j) hist[j] = 0;
    std::vector<ManyOp> h_ops(n);
    for (u32 i = 0; i < n; ++i) h_ops[i] = ManyOp{xs[i]->view(), xs[i]->a_lo.get(), xs[i]->a_hi.get()};
    Buf<ManyOp> ops(c->pool, n);
    h2d(c, ops.get(), h_ops.data(), n);
    Resident nr;
    Buf<u32> cap, single, popc(c->pool, nwords), list_n(c->pool, 3);
    Buf<u64> hmask;
    Buf<BDesc> lists;  // [3][nb]: the visited multi-held buckets by route
    u64 N = 0;
    {
        StageTimer tm(c, ST_DIR);
        nr.bv = Buf<u64>(c->pool, nwords);
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        hipLaunchKernelGGL(k_thresh_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, (const ManyOp*)ops.get(), n, t, nr.bv.get(), popc.get());
        nr.nb = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
        if (nr.nb == 0) { CBLX_HIP(hipStreamSynchronize(c->stream)); return Resident(); }  // no prefix has t holders
        const u64 nb = nr.nb;
        if (count_only) { nr.prefix = Buf<u32>(c->pool, nb + 1); single = Buf<u32>(c->pool, nb + 1); }
        else { alloc_dir_rows(c, nr); cap = Buf<u32>(c->pool, nb + 1); }
        hmask = Buf<u64>(c->pool, nb + 1);
        lists = Buf<BDesc>(c->pool, 3 * nb);
        CBLX_HIP(hipMemsetAsync(list_n.get(), 0, 3 * 4, c->stream));
        hipLaunchKernelGGL(k_thresh_table, grid1(nprefix, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nprefix, (const u64*)nr.bv.get(), (const u64*)nr.rank_dir.get(),
                           (const ManyOp*)ops.get(), n, t, nb, nr.prefix.get(), hmask.get(), cap.get(), nr.cnt.get(), nr.kind.get(), lists.get(), list_n.get(), single.get());
        CBLX_HIP(hipGetLastError());
        if (!count_only) N = seal_runs<WS>(c, nr, cap.get());
    }
    const u64 nb = nr.nb;
    const std::vector<u32> ln = d2h_vec<u32>(c, list_n.get(), 3);
    if (ln[0] || ln[1] || ln[2]) sort_many_sides<C>(c, xs, ops.get(), nb, nr.prefix.get(), hmask.get(), t >= 2 ? SETOP_AND : SETOP_OR);  // visited: m >= max(t, 2)
    // counting: a grid of a few residencies of the chip, one row of tallies per workgroup
    const u32 g0 = count_only ? std::min<u32>(ln[0], 1u << 14) : ln[0], g1 = count_only ? std::min<u32>(ln[1], 1u << 13) : ln[1], g2 = count_only ? std::min<u32>(ln[2], 1u << 12) : ln[2];
    Buf<u64> tally;
    if (count_only) tally = Buf<u64>(c->pool, (size_t)(g0 + g1 + g2 + 1) * (MANY_MAX + 1));
    auto with_mode = [&](auto&& f) { if (count_only) f(std::true_type()); else f(std::false_type()); };
    if (ln[0] || ln[1]) {
        StageTimer tm(c, ST_BBIG);
        with_mode([&](auto mode) {
            constexpr bool COUNT = decltype(mode)::value;
            if (ln[0])
                hipLaunchKernelGGL((k_bucket_atleast<WS, MANY_SMALL, 64, COUNT>), dim3(g0), dim3(64), 0, c->stream, (const BDesc*)lists.get(), (const u32*)list_n.get(),
                                   (const u32*)nr.prefix.get(), (const u64*)hmask.get(), (const ManyOp*)ops.get(), (const u64*)nr.start.get(), (const u32*)cap.get(), nr.a_lo.get(),
                                   nr.a_hi.get(), P.SB, nr.cnt.get(), t, tally.get());
            if (ln[1])
                hipLaunchKernelGGL((k_bucket_atleast<WS, MANY_LDS, 256, COUNT>), dim3(g1), dim3(256), 0, c->stream, (const BDesc*)lists.get() + nb, (const u32*)list_n.get() + 1,
                                   (const u32*)nr.prefix.get(), (const u64*)hmask.get(), (const ManyOp*)ops.get(), (const u64*)nr.start.get(), (const u32*)cap.get(), nr.a_lo.get(),
                                   nr.a_hi.get(), P.SB, nr.cnt.get(), t, tally.get() + (size_t)g0 * (MANY_MAX + 1));
        });
        CBLX_HIP(hipGetLastError());
    }
    if (ln[2]) {
        StageTimer tm(c, ST_BHUGE);
        const u32 nl = ln[2];
        const BDesc* ll = lists.get() + 2 * nb;
        with_mode([&](auto mode) {
            constexpr bool COUNT = decltype(mode)::value;
            hipLaunchKernelGGL((k_bucket_atleast_long<WS, COUNT>), dim3(g2), dim3(256), 0, c->stream, ll, nl, (const u32*)nr.prefix.get(), (const u64*)hmask.get(),
                               (const ManyOp*)ops.get(), (const u64*)nr.start.get(), (const u32*)cap.get(), nr.a_lo.get(), nr.a_hi.get(), P.SB,
                               nr.cnt.get(), t, tally.get() + (size_t)(g0 + g1) * (MANY_MAX + 1));
        });
        CBLX_HIP(hipGetLastError());
    }
    if (count_only) {
        StageTimer tm(c, ST_COMMON);
        Buf<u64> partial(c->pool, COMMON_SUM_GROUPS), total(c->pool, 1), d_hist(c->pool, MANY_MAX + 1);
        const u32 ng = (u32)std::min<u64>(COMMON_SUM_GROUPS, ceil_div(nb, 256));
        hipLaunchKernelGGL(k_common_sum<u32>, dim3(ng), dim3(256), 0, c->stream, (const u32*)single.get(), nb, partial.get());
        hipLaunchKernelGGL(k_common_sum<u64>, dim3(1), dim3(256), 0, c->stream, (const u64*)partial.get(), (u64)ng, total.get());
        hipLaunchKernelGGL(k_tally_sum, dim3(MANY_MAX + 1), dim3(256), 0, c->stream, (const u64*)tally.get(), g0 + g1 + g2, (const u64*)total.get(), d_hist.get());
        CBLX_HIP(hipGetLastError());
        ReadGroup rg(c);
        const size_t h = rg.add(d_hist.get(), MANY_MAX + 1);
        rg.wait();  // the tables and lists of this call die here
        for (u32 j = 0; j <= n; ++j) hist[j] = rg.get<u64>(h, j);
        return Resident();
    }
    if (!set_op_tail(c, nr, popc, nwords, N)) return Resident();
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the lists and tables of this call die here
    return nr;
}

template <typename C> void set_op_direct(cblx_ctx* c, Resident& a, Resident& b, u32 op) { c->res = set_op_build<C>(c, a, b, op, false); }
// `a OP= &mut b` for AND / SUB / XOR, a = c->res: built beside a from a and b, then moved into a, as merge_direct does for `|=`
template <typename C> void set_op_assign_direct(cblx_ctx* c, Resident& b, u32 op) {
    Resident nr = set_op_build<C>(c, c->res, b, op, true);
    c->res = std::move(nr);
}

// ---- |a AND b| of two resident indexes on this device, and nothing else (cblx_intersection_count) ----------------------------------
// The candidates are a.bv & b.bv with their popcount scan, as set_op_build finds AND's; k_merge_table gives both sides' (count, kind, start) per candidate,
// k_common_plan the four route lists, the four kernels one u32 per candidate, two sum passes the total. The scratch is sized by the candidate BUCKETS, never
// by words, and neither operand is written: no Vec is sorted, no kind changes. The total and the four list lengths come back in one read (the kernels walk
// their lists by *list_n on the device). `c` is a's context: its stream, pool and mailbox; b's stream is idle (the caller's business).
// stats (COMMON_ROUTES + 1 entries, or null): candidates, then the buckets of every route in common_route's order.
template <typename C> u64 intersection_count(cblx_ctx* c, const Resident& a, const Resident& b, u64* stats) {
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    StageTimer t(c, ST_COMMON);
    Buf<u64> bv(c->pool, nwords), rank_dir(c->pool, nwords + 1);
    Buf<u32> popc(c->pool, nwords);
    hipLaunchKernelGGL(k_setop_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, a.bv.get(), b.bv.get(), SETOP_AND, bv.get(), popc.get());
    const u64 nb = exclusive_scan<u64>(c, popc.get(), nwords, rank_dir.get());
    if (nb == 0) { CBLX_HIP(hipStreamSynchronize(c->stream)); return 0; }  // no prefix is held by both
    Buf<u32> prefix(c->pool, nb + 1), raw(c->pool, nb + 1), m_cs(c->pool, nb + 1), m_co(c->pool, nb + 1), common(c->pool, nb), list_n(c->pool, COMMON_ROUTES);
    Buf<u64> m_sstart(c->pool, nb + 1), m_ostart(c->pool, nb + 1), partial(c->pool, COMMON_SUM_GROUPS), total(c->pool, 1);
    Buf<u8> m_skind(c->pool, nb + 1), m_okind(c->pool, nb + 1);
    Buf<BDesc> lists(c->pool, (size_t)COMMON_ROUTES * nb);
    CBLX_HIP(hipMemsetAsync(list_n.get(), 0, COMMON_ROUTES * 4, c->stream));
    CBLX_HIP(hipMemsetAsync(common.get(), 0, nb * 4, c->stream));
    hipLaunchKernelGGL(k_merge_table, grid1(nprefix, 256), dim3(256), 0, c->stream, nprefix, bv.get(), rank_dir.get(), a.view(), b.view(), prefix.get(), raw.get(), m_cs.get(),
                       m_sstart.get(), m_ostart.get(), m_skind.get(), m_okind.get());
    hipLaunchKernelGGL(k_common_plan, grid1(nb, CLASSIFY_THREADS), dim3(CLASSIFY_THREADS), 0, c->stream, nb, (const u32*)raw.get(), (const u32*)m_cs.get(), m_co.get(),
                       (const u8*)m_skind.get(), (const u8*)m_okind.get(), lists.get(), list_n.get());
    CBLX_HIP(hipGetLastError());
    // a grid no larger than a few residencies of the chip: a workgroup takes the buckets blockIdx.x, + gridDim.x, ... of its list
    auto args = [&](int route) {
        return CommonArgs{lists.get() + (size_t)route * nb, list_n.get() + route, m_cs.get(), m_co.get(), m_sstart.get(), m_ostart.get(), a.a_lo.get(), a.a_hi.get(),
                          b.a_lo.get(), b.a_hi.get(), P.SB, common.get()};
    };
    auto groups = [&](u64 most) { return dim3((unsigned)std::min<u64>(nb, most)); };
    hipLaunchKernelGGL((k_common_wave<WS>), groups(1u << 16), dim3(64), 0, c->stream, args(COMMON_WAVE));
    hipLaunchKernelGGL((k_common_lds<WS>), groups(1u << 14), dim3(COMMON_THREADS), 0, c->stream, args(COMMON_WG));
    hipLaunchKernelGGL((k_common_merge<WS>), groups(1u << 14), dim3(UNI_THREADS), 0, c->stream, args(COMMON_MERGE));
    hipLaunchKernelGGL((k_common_sliced<WS>), groups(1u << 14), dim3(COMMON_THREADS), 0, c->stream, args(COMMON_SLICED));
    CBLX_HIP(hipGetLastError());
    const u32 ng = (u32)std::min<u64>(COMMON_SUM_GROUPS, ceil_div(nb, 256));
    hipLaunchKernelGGL(k_common_sum<u32>, dim3(ng), dim3(256), 0, c->stream, (const u32*)common.get(), nb, partial.get());
    hipLaunchKernelGGL(k_common_sum<u64>, dim3(1), dim3(256), 0, c->stream, (const u64*)partial.get(), (u64)ng, total.get());
    CBLX_HIP(hipGetLastError());
    ReadGroup rg(c);
    const size_t h_tot = rg.add(total.get()), h_ln = rg.add(list_n.get(), COMMON_ROUTES);
    rg.wait();  // the tables and lists of this call die here
    if (stats) {
        stats[0] = nb;
        for (int k = 0; k < COMMON_ROUTES; ++k) stats[1 + k] = rg.get<u32>(h_ln, k);
    }
    return rg.get<u64>(h_tot);
}
// |a AND b| of two flushed contexts on one device; a == b and an empty operand are answered without a kernel (stats: all zero)
u64 intersection_count_ctx(cblx_ctx* a, cblx_ctx* b, u64* stats) {
    if (stats) for (int k = 0; k <= COMMON_ROUTES; ++k) stats[k] = 0;
    if (a == b) return a->res.count;
    if (a->res.count == 0 || b->res.count == 0) return 0;
    CBLX_HIP(hipStreamSynchronize(b->stream));
    u64 n = 0;
    dispatch(a->P, [&](auto cfg) { n = intersection_count<decltype(cfg)>(a, a->res, b->res, stats); });
    collect_events(a);
    return n;
}

// ---- WordSet::remove_batch (src/wordset/mod.rs:218-237) over n device words ------------------------------------------------
// `gstart` (n + 1 counters): 1 where a word starts a remove_batch call (a chunk of get_seq_words), 0 elsewhere; k_rm_visit adds the prefix changes, or every
// word with `every` (n successive CBL::remove calls). d_was: CBL::remove's return value per word (n bytes, or null). The result is built beside the resident
// index — k_bucket_remove writes what is left of the visited buckets, a scan of the new lengths gives the runs of a compacted arena, k_rm_gather fills it from
// the replay's output and from the old runs of the other buckets — and moved in at the end, so an error leaves the index as it was.
template <typename C> void remove_words(cblx_ctx* c, const u64* w_lo, const typename C::HiT* w_hi, u64 n, Buf<u32>& gstart, bool every, u8* d_was) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    if (d_was && n) CBLX_HIP(hipMemsetAsync(d_was, 0, n, c->stream));
    if (n == 0 || c->res.nb == 0) { CBLX_HIP(hipStreamSynchronize(c->stream)); return; }
    if (n >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "a single removal batch takes fewer than 2^32-16 words");
    const Resident& s = c->res;
    const u64 nb = s.nb, nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    const u64* s_hi = WS ? s.a_hi.get() : (const u64*)nullptr;
    Buf<u32> wrank(c->pool, n + 1), gbefore(c->pool, n + 1), visited(c->pool, nb + 1), cap(c->pool, nb + 1), mingroup(c->pool, nb + 1);
    Buf<u64> voff(c->pool, nb + 2);
    Buf<u32> too_long(c->pool, 1);
    u64 V = 0;
    {
        StageTimer t(c, ST_DIR);
        CBLX_HIP(hipMemsetAsync(visited.get(), 0, (nb + 1) * 4, c->stream));
        CBLX_HIP(hipMemsetAsync(mingroup.get(), 0xFF, (nb + 1) * 4, c->stream));
        CBLX_HIP(hipMemsetAsync(too_long.get(), 0, 4, c->stream));
        hipLaunchKernelGGL(k_rm_visit<HiT>, grid1(n, 256), dim3(256), 0, c->stream, w_lo, w_hi, n, P.SB, P.PB, s.view(), every ? 1u : 0u, gstart.get(), wrank.get(), visited.get());
        exclusive_scan<u32>(c, gstart.get(), n, gbefore.get());
        hipLaunchKernelGGL(k_rm_caps, grid1(nb, 256), dim3(256), 0, c->stream, nb, (const u32*)visited.get(), (const u32*)s.cnt.get(), cap.get(), too_long.get());
        V = exclusive_scan<u64>(c, cap.get(), nb, voff.get());
        if (d2h<u32>(c, too_long.get())) throw Error(CBLX_ERANGE, "removal from a bucket of more than 2^31 words is not supported");
        hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, voff.get() + nb, V);
        CBLX_HIP(hipGetLastError());
    }
    if (V == 0) { CBLX_HIP(hipStreamSynchronize(c->stream)); return; }  // no word of the batch names a prefix of the index
    u64 H = 64;
    while (H < 2 * V) H <<= 1;
    Buf<u64> table(c->pool, H), wslot;
    Buf<u32> first(c->pool, V + 1), lists(c->pool, 3 * nb), list_n(c->pool, 3);
    if (d_was) wslot = Buf<u64>(c->pool, n + 1);
    Resident nr;
    nr.nb = nb;
    auto dup = [&](auto& d, const auto& o) {
        typedef typename std::remove_reference<decltype(*o.get())>::type T;
        if (!o.get()) return;
        d = Buf<T>(c->pool, o.n);
        device_copy(c->stream, d.get(), o.get(), o.n * sizeof(T));
    };
    dup(nr.bv, s.bv); dup(nr.rank_dir, s.rank_dir); dup(nr.prefix, s.prefix); dup(nr.cnt, s.cnt); dup(nr.kind, s.kind);  // buckets the batch does not visit keep length and kind
    nr.start = Buf<u64>(c->pool, nb + 1);
    Buf<u64> x_lo(c->pool, V + 1), x_hi(c->pool, WS ? V + 1 : 1);  // what the replay leaves of the visited buckets, at their table slots
    Buf<u8> moved(c->pool, nb + 1);
    CBLX_HIP(hipMemsetAsync(moved.get(), 0, nb + 1, c->stream));
    std::vector<u32> ln;
    {
        StageTimer t(c, ST_REMOVE);
        CBLX_HIP(hipMemsetAsync(table.get(), 0xFF, H * 8, c->stream));
        CBLX_HIP(hipMemsetAsync(first.get(), 0xFF, (V + 1) * 4, c->stream));
        CBLX_HIP(hipMemsetAsync(list_n.get(), 0, 3 * 4, c->stream));
        const u64 step = 1ull << 31;
        for (u64 v0 = 0; v0 < V; v0 += step)
            hipLaunchKernelGGL(k_rm_build, grid1(std::min(step, V - v0), 256), dim3(256), 0, c->stream, v0, V, nb, (const u64*)voff.get(), (const u32*)s.cnt.get(), (const u64*)s.start.get(),
                               (const u64*)s.a_lo.get(), s_hi, P.SB, table.get(), H - 1);
        hipLaunchKernelGGL(k_rm_probe<HiT>, grid1(n, 256), dim3(256), 0, c->stream, w_lo, w_hi, n, P.SB, (const u32*)wrank.get(), (const u32*)gstart.get(), (const u32*)gbefore.get(),
                           (const u64*)voff.get(), (const u64*)s.start.get(), (const u64*)s.a_lo.get(), s_hi, (const u64*)table.get(), H - 1, first.get(), mingroup.get(), wslot.get());
        if (d_was) hipLaunchKernelGGL(k_rm_flags, grid1(n, 256), dim3(256), 0, c->stream, n, (const u64*)wslot.get(), (const u32*)first.get(), d_was);
        hipLaunchKernelGGL(k_rm_classify, grid1(nb, 256), dim3(256), 0, c->stream, nb, (const u32*)cap.get(), lists.get(), list_n.get());
        CBLX_HIP(hipGetLastError());
        ln = d2h_vec<u32>(c, list_n.get(), 3);
        Buf<u64> g_keys;
        Buf<u32> g_pos, g_elem;
        if (ln[2]) { g_keys = Buf<u64>(c->pool, V + 1); g_pos = Buf<u32>(c->pool, V + 1); g_elem = Buf<u32>(c->pool, V + 1); }
        auto go = [&](auto thr, auto lds, int cls) {
            constexpr int T = decltype(thr)::value, CAPV = decltype(lds)::value;
            if (!ln[cls]) return;
            hipLaunchKernelGGL((k_bucket_remove<WS, T, CAPV>), dim3(ln[cls]), dim3(T), 0, c->stream, (const u32*)(lists.get() + (size_t)cls * nb), (const u32*)(list_n.get() + cls),
                               (const u64*)s.start.get(), (const u32*)s.cnt.get(), (const u8*)s.kind.get(), (const u64*)voff.get(), (const u32*)first.get(), (const u32*)gstart.get(),
                               (const u32*)gbefore.get(), (const u32*)mingroup.get(), (const u64*)s.a_lo.get(), s_hi, x_lo.get(), x_hi.get(), nr.cnt.get(), nr.kind.get(), moved.get(),
                               g_keys.get(), g_pos.get(), g_elem.get());
        };
        go(std::integral_constant<int, 64>(), std::integral_constant<int, (int)RM_SMALL>(), 0);
        go(std::integral_constant<int, 256>(), std::integral_constant<int, (int)RM_LDS>(), 1);
        go(std::integral_constant<int, 256>(), std::integral_constant<int, 0>(), 2);
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the global tables die here
    }
    // the compacted arena: runs as long as the buckets are now
    u64 N = 0;
    {
        StageTimer t(c, ST_EXPAND);
        N = seal_runs<WS>(c, nr, nr.cnt.get());
        with_lpb(N, nb, [&](auto lpb) {
            constexpr int LPB = decltype(lpb)::value;
            hipLaunchKernelGGL((k_rm_gather<WS, LPB>), lpb_grid(nb, LPB), dim3(256), 0, c->stream, nb, (const u64*)nr.start.get(), (const u32*)nr.cnt.get(), (const u8*)moved.get(),
                               (const u64*)voff.get(), (const u64*)s.start.get(), (const u64*)s.a_lo.get(), s_hi, (const u64*)x_lo.get(), (const u64*)x_hi.get(), nr.a_lo.get(),
                               nr.a_hi.get());
        });
        CBLX_HIP(hipGetLastError());
    }
    // emptied buckets leave the directory and the bitvector, the k-mers are counted
    Buf<u32> popc(c->pool, nwords);
    const bool any = set_op_tail(c, nr, popc, nwords, N);
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the tables of this call die here
    c->res = any ? std::move(nr) : Resident();
}

// CBL::remove_seq (src/cbl.rs:343-354) for every sequence of a device-resident batch: KRN-1 as for a query, one remove_batch per chunk
void remove_device_one(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, const u64* ends) {
    dispatch(c->P, [&](auto cfg) {
        typedef decltype(cfg) C;
        typedef typename C::HiT HiT;
        ChunkPlan pl;
        plan_chunks(c, d_bases, d_offsets, nseq, pl, ends);
        const u64 nk = pl.n_kmers;
        if (nk == 0 || c->res.nb == 0) return;
        if (nk >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "one sequence of 2^32-16 k-mers or more is not supported");
        Buf<u64> w_lo(c->pool, nk + 2);
        Buf<u8> w_hi(c->pool, (nk + 2) * std::max<size_t>(1, hi_elem_size(c->P)));
        Buf<u32> gstart(c->pool, nk + 1);
        CBLX_HIP(hipMemsetAsync(gstart.get(), 0, (nk + 1) * 4, c->stream));
        encode<C>(c, d_bases, pl, w_lo.get(), (HiT*)w_hi.get(), 0);
        hipLaunchKernelGGL(k_rm_chunk_marks, grid1(pl.nchunks, 256), dim3(256), 0, c->stream, (const u64*)pl.kmer_off.get(), pl.nchunks, nk, gstart.get());
        CBLX_HIP(hipGetLastError());
        remove_words<C>(c, w_lo.get(), (const HiT*)w_hi.get(), nk, gstart, false, nullptr);
    });
    collect_events(c);
}
// cut into sub-batches at sequence boundaries exactly as insert_device cuts an insert (a sequence boundary is a chunk boundary: same result)
void remove_device(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq) {
    if (nseq == 0) return;
    check_aligned16(d_bases, "d_bases");
    const u64 cap = batch_max_bases();
    const u64 first = d2h<u64>(c, d_offsets), last = d2h<u64>(c, d_offsets + nseq);
    if (offsets_span(first, last) <= cap) {
        const u64 ends[2] = {first, last};
        remove_device_one(c, d_bases, d_offsets, nseq, ends);
        return;
    }
    {   // a sequence shorter than K anywhere in the batch: nothing is removed, as when the batch goes in as one
        Buf<unsigned long long> ml(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(ml.get(), 0xFF, 8, c->stream));
        hipLaunchKernelGGL(k_rm_min_len, grid1(nseq, 256), dim3(256), 0, c->stream, d_offsets, nseq, ml.get());
        CBLX_HIP(hipGetLastError());
        const u64 m = d2h<unsigned long long>(c, ml.get());
        if (m < c->P.K) throw Error(CBLX_ESHORT, "Sequence size (" + std::to_string(m) + ") is smaller than K (" + std::to_string(c->P.K) + ")");
    }
    u64 a = 0, oa = first;
    while (a < nseq) {
        u64 lo = a + 1, hi = nseq;  // largest b in [a + 1, nseq] with offsets[b] - oa <= cap (a + 1 if even one sequence is longer)
        if (d2h<u64>(c, d_offsets + hi) - oa <= cap) lo = hi;
        else {
            while (hi - lo > 1) {
                const u64 mid = lo + (hi - lo) / 2;
                if (d2h<u64>(c, d_offsets + mid) - oa <= cap) lo = mid; else hi = mid;
            }
        }
        remove_device_one(c, d_bases, d_offsets + a, lo - a, nullptr);
        a = lo;
        oa = d2h<u64>(c, d_offsets + a);
    }
}

}  // namespace
