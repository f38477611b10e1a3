// bubbles.hpp — bubble popping on the compacted graph, on the host: the marks of the simple bubbles (bubble_table, bubble_mark,
// bubbles_observe), a round and the rounds of pop_bubbles, and the carry of a caller's counts through a removal (carry_counts). The link table is
// section 6m's (gfa_count, gfa_fill), the coverage section 6p's (kc_of_table); the form follows the index. With counts the array is the caller's device
// array of section 6p: refused when its length is not count(), and rewritten in place behind every removing round.
// Kernels: kernels_bubbles.hpp. Included by cblx.cpp only, behind abundance.hpp.
#pragma once
#include "abundance.hpp"
#include "kernels_bubbles.hpp"

namespace {

// d_counts == null with n_counts == 0 selects the length rule; otherwise section 6p's guard. Pending inserts are applied either way.
bool bubble_counted(cblx_ctx* c, const u32* d_counts, u64 n_counts) {
    if (!d_counts && n_counts) throw Error(CBLX_EINVAL, "null counts with n_counts = " + std::to_string(n_counts));
    if (!d_counts) { flush(c); return false; }
    abundance_require(c, d_counts, n_counts);
    return true;
}

// What a call holds between its steps: per k-mer `unitig`, per unitig `length`, the link table, in the plain form `left`, with counts `kc`.
struct BubbleRun {
    UnitigForm form = UnitigForm::Plain;
    u64 n = 0, n_unitigs = 0, n_links = 0;
    Buf<u32> unitig, length, link_to;
    Buf<u8> link_rev, left;
    Buf<u64> link_start, kc;
};
// (a) The compaction and its link table; in the plain form left[u] from the kept masks. The masks, offsets and `reversed` are back in the pool on return.
// (b) With counts, kc.
void bubble_table(cblx_ctx* c, BubbleRun& b, const u32* d_counts) {
    GfaRun g;
    gfa_count(c, g);
    b.form = g.form; b.n = g.n; b.n_unitigs = g.n_unitigs; b.n_links = g.n_links;
    if (g.n == 0) return;
    const u64 n = g.n, nu = g.n_unitigs, nl = g.n_links;
    if (n >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "the index holds " + std::to_string(n) + " k-mers: bubbles need fewer than 2^32 - 16");
    if (2 * nu >= (1ull << 32)) throw Error(CBLX_ERANGE, "the index holds " + std::to_string(nu) + " unitigs: bubbles need fewer than 2^31");
    b.link_to = Buf<u32>(c->pool, std::max<u64>(nl, 1)); b.link_rev = Buf<u8>(c->pool, std::max<u64>(nl, 1));
    if (nl) {
        CBLX_HIP(hipMemsetAsync(b.link_to.get(), 0xFF, nl * 4, c->stream));  // a link the fill does not write names no unitig
        CBLX_HIP(hipMemsetAsync(b.link_rev.get(), 0, nl, c->stream));
        gfa_fill(c, g, b.link_to.get(), b.link_rev.get());
    }
    if (g.form == UnitigForm::Plain) {
        b.left = Buf<u8>(c->pool, nu);
        hipLaunchKernelGGL(k_bubble_left, grid1(n, 256), dim3(256), 0, c->stream, (const u32*)g.unitig.get(), (const u32*)g.offset.get(), (const u8*)g.masks.get(), n, b.left.get());
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));
    }
    g.masks.reset(); g.offset.reset(); g.reversed.reset();
    b.unitig = std::move(g.unitig); b.length = std::move(g.length); b.link_start = std::move(g.link_start);
    if (d_counts) {
        b.kc = Buf<u64>(c->pool, nu);
        kc_of_table(c, b.unitig.get(), n, d_counts, nu, b.kc.get());
    }
}
// (c) kind (a device array of b.n_unitigs elements, or null) and the three counts: kept arms, popped arms, the k-mers of the popped arms; b.n != 0
void bubble_mark(cblx_ctx* c, const BubbleRun& b, u64 max_kmers, u8* d_kind, u64 counts[3]) {
    const u64 nu = b.n_unitigs;
    const bool bi = b.form == UnitigForm::Bidirected;
    Buf<u64> d_cnt(c->pool, 3);
    CBLX_HIP(hipMemsetAsync(d_cnt.get(), 0, 3 * 8, c->stream));
    if (d_kind) CBLX_HIP(hipMemsetAsync(d_kind, 0, nu, c->stream));
    hipLaunchKernelGGL(k_bubble_mark, grid1(bi ? 2 * nu : nu, 256), dim3(256), 0, c->stream, (const u64*)b.link_start.get(), (const u32*)b.link_to.get(),
                       (const u8*)b.link_rev.get(), (const u32*)b.length.get(), (const u8*)b.left.get(), (const u64*)b.kc.get(), nu, bi, max_kmers, d_kind, d_cnt.get());
    CBLX_HIP(hipGetLastError());
    const std::vector<u64> h = d2h_vec<u64>(c, d_cnt.get(), 3);
    for (int k = 0; k < 3; ++k) counts[k] = h[k];
}
// cblx_bubbles_mark*: the count out, the capacity, then the marks into the caller's device array (`device`) or into a pool array copied back
void bubbles_observe(cblx_ctx* c, bool device, u64 max_kmers, const u32* d_counts, u64 n_counts, u8* kind, u64 cap_unitigs, u64* n_unitigs, u64* counts) {
    if (max_kmers == 0) throw Error(CBLX_EINVAL, "max_kmers must be at least 1");
    const bool counted = bubble_counted(c, d_counts, n_counts);
    BubbleRun b;
    try { bubble_table(c, b, counted ? d_counts : nullptr); } catch (...) { collect_events(c); throw; }
    collect_events(c);
    const u64 nu = b.n_unitigs;
    if (n_unitigs) *n_unitigs = nu;
    if (kind && cap_unitigs < nu) throw Error(CBLX_ERANGE, "output capacity too small: the index holds " + std::to_string(b.n) + " k-mers in " + std::to_string(nu) + " unitigs");
    u64 h[3] = {0, 0, 0};
    if (b.n != 0) {
        Buf<u8> d_k;
        if (!device && kind) d_k = Buf<u8>(c->pool, nu);
        bubble_mark(c, b, max_kmers, device ? kind : d_k.get(), h);
        if (!device && kind) xfer(c).d2h_copy(kind, d_k.get(), nu);
        CBLX_HIP(hipStreamSynchronize(c->stream));
    }
    if (counts) for (int k = 0; k < 3; ++k) counts[k] = h[k];
}

// (f) The carry of a caller's counts through a removal, for any caller that holds the survivors of the removal as packed k-mers in the iteration order of
// before (keep_lo / keep_hi, keep_hi null for K <= 31) with their counts (keep_counts): d_counts[j], j < m, becomes the count of the survivor whose
// ordinal in the index as it is now is j, and elements m .. n_before - 1 become 0. The index must hold exactly the m survivors.
void carry_counts(cblx_ctx* c, const u64* keep_lo, const u64* keep_hi, const u32* keep_counts, u64 m, u32* d_counts, u64 n_before) {
    if (c->res.count != m) throw Error(CBLX_EDEVICE, "the survivors and the index after the removal do not add up (internal error)");
    if (m) {
        Buf<u64> rank(c->pool, m);
        dispatch(c->P, [&](auto cfg) { rank_kmers_device<decltype(cfg)>(c, keep_lo, keep_hi, m, rank.get()); });
        Buf<u32> tmp(c->pool, m), bad(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(bad.get(), 0, 4, c->stream));
        hipLaunchKernelGGL(k_counts_scatter, grid1(m, 256), dim3(256), 0, c->stream, (const u64*)rank.get(), keep_counts, m, tmp.get(), bad.get());
        CBLX_HIP(hipGetLastError());
        if (d2h<u32>(c, bad.get())) throw Error(CBLX_EDEVICE, "a surviving k-mer has no ordinal below the new count (internal error)");
        CBLX_HIP(hipMemcpyAsync(d_counts, tmp.get(), m * 4, hipMemcpyDeviceToDevice, c->stream));
        if (n_before > m) CBLX_HIP(hipMemsetAsync(d_counts + m, 0, (n_before - m) * 4, c->stream));
        CBLX_HIP(hipStreamSynchronize(c->stream));  // tmp dies here
    } else if (n_before) {
        CBLX_HIP(hipMemsetAsync(d_counts, 0, n_before * 4, c->stream));
        CBLX_HIP(hipStreamSynchronize(c->stream));
    }
}

// One round of pop_bubbles: compact, mark, select the k-mers of the popped arms in iteration order, and remove their words as one
// WordSet::remove_batch, exactly as a round of clip_tips; with counts (d_counts != null, of c->res.count elements) the survivors and their counts leave
// in the same export sweep and the array is carried. Returns the selected k-mers (0: nothing was removed, nothing written); counts as in bubble_mark.
// Everything but the batch — and with counts the survivors — is back in the pool before remove_words takes its workspace.
u64 bubble_round(cblx_ctx* c, u64 max_kmers, u32* d_counts, u64 counts[3]) {
    const bool wide = c->P.wide_kmer();
    Buf<u64> s_lo, s_hi, k_lo, k_hi;
    Buf<u32> k_cnt;
    u64 ns = 0, n = 0;
    {
        BubbleRun b;
        bubble_table(c, b, d_counts);
        for (int k = 0; k < 3; ++k) counts[k] = 0;
        if (b.n == 0) return 0;
        n = b.n;
        Buf<u8> kind(c->pool, b.n_unitigs);
        bubble_mark(c, b, max_kmers, kind.get(), counts);
        if (counts[1] == 0) return 0;
        b.link_start.reset(); b.link_to.reset(); b.link_rev.reset(); b.left.reset(); b.kc.reset(); b.length.reset();
        Buf<u32> sel(c->pool, n), pos(c->pool, n);
        hipLaunchKernelGGL(k_bubble_select, grid1(n, 256), dim3(256), 0, c->stream, (const u32*)b.unitig.get(), (const u8*)kind.get(), n, sel.get());
        CBLX_HIP(hipGetLastError());
        ns = exclusive_scan<u32>(c, sel.get(), n, pos.get());
        if (ns != counts[2]) throw Error(CBLX_EDEVICE, "the selected k-mers and the lengths of the popped arms do not add up (internal error)");
        b.unitig.reset(); kind.reset();
        s_lo = Buf<u64>(c->pool, ns + 2);
        if (wide) s_hi = Buf<u64>(c->pool, ns + 2);
        if (d_counts) {
            k_lo = Buf<u64>(c->pool, n - ns + 2);
            if (wide) k_hi = Buf<u64>(c->pool, n - ns + 2);
            k_cnt = Buf<u32>(c->pool, n - ns + 2);
        }
        export_passes(c, 0, n, [&](u64 a, u64 m, const u64* e_lo, const u64* e_hi, const u64*) {
            hipLaunchKernelGGL(k_bubble_gather, grid1(m, 256), dim3(256), 0, c->stream, e_lo, e_hi, a, m, (const u32*)sel.get(), (const u32*)pos.get(), s_lo.get(), s_hi.get(),
                               (const u32*)d_counts, k_lo.get(), k_hi.get(), k_cnt.get());
            CBLX_HIP(hipGetLastError());
        });  // sel / pos die behind its sync
    }
    dispatch(c->P, [&](auto cfg) {
        typedef decltype(cfg) C;
        typedef typename C::HiT HiT;
        Buf<u64> w_lo(c->pool, ns + 2);
        Buf<u8> w_hi(c->pool, (ns + 2) * std::max<size_t>(1, hi_elem_size(c->P)));
        Buf<u32> bad(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(bad.get(), 0, 4, c->stream));
        hipLaunchKernelGGL((k_kmers_to_words<C::WIDE, HiT>), grid1(ns, 256), dim3(256), 0, c->stream, (const u64*)s_lo.get(), (const u64*)s_hi.get(), ns, c->P, w_lo.get(),
                           (HiT*)w_hi.get(), bad.get());
        CBLX_HIP(hipGetLastError());
        if (d2h<u32>(c, bad.get())) throw Error(CBLX_EDEVICE, "an exported k-mer is no IntKmer<K> (internal error)");
        s_lo.reset(); s_hi.reset();
        Buf<u32> gstart(c->pool, ns + 1);
        CBLX_HIP(hipMemsetAsync(gstart.get(), 0, (ns + 1) * 4, c->stream));
        remove_words<C>(c, w_lo.get(), (const HiT*)w_hi.get(), ns, gstart, false, nullptr);  // groups: the maximal runs of equal prefix, one per bucket
    });
    if (d_counts) carry_counts(c, k_lo.get(), k_hi.get(), k_cnt.get(), n - ns, d_counts, n);
    return ns;
}
// stats: rounds, bubbles, popped, popped_kmers, kmers_left, fixpoint (cblx_bubble_stats). max_rounds = 0: until nothing is popped. With counts the array
// has n_counts = count() elements on entry; behind every removing round its first kmers_left elements are the survivors' counts and the rest 0.
void pop_bubbles(cblx_ctx* c, u64 max_kmers, u32* d_counts, u64 n_counts, u32 max_rounds, u64 stats[6]) {
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    const bool counted = bubble_counted(c, d_counts, n_counts);
    for (u32 r = 0;; ++r) {
        u64 counts[3];
        const u64 ns = bubble_round(c, max_kmers, counted ? d_counts : nullptr, counts);
        ++stats[0];
        if (ns == 0) { stats[5] = 1; break; }
        stats[1] += counts[0]; stats[2] += counts[1]; stats[3] += counts[2];
        if (r + 1 == max_rounds) break;
    }
    stats[4] = c->res.count;
}

}  // namespace
