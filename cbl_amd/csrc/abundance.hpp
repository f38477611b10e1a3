// abundance.hpp — k-mer abundances from reads, on the host: the tally of a batch of reads into a caller's array of counts
// (abundance_tally), its spectrum (abundance_hist), the coverage of the unitigs (unitig_kc), the GFA text with LN / KC tags (gfa_text_tagged,
// gfa_tagged_to_fd) and the filter (abundance_filter). The counts are the caller's: a device array of one uint32 per stored k-mer, by ordinal; every call
// flushes and then refuses an array whose length is not count().
// Kernels: kernels_abundance.hpp. Included by cblx.cpp only, behind graph.hpp.
#pragma once
#include "graph.hpp"
#include "kernels_abundance.hpp"

namespace {

// the guard against an array from before a change of the index; pending inserts are applied first
void abundance_require(cblx_ctx* c, const u32* d_counts, u64 n_counts) {
    flush(c);
    if (n_counts != c->res.count)
        throw Error(CBLX_EINVAL, "n_counts is " + std::to_string(n_counts) + " but the index holds " + std::to_string(c->res.count) + " k-mers (an array from before a change?)");
    if (n_counts && !d_counts) throw Error(CBLX_EINVAL, "null argument");
}

// ---- the tally ---------------------------------------------------------------------------------------------------------------------------------------
// One run of sequences of at least K bases each (`ends`: its first and last offset where the caller knows them): the front end of the small-batch branch of
// query_device — plan, encode into word buffers — then k_rank_tally in launches of at most 2^28 words. res_off is null for an empty index: nothing is
// encoded. Returns the occurrences of the run.
template <typename C> u64 tally_run(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, const u64* ends, const u64* res_off, u32* d_counts, u64 n_counts,
                                    u64* d_totals) {
    typedef typename C::HiT HiT;
    ChunkPlan pl;
    plan_chunks(c, d_bases, d_offsets, nseq, pl, ends);
    const u64 nk = pl.n_kmers;
    if (nk == 0 || !res_off) return nk;
    if (nk >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "too many k-mers in one abundance batch");
    Buf<u64> w_lo(c->pool, nk + 2);
    Buf<u8> w_hi(c->pool, (nk + 2) * std::max<size_t>(1, hi_elem_size(c->P)));
    encode<C>(c, d_bases, pl, w_lo.get(), (HiT*)w_hi.get(), 0);
    const u64 step = 1ull << 28;  // QL lanes per word: 2^31 work items per launch
    for (u64 a = 0; a < nk; a += step) {
        const u64 m = std::min(step, nk - a);
        hipLaunchKernelGGL(k_rank_tally<HiT>, grid1(m * QL, 256), dim3(256), 0, c->stream, (const u64*)w_lo.get() + a,
                           HiTraits<HiT>::has ? (const HiT*)w_hi.get() + a : (const HiT*)w_hi.get(), m, c->P.SB, c->P.PB, c->res.view(), c->res.a_lo.get(),
                           c->P.wide_suffix() ? c->res.a_hi.get() : (const u64*)nullptr, res_off, d_counts, n_counts, d_totals);
    }
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the words die here
    return nk;
}
// counts[i] += the occurrences of stored k-mer i in the nseq sequences of a device batch, saturating at 2^32 - 1; *total occurrences, *found of them held.
// `h_offsets`: the offsets on the host where the caller has them, else null. The plan refuses a sequence shorter than K, and here such a sequence gives
// no occurrence. A batch with such sequences is compacted once: from the offsets on the host (read back once when the plan refused the whole batch) the
// sequences of at least K bases get new offsets, k_abundance_compact copies their bases side by side, and the compacted batch takes one plan and one tally.
// The cost: the offsets over PCIe (both ways in the device entry), and one copy of the kept bases.
void abundance_tally(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, const u64* h_offsets, u64 nseq, u32* d_counts, u64 n_counts, u64* total, u64* found) {
    if (total) *total = 0;
    if (found) *found = 0;
    abundance_require(c, d_counts, n_counts);
    if (nseq == 0) return;
    if (!d_bases || !d_offsets) throw Error(CBLX_EINVAL, "null argument");
    check_aligned16(d_bases, "d_bases");
    const u64 K = c->P.K;
    Buf<u64> res_off, totals(c->pool, 2);
    CBLX_HIP(hipMemsetAsync(totals.get(), 0, 16, c->stream));
    if (c->res.count) iteration_offsets(c, res_off);
    auto run = [&](const u8* bases, const u64* offsets, u64 ns, const u64* ends) {
        u64 nk = 0;
        dispatch(c->P, [&](auto cfg) { nk = tally_run<decltype(cfg)>(c, bases, offsets, ns, ends, res_off.get(), d_counts, n_counts, totals.get()); });
        return nk;
    };
    u64 tot = 0;
    std::vector<u64> offs;
    bool done = false;
    if (!h_offsets) {
        try { tot = run(d_bases, d_offsets, nseq, nullptr); done = true; }
        catch (const Error& e) {
            if (e.code != CBLX_ESHORT) throw;  // (the plan refuses before anything is encoded: nothing was tallied)
            offs = d2h_vec<u64>(c, d_offsets, nseq + 1);
            h_offsets = offs.data();
        }
    }
    if (!done) {
        u64 kept = 0;
        for (u64 i = 0; i < nseq; ++i) {
            if (h_offsets[i + 1] < h_offsets[i]) throw Error(CBLX_EINVAL, "offsets must be non-decreasing");
            if (h_offsets[i + 1] - h_offsets[i] >= K) ++kept;
        }
        if (kept == nseq) {
            const u64 ends[2] = {h_offsets[0], h_offsets[nseq]};
            tot = run(d_bases, d_offsets, nseq, ends);
        } else if (kept) {
            std::vector<u64> src(kept), dst(kept + 1);
            u64 k = 0, bytes = 0;
            for (u64 i = 0; i < nseq; ++i) {
                const u64 len = h_offsets[i + 1] - h_offsets[i];
                if (len < K) continue;
                src[k] = h_offsets[i]; dst[k] = bytes;
                bytes += len; ++k;
            }
            dst[kept] = bytes;
            Buf<u64> d_src(c->pool, kept), d_dst(c->pool, kept + 1);
            Buf<u8> packed(c->pool, bytes + 64);
            h2d(c, d_src.get(), src.data(), kept);
            h2d(c, d_dst.get(), dst.data(), kept + 1);
            CBLX_HIP(hipMemsetAsync(packed.get() + bytes, 0, 64, c->stream));
            const u64 step = 1ull << 31;
            for (u64 a = 0; a < bytes; a += step)
                hipLaunchKernelGGL(k_abundance_compact, grid1(std::min(step, bytes - a), 256), dim3(256), 0, c->stream, d_bases, (const u64*)d_src.get(), (const u64*)d_dst.get(),
                                   kept, a, std::min(step, bytes - a), packed.get());
            CBLX_HIP(hipGetLastError());
            CBLX_HIP(hipStreamSynchronize(c->stream));  // src / dst were read by then
            const u64 ends[2] = {0, bytes};
            tot = run(packed.get(), d_dst.get(), kept, ends);  // (ends behind a sync: the compacted batch dies here)
        }
    }
    const std::vector<u64> h = d2h_vec<u64>(c, totals.get(), 2);
    if (c->res.count && h[0] != tot) throw Error(CBLX_EDEVICE, "the tallied words and the planned k-mers do not add up (internal error)");
    if (total) *total = tot;
    if (found) *found = h[1];
    collect_events(c);
}

// hist[j] = the ordinals with counts[i] == j (j < 255), hist[255] = those with counts[i] >= 255
void abundance_hist(cblx_ctx* c, const u32* d_counts, u64 n_counts, u64 hist[256]) {
    abundance_require(c, d_counts, n_counts);
    Buf<u64> d_hist(c->pool, 256);
    CBLX_HIP(hipMemsetAsync(d_hist.get(), 0, 256 * 8, c->stream));
    const u64 step = 1ull << 31;
    for (u64 a = 0; a < n_counts; a += step) {
        const u64 m = std::min(step, n_counts - a);
        hipLaunchKernelGGL(k_abundance_hist, grid1(m, 256), dim3(256), 0, c->stream, d_counts + a, m, d_hist.get());
    }
    CBLX_HIP(hipGetLastError());
    const std::vector<u64> h = d2h_vec<u64>(c, d_hist.get(), 256);
    for (int j = 0; j < 256; ++j) hist[j] = h[j];
}

// ---- unitig coverage ------------------------------------------------------------------------------------------------------------------------------------
// d_kc[u] = the sum of counts[i] over the k-mers of unitig u of a table's `unitig` array (nu words, zeroed here); asynchronous on the stream
void kc_of_table(cblx_ctx* c, const u32* unitig, u64 n, const u32* d_counts, u64 nu, u64* d_kc) {
    CBLX_HIP(hipMemsetAsync(d_kc, 0, nu * 8, c->stream));
    hipLaunchKernelGGL(k_unitig_kc, grid1(n, 256), dim3(256), 0, c->stream, unitig, d_counts, n, nu, d_kc);
    CBLX_HIP(hipGetLastError());
}
// The form follows the index, as in section 6m. The compaction and of its table `unitig` and `length` only; the ranking's arrays are back in the pool on
// return. The counts are checked before anything is computed, the form's refusal comes from unitig_compute.
struct CoverageRun {
    UnitigForm form = UnitigForm::Plain;
    u64 n = 0, n_unitigs = 0;
    Buf<u32> unitig, length;
};
void coverage_table(cblx_ctx* c, CoverageRun& r, const u32* d_counts, u64 n_counts) {
    abundance_require(c, d_counts, n_counts);
    UnitigRun u;
    r.form = gfa_form(c);
    unitig_compute(c, u, r.form);
    r.n = u.n; r.n_unitigs = u.n_unitigs;
    if (u.n == 0) return;
    r.unitig = Buf<u32>(c->pool, u.n); r.length = Buf<u32>(c->pool, u.n_unitigs);
    unitig_number(c, u, r.unitig.get(), nullptr, nullptr, nullptr, r.length.get(), nullptr);
}
// cblx_unitig_coverage*: the count out, the capacity, then kc into the caller's device array (`device`) or into a pool array copied back
void unitig_kc(cblx_ctx* c, bool device, const u32* d_counts, u64 n_counts, u64* kc, u64 cap_unitigs, u64* n_unitigs) {
    CoverageRun r;
    coverage_table(c, r, d_counts, n_counts);
    collect_events(c);
    const u64 nu = r.n_unitigs;
    if (n_unitigs) *n_unitigs = nu;
    if (kc && cap_unitigs < nu) throw Error(CBLX_ERANGE, "output capacity too small: the index holds " + std::to_string(r.n) + " k-mers in " + std::to_string(nu) + " unitigs");
    if (!kc || r.n == 0) return;
    Buf<u64> d_kc;
    if (!device) d_kc = Buf<u64>(c->pool, nu);
    kc_of_table(c, r.unitig.get(), r.n, d_counts, nu, device ? kc : d_kc.get());
    CBLX_HIP(hipStreamSynchronize(c->stream));  // (the copy below runs on the transfer lanes' own streams)
    if (!device) xfer(c).d2h_copy(kc, d_kc.get(), nu * 8);
}

// ---- the GFA text with tags -------------------------------------------------------------------------------------------------------------------------------
// gfa_text with the S lines of section 6p: the bytes of a line count its tags, and k_gfa_s_tags runs behind the text kernels, whose '\n' behind the letters it
// replaces by the tab of the first tag. d_counts null: LN only.
struct GfaTags {
    const u32* d_counts = nullptr;
    Buf<u64> kc;  // lives until gfa_text's last sync
    bool s_bytes(cblx_ctx* c, const GfaRun& g, u32* bytes) {
        const u64 nu = g.n_unitigs;
        if (d_counts) {
            kc = Buf<u64>(c->pool, nu);
            kc_of_table(c, g.unitig.get(), g.n, d_counts, nu, kc.get());
        }
        hipLaunchKernelGGL(k_gfa_s_bytes_tagged, grid1(nu, 256), dim3(256), 0, c->stream, (const u32*)g.length.get(), (const u64*)kc.get(), nu, (u32)c->P.K, bytes);
        CBLX_HIP(hipGetLastError());
        return true;
    }
    void s_tags(cblx_ctx* c, const GfaRun& g, const u64* s_base, u8* d_out) {
        hipLaunchKernelGGL(k_gfa_s_tags, grid1(g.n_unitigs, 256), dim3(256), 0, c->stream, (const u32*)g.length.get(), (const u64*)kc.get(), s_base, g.n_unitigs, (u32)c->P.K,
                           d_out);
        CBLX_HIP(hipGetLastError());
    }
};
template <typename Fits> void gfa_text_tagged(cblx_ctx* c, GfaText& t, const u32* d_counts, u64 n_counts, u8* d_out, Fits&& fits) {
    if (d_counts) abundance_require(c, d_counts, n_counts);
    GfaTags tags;
    tags.d_counts = d_counts;
    gfa_text(c, t, d_out, fits, tags);
}
void gfa_tagged_to_fd(cblx_ctx* c, const u32* d_counts, u64 n_counts, int fd, u64 chunk_bytes, u64* n_unitigs, u64* n_links, u64* bytes) {
    GfaText t;
    gfa_text_tagged(c, t, d_counts, n_counts, nullptr, [](u64) { return true; });
    if (n_unitigs) *n_unitigs = t.n_unitigs;
    if (n_links) *n_links = t.n_links;
    if (bytes) *bytes = t.bytes;
    if (chunk_bytes == 0) chunk_bytes = LIST_CHUNK_DEFAULT * (c->P.K + 1);
    const u64 cbytes = std::min<u64>(chunk_bytes, t.bytes);
    stream_chunks_to_fd(c, fd, t.bytes, cbytes, "GFA", [&](u64 i, u64) -> const u8* { return t.text.get() + i * cbytes; });
}

// ---- the filter ---------------------------------------------------------------------------------------------------------------------------------------------
// cblx_abundance_filter: the selection under either rule, the selected k-mers in iteration order, and their words removed as one WordSet::remove_batch, exactly
// as a round of clip_tips. stats: kmers, removed_kmers, unitigs, removed_unitigs, kmers_left, min_count (cblx_abundance_stats); an empty index leaves all
// six 0. Everything but the batch of selected k-mers is back in the pool before remove_words takes its workspace. The counts are read, never written.
void abundance_filter(cblx_ctx* c, const u32* d_counts, u64 n_counts, u32 min_count, bool unitigs, u64 stats[6]) {
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    abundance_require(c, d_counts, n_counts);
    if (unitigs) unitig_require(c, gfa_form(c));  // the form's refusal, before anything changes
    const u64 n = c->res.count;
    if (n == 0) return;
    if (n >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "the index holds " + std::to_string(n) + " k-mers: the abundance filter needs fewer than 2^32 - 16");
    stats[0] = stats[4] = n;
    stats[5] = min_count;
    const bool wide = c->P.wide_kmer();
    Buf<u64> s_lo, s_hi;
    u64 ns = 0;
    {
        CoverageRun r;
        Buf<u64> kc;
        u64 gone[2] = {0, 0};  // the unitigs that go and their k-mers
        if (unitigs) {
            coverage_table(c, r, d_counts, n_counts);
            const u64 nu = stats[2] = r.n_unitigs;
            kc = Buf<u64>(c->pool, nu);
            kc_of_table(c, r.unitig.get(), n, d_counts, nu, kc.get());
            Buf<u64> d_gone(c->pool, 2);
            CBLX_HIP(hipMemsetAsync(d_gone.get(), 0, 16, c->stream));
            hipLaunchKernelGGL(k_abundance_unitig_stats, grid1(nu, 256), dim3(256), 0, c->stream, (const u64*)kc.get(), (const u32*)r.length.get(), nu, min_count, d_gone.get());
            CBLX_HIP(hipGetLastError());
            const std::vector<u64> h = d2h_vec<u64>(c, d_gone.get(), 2);
            gone[0] = h[0]; gone[1] = h[1];
            if (gone[1] == 0) return;
        }
        Buf<u32> sel(c->pool, n), pos(c->pool, n);
        hipLaunchKernelGGL(k_abundance_select, grid1(n, 256), dim3(256), 0, c->stream, d_counts, n, min_count, (const u32*)r.unitig.get(), (const u64*)kc.get(),
                           (const u32*)r.length.get(), sel.get());
        CBLX_HIP(hipGetLastError());
        ns = exclusive_scan<u32>(c, sel.get(), n, pos.get());
        if (unitigs && ns != gone[1]) throw Error(CBLX_EDEVICE, "the selected k-mers and the lengths of the selected unitigs do not add up (internal error)");
        if (ns == 0) return;
        stats[3] = gone[0];
        r = CoverageRun(); kc.reset();
        s_lo = Buf<u64>(c->pool, ns + 2);
        if (wide) s_hi = Buf<u64>(c->pool, ns + 2);
        export_passes(c, 0, n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64*) {
            hipLaunchKernelGGL(k_abundance_gather, grid1(m, 256), dim3(256), 0, c->stream, k_lo, k_hi, a, m, (const u32*)sel.get(), (const u32*)pos.get(), s_lo.get(), s_hi.get());
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
    stats[1] = ns;
    stats[4] = c->res.count;
}

}  // namespace
