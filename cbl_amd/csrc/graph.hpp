// graph.hpp — the index as a de Bruijn graph, on the host: the checks a batch of packed k-mers goes through, the export of the index pass by pass
// (export_passes), neighbour masks (neighbor_masks_device, neighbor_masks_range), the rank of a k-mer (rank_words,
// rank_kmers_device) and the compaction into unitigs, plain (section 6k) and bidirected (section 6l): unitig_compute, unitig_number, unitig_text,
// unitigs_to_fd; the links between the unitigs with the GFA text of the compacted graph (section 6m): gfa_count, gfa_fill, gfa_text, gfa_to_fd; and tip
// clipping (section 6n): tip_table, tip_ends, tip_mark, clip_tips; and the connected components of the compacted graph with their filter (section 6o):
// component_table, component_filter.
// Kernels: kernels_graph.hpp, kernels_unitig.hpp, kernels_biunitig.hpp, kernels_gfa.hpp, kernels_tips.hpp, kernels_components.hpp. Included by cblx.cpp only.
#pragma once
#include "list.hpp"
#include "kernels_graph.hpp"
#include "kernels_unitig.hpp"
#include "kernels_biunitig.hpp"
#include "kernels_gfa.hpp"
#include "kernels_tips.hpp"
#include "kernels_components.hpp"

namespace {

// ---- packed k-mers from a caller ---------------------------------------------------------------------------------------------------------
// the arrays of a batch: `lo`, the `hi` halves where K >= 33, and `out`, which takes the answer
inline void require_kmer_arrays(const cblx_ctx* c, const void* lo, const void* hi, const void* out) {
    if (!out || !lo || (c->P.wide_kmer() && !hi)) throw Error(CBLX_EINVAL, c->P.wide_kmer() ? "null argument (K >= 33 needs the hi halves of the k-mers)" : "null argument");
}
// every one of n packed k-mers of device arrays (d_hi may be null for K <= 31) is an IntKmer<K>, or the call is refused. `bad`: one zeroed word.
static const char* const NOT_A_KMER = "k-mer has bits set above 2K (not an IntKmer<K>)";
template <typename C> void check_packed_kmers(cblx_ctx* c, const u64* d_lo, const u64* d_hi, u64 n, u32* bad) {
    for (u64 a = 0; a < n; a += 1ull << 31)
        hipLaunchKernelGGL((k_kmers_check<C::WIDE>), grid1(std::min<u64>(1ull << 31, n - a), 256), dim3(256), 0, c->stream, d_lo + a, d_hi ? d_hi + a : d_hi,
                           std::min<u64>(1ull << 31, n - a), c->P, bad);
    CBLX_HIP(hipGetLastError());
    if (d2h<u32>(c, bad)) throw Error(CBLX_EINVAL, NOT_A_KMER);
}

// ---- de Bruijn neighbourhoods (kernels_graph.hpp) ------------------------------------------------------
// k-mers per pass: 8 words and 8 flag bytes of scratch each. CBLX_NEIGHBOR_PASS overrides the default; at most 2^28, so that the 8 x pass
// ordinals of a pass stay below 2^32 - 16 and its lanes fit one grid.
static const u64 NEIGHBOR_PASS_DEFAULT = 1ull << 22, NEIGHBOR_PASS_MAX = 1ull << 28;
u64 neighbor_pass() {  // read per call: tests switch it
    const char* e = std::getenv("CBLX_NEIGHBOR_PASS");
    const u64 p = e ? std::strtoull(e, nullptr, 10) : NEIGHBOR_PASS_DEFAULT;
    return std::min(std::max<u64>(p, 1), NEIGHBOR_PASS_MAX);
}
// Elements [first, first + n) of the iteration order (n != 0, inside the index) in passes of at most neighbor_pass() k-mers: the export path of
// cblx_export_kmers_range_device fills a scratch k-mer array, then body(a, m, k_lo, k_hi, res_off) queues its work on the m k-mers from element
// first + a (k_hi is null for K <= 31; res_off of iteration_offsets). The stream is drained before the scratch goes back to the pool.
template <typename Body> void export_passes(cblx_ctx* c, u64 first, u64 n, Body&& body) {
    const u64 pass = std::min(neighbor_pass(), n);
    const bool wide = c->P.wide_kmer();
    Buf<u64> res_off, k_lo(c->pool, pass), k_hi(c->pool, wide ? pass : 1);
    iteration_offsets(c, res_off);
    for (u64 a = 0; a < n; a += pass) {
        const u64 m = std::min(pass, n - a);
        export_range_launch(c, res_off.get(), first + a, m, k_lo.get(), wide ? k_hi.get() : (u64*)nullptr, nullptr);
        body(a, m, (const u64*)k_lo.get(), wide ? (const u64*)k_hi.get() : (const u64*)nullptr, (const u64*)res_off.get());
    }
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the scratch k-mers, and what the caller held for the passes, die here
}
// d_masks[i] = the neighbour mask of packed k-mer i of device arrays (d_hi may be null for K <= 31) against c's resident index, in passes of at most
// neighbor_pass() k-mers: k_neighbor_words makes the 8 m words of a pass, a flags query answers them — by the join on tagged records where
// query_flags_by_join holds and 8 m >= query_join_min(), by k_contains otherwise and on an empty index — and k_fold_neighbor_flags leaves m bytes.
// `check`: the arrays are a caller's; all of them are checked before the first pass writes a mask (a refusal writes nothing).
template <typename C> void neighbor_masks_device(cblx_ctx* c, const u64* d_lo, const u64* d_hi, u64 n, u8* d_masks, bool check = true) {
    typedef typename C::HiT HiT;
    const Consts& P = c->P;
    if (n == 0) return;
    Buf<u32> bad(c->pool, 1);
    CBLX_HIP(hipMemsetAsync(bad.get(), 0, 4, c->stream));
    if (check) check_packed_kmers<C>(c, d_lo, d_hi, n, bad.get());
    const u64 pass = std::min(neighbor_pass(), n);
    const bool by_join = query_flags_by_join(P) && c->res.count != 0;
    const u64 join_min = query_join_min();
    Buf<u8> flags(c->pool, 8 * pass + 16);
    for (u64 a = 0; a < n; a += pass) {
        const u64 m = std::min(pass, n - a), nw = 8 * m;
        const u64* k_hi = d_hi ? d_hi + a : d_hi;
        if (by_join && nw >= join_min) {
            Records rec;
            begin_tagged_records(c, rec, nw);
            hipLaunchKernelGGL((k_neighbor_words<C::WIDE, HiT, true>), grid1(nw, 256), dim3(256), 0, c->stream, d_lo + a, k_hi, m, P, rec.lo.get(), (u64*)rec.hi.get(), bad.get());
            CBLX_HIP(hipGetLastError());
            CBLX_HIP(hipMemsetAsync(flags.get(), 0, nw, c->stream));
            join_tagged_records<C>(c, rec, nw, Buf<u32>(), flags.get());  // no fused histogram: the partition counts its first pass itself
        } else {
            Buf<u64> w_lo(c->pool, nw + 2);
            Buf<u8> w_hi(c->pool, (nw + 2) * std::max<size_t>(1, hi_elem_size(P)));
            hipLaunchKernelGGL((k_neighbor_words<C::WIDE, HiT, false>), grid1(nw, 256), dim3(256), 0, c->stream, d_lo + a, k_hi, m, P, w_lo.get(), (HiT*)w_hi.get(), bad.get());
            contains_words<C>(c, w_lo.get(), (const HiT*)w_hi.get(), nw, flags.get());
            CBLX_HIP(hipStreamSynchronize(c->stream));  // the words die here
        }
        hipLaunchKernelGGL(k_fold_neighbor_flags, grid1(m, 256), dim3(256), 0, c->stream, (const u64*)flags.get(), m, d_masks + a);
        CBLX_HIP(hipGetLastError());
    }
    if (d2h<u32>(c, bad.get())) throw Error(CBLX_EINVAL, NOT_A_KMER);  // (not after the check, and not on exported k-mers) — also: the flags may go back to the pool
}
// The same for elements [first, first + n) of the iteration order (n != 0, inside the index), pass by pass through the device form. d_masks (n bytes)
// and / or d_table (25 words, zeroed by the caller: k_degree_tally adds every pass's masks) take the result.
void neighbor_masks_range(cblx_ctx* c, u64 first, u64 n, u8* d_masks, u64* d_table) {
    Buf<u8> tmp;
    if (!d_masks) tmp = Buf<u8>(c->pool, std::min(neighbor_pass(), n));
    export_passes(c, first, n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64*) {
        u8* out = d_masks ? d_masks + a : tmp.get();
        dispatch(c->P, [&](auto cfg) { neighbor_masks_device<decltype(cfg)>(c, k_lo, k_hi, m, out, false); });
        if (d_table) {
            hipLaunchKernelGGL(k_degree_tally, dim3((unsigned)std::min<u64>(1024, ceil_div(m, 256))), dim3(256), 0, c->stream, (const u8*)out, m, d_table);
            CBLX_HIP(hipGetLastError());
        }
    });
}

// ---- unitigs (kernels_unitig.hpp, kernels_biunitig.hpp; DESIGN.md sections 6k and 6l) -----------------------------------------------------
// rank[i] = the ordinal of word i in the iteration order, ~0 when the index does not hold it (`res_off` of iteration_offsets)
template <typename C> void rank_words(cblx_ctx* c, const u64* res_off, const u64* w_lo, const typename C::HiT* w_hi, u64 n, u64* d_rank) {
    typedef typename C::HiT HiT;
    const u64 step = 1ull << 28;  // QL lanes per query: 2^31 work items per launch
    for (u64 a = 0; a < n; a += step) {
        const u64 m = std::min(step, n - a);
        hipLaunchKernelGGL(k_rank<HiT>, grid1(m * QL, 256), dim3(256), 0, c->stream, w_lo + a, HiTraits<HiT>::has ? w_hi + a : w_hi, m, c->P.SB, c->P.PB, c->res.view(),
                           c->res.a_lo.get(), c->P.wide_suffix() ? c->res.a_hi.get() : (const u64*)nullptr, res_off, d_rank + a);
    }
    CBLX_HIP(hipGetLastError());
}
// The ranks of n packed k-mers of device arrays (d_hi may be null for K <= 31; n != 0), in passes of RANK_PASS k-mers: the whole batch is checked
// before the first pass writes a rank, then k_kmers_to_words (which canonicalises where the index is canonical) and k_rank.
static const u64 RANK_PASS = 1ull << 24;
template <typename C> void rank_kmers_device(cblx_ctx* c, const u64* d_lo, const u64* d_hi, u64 n, u64* d_rank) {
    typedef typename C::HiT HiT;
    const Consts& P = c->P;
    Buf<u32> bad(c->pool, 1);
    CBLX_HIP(hipMemsetAsync(bad.get(), 0, 4, c->stream));
    check_packed_kmers<C>(c, d_lo, d_hi, n, bad.get());
    const u64 pass = std::min(RANK_PASS, n);
    Buf<u64> res_off, w_lo(c->pool, pass + 2);
    Buf<u8> w_hi(c->pool, (pass + 2) * std::max<size_t>(1, hi_elem_size(P)));
    iteration_offsets(c, res_off);
    for (u64 a = 0; a < n; a += pass) {
        const u64 m = std::min(pass, n - a);
        hipLaunchKernelGGL((k_kmers_to_words<C::WIDE, HiT>), grid1(m, 256), dim3(256), 0, c->stream, d_lo + a, d_hi ? d_hi + a : d_hi, m, P, w_lo.get(), (HiT*)w_hi.get(),
                           bad.get());
        rank_words<C>(c, res_off.get(), w_lo.get(), (const HiT*)w_hi.get(), m, d_rank + a);
    }
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the words die here
}

// The compaction of the resident index in one of two forms. Plain (section 6k): the unitigs of a non-canonical index, over its n k-mers. Bidirected
// (section 6l): those of a canonical index with odd K — the same run on the 2 n oriented k-mers, then the choice of one image of every mirror pair.
// Links, list ranking and the cut of the pure cycles (compute), then numbering into whatever arrays the caller has (number). Ordinals are 32-bit
// inside. Every call recomputes.
enum class UnitigForm { Plain, Bidirected };
struct UnitigRun {
    UnitigForm form = UnitigForm::Plain;
    u64 n = 0, n_unitigs = 0, n_circular = 0;  // n: the stored k-mers; next .. circular hold ids = n (plain) or 2 n (bidirected) elements
    u32 rounds = 0;  // jump rounds, the ones after a cycle cut included
    Buf<u32> next, prev, anc[2], dist[2];
    Buf<u8> circular;
    Buf<u8> masks;  // the n neighbour masks, only where unitig_compute was asked to keep them (section 6m)
    int cur = 0;  // anc[cur] / dist[cur] hold the ranking; the other pair is scratch (the head flags and their scan, in the end)
    u64 ids() const { return form == UnitigForm::Bidirected ? 2 * n : n; }
};
// what a form refuses, before anything is computed (or a file opened)
void unitig_require(const cblx_ctx* c, UnitigForm form) {
    if (form == UnitigForm::Plain) {
        if (c->P.canonical) throw Error(CBLX_EINVAL, "unitigs of a canonical index (bidirected unitigs) are not supported");
        return;
    }
    if (!c->P.canonical) throw Error(CBLX_EINVAL, "bidirected unitigs are those of a canonical index: a non-canonical index has cblx_unitig_table and cblx_unitigs_*");
    if ((c->P.K & 1u) == 0) throw Error(CBLX_EINVAL, "bidirected unitigs need an odd K (a k-mer of even K can be its own reverse complement)");
}
// List ranking over u.prev / u.next, arrays of n ids (the k-mers of section 6k, the oriented k-mers of section 6l): pointer jumping, and the cut of the
// pure cycles when the count of unfinished ids repeats. `counters`: 130 zeroed words — [r] the unfinished ids of round r, [129] the cycles cut.
void unitig_rank(cblx_ctx* c, UnitigRun& u, u64 n, Buf<u64>& counters) {
    const dim3 gn = grid1(n, 256), b256(256);
    hipLaunchKernelGGL(k_unitig_rank_init, gn, b256, 0, c->stream, u.prev.get(), n, u.anc[0].get(), u.dist[0].get());
    u.cur = 0;
    u64 last = ~0ull;
    bool cut = false;
    for (u32 r = 0;; ++r) {
        if (r >= 128) throw Error(CBLX_EDEVICE, "unitig ranking did not end (internal error)");
        const int o = u.cur ^ 1;
        hipLaunchKernelGGL(k_unitig_jump, gn, b256, 0, c->stream, u.anc[u.cur].get(), u.dist[u.cur].get(), n, u.anc[o].get(), u.dist[o].get(), counters.get() + r);
        CBLX_HIP(hipGetLastError());
        u.cur = o;
        ++u.rounds;
        const u64 open = d2h<u64>(c, counters.get() + r);  // the k-mers that were unfinished when the round began
        if (open == 0) break;
        if (open != last) { last = open; continue; }
        // every path is finished: the `open` unfinished k-mers are the members of the pure cycles
        if (cut) throw Error(CBLX_EDEVICE, "unitig ranking stalled after the cycle cut (internal error)");
        cut = true;
        last = ~0ull;
        Buf<u32> lo[2] = {Buf<u32>(c->pool, n), Buf<u32>(c->pool, n)}, ptr[2] = {Buf<u32>(c->pool, n), Buf<u32>(c->pool, n)};
        hipLaunchKernelGGL(k_cycle_init, gn, b256, 0, c->stream, u.anc[u.cur].get(), u.dist[u.cur].get(), u.next.get(), n, lo[0].get(), ptr[0].get());
        int lc = 0;
        for (u64 span = 1; span < open; span <<= 1, lc ^= 1)  // a cycle has at most `open` members
            hipLaunchKernelGGL(k_cycle_min, gn, b256, 0, c->stream, lo[lc].get(), ptr[lc].get(), n, lo[lc ^ 1].get(), ptr[lc ^ 1].get());
        hipLaunchKernelGGL(k_cycle_cut, gn, b256, 0, c->stream, lo[lc].get(), n, u.next.get(), u.prev.get(), u.circular.get(), u.anc[u.cur].get(), u.dist[u.cur].get(),
                           counters.get() + 129);
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // lo / ptr die here
    }
}
// The workspace is six 32-bit arrays and a byte array of `ids` elements — about twice as much for the bidirected form — and the n masks while the links
// are made. In the end the scratch pair holds the flags of the (kept) heads (anc) and their exclusive scan (dist). `keep_masks`: the masks stay in
// u.masks instead of going back to the pool behind the links.
void unitig_compute(cblx_ctx* c, UnitigRun& u, UnitigForm form, bool keep_masks = false) {
    flush(c);
    unitig_require(c, form);
    const bool bi = form == UnitigForm::Bidirected;
    const u64 n = c->res.count;
    if (n >= (bi ? 0x7FFFFFF8ull : 0xFFFFFFF0ull))
        throw Error(CBLX_ERANGE, "the index holds " + std::to_string(n) + " k-mers: " + (bi ? "bidirected unitigs need fewer than 2^31 - 8" : "unitigs need fewer than 2^32 - 16"));
    u.form = form;
    u.n = n;
    if (n == 0) return;
    const u64 ids = u.ids();
    const dim3 gi = grid1(ids, 256), b256(256);
    u.next = Buf<u32>(c->pool, ids); u.prev = Buf<u32>(c->pool, ids);
    u.circular = Buf<u8>(c->pool, ids);
    for (int i = 0; i < 2; ++i) { u.anc[i] = Buf<u32>(c->pool, ids); u.dist[i] = Buf<u32>(c->pool, ids); }
    Buf<u64> counters(c->pool, 130);  // [r] unfinished ids of round r; [129] cycles cut: one per circular unitig, two in the bidirected form
    CBLX_HIP(hipMemsetAsync(u.next.get(), 0xFF, ids * 4, c->stream));
    CBLX_HIP(hipMemsetAsync(u.prev.get(), 0xFF, ids * 4, c->stream));
    CBLX_HIP(hipMemsetAsync(u.circular.get(), 0, ids, c->stream));
    CBLX_HIP(hipMemsetAsync(counters.get(), 0, 130 * 8, c->stream));
    {   // (a) all masks, (b) the links, pass by pass
        Buf<u8> masks(c->pool, n + 8);
        neighbor_masks_range(c, 0, n, masks.get(), nullptr);
        const u64* a_hi = c->P.wide_suffix() ? c->res.a_hi.get() : (const u64*)nullptr;
        export_passes(c, 0, n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64* res_off) {
            dispatch(c->P, [&](auto cfg) {
                typedef decltype(cfg) C;
                const u64 step = 1ull << 27;  // bidirected: 2 QL lanes per k-mer, 2^31 work items per launch
                if (!bi)
                    hipLaunchKernelGGL((k_unitig_links<C::WIDE>), grid1(m * QL, 256), b256, 0, c->stream, k_lo, k_hi, a, m, masks.get(), c->P, c->res.view(), c->res.a_lo.get(), a_hi,
                                       res_off, u.next.get(), u.prev.get());
                else for (u64 b = 0; b < m; b += step) {
                    const u64 mb = std::min(step, m - b);
                    hipLaunchKernelGGL((k_biunitig_links<C::WIDE>), grid1(2 * mb * QL, 256), b256, 0, c->stream, k_lo + b, k_hi ? k_hi + b : k_hi, a + b, mb, masks.get(), c->P,
                                       c->res.view(), c->res.a_lo.get(), a_hi, res_off, u.next.get(), u.prev.get());
                }
            });
            CBLX_HIP(hipGetLastError());
        });  // the masks die behind its sync
        if (keep_masks) u.masks = std::move(masks);
    }
    // (c) pointer jumping; (d) the cycle cut when the count of unfinished ids repeats. Bidirected: a cycle and its mirror are both cut, in front of
    // the same stored k-mer
    unitig_rank(c, u, ids, counters);
    const u64 cuts = d2h<u64>(c, counters.get() + 129);
    if (bi && (cuts & 1)) throw Error(CBLX_EDEVICE, "a cycle of oriented k-mers without its mirror (internal error)");
    u.n_circular = bi ? cuts / 2 : cuts;
    // (e) head flags — bidirected: tails -> kept heads — -> exclusive scan -> unitig numbers, in the scratch pair
    const int o = u.cur ^ 1;
    if (!bi) hipLaunchKernelGGL(k_unitig_heads, gi, b256, 0, c->stream, u.prev.get(), ids, u.anc[o].get());
    else {
        hipLaunchKernelGGL(k_biunitig_tails, gi, b256, 0, c->stream, u.anc[u.cur].get(), u.next.get(), ids, u.anc[o].get());
        hipLaunchKernelGGL(k_biunitig_keep, gi, b256, 0, c->stream, u.prev.get(), u.circular.get(), ids, u.anc[o].get());
    }
    CBLX_HIP(hipGetLastError());
    u.n_unitigs = exclusive_scan<u32>(c, u.anc[o].get(), ids, u.dist[o].get());
}
// per stored k-mer unitig / offset / reversed (bidirected form only), per unitig head / length / flags (device arrays of u.n and u.n_unitigs elements;
// any may be null); u.n != 0
void unitig_number(cblx_ctx* c, const UnitigRun& u, u32* d_unitig, u32* d_offset, u8* d_reversed, u32* d_head, u32* d_length, u8* d_flags) {
    const int o = u.cur ^ 1;
    if (u.form == UnitigForm::Plain)
        hipLaunchKernelGGL(k_unitig_number, grid1(u.n, 256), dim3(256), 0, c->stream, u.anc[u.cur].get(), u.dist[u.cur].get(), u.next.get(), u.dist[o].get(), u.circular.get(), u.n,
                           d_unitig, d_offset, d_head, d_length, d_flags);
    else
        hipLaunchKernelGGL(k_biunitig_number, grid1(u.ids(), 256), dim3(256), 0, c->stream, u.anc[u.cur].get(), u.dist[u.cur].get(), u.next.get(), u.anc[o].get(), u.dist[o].get(),
                           u.circular.get(), u.ids(), d_unitig, d_offset, d_reversed, d_head, d_length, d_flags);
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));
}
void unitig_caps(const UnitigRun& u, bool per_kmer, u64 cap_kmers, bool per_unitig, u64 cap_unitigs) {
    if ((per_kmer && cap_kmers < u.n) || (per_unitig && cap_unitigs < u.n_unitigs))
        throw Error(CBLX_ERANGE, "output capacity too small: the index holds " + std::to_string(u.n) + " k-mers in " + std::to_string(u.n_unitigs) + " unitigs");
}
// The text of all unitigs in device memory: n + U K bytes, lines in unitig order (text.get() is null for an empty index); the same sizes and the
// same layout in both forms.
struct UnitigText {
    Buf<u8> text;
    u64 bytes = 0, n_unitigs = 0;
};
// The letters and the '\n' of every unitig's line, K + length[u] bytes from d_out + base[u] (device arrays of a table; `reversed` is null in the plain form)
void unitig_lines(cblx_ctx* c, u64 n, const u32* unitig, const u32* offset, const u8* reversed, const u32* length, const u64* base, u8* d_out) {
    const u32 K = c->P.K;
    export_passes(c, 0, n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64*) {
        if (!reversed)
            hipLaunchKernelGGL(k_unitig_text, grid1(m, 256), dim3(256), 0, c->stream, k_lo, k_hi, a, m, unitig, offset, length, base, K, d_out);
        else
            hipLaunchKernelGGL(k_biunitig_text, grid1(m, 256), dim3(256), 0, c->stream, k_lo, k_hi, a, m, unitig, offset, reversed, length, base, K, d_out);
        CBLX_HIP(hipGetLastError());
    });  // the caller's arrays may die behind its sync
}
// `d_out`: the caller's buffer, or null: t.text is allocated. fits(need) is called once the need is known: it may refuse (throw), or return false when the
// size is all that is wanted.
template <typename Fits> void unitig_text(cblx_ctx* c, UnitigForm form, UnitigText& t, u8* d_out, Fits&& fits) {
    UnitigRun u;
    unitig_compute(c, u, form);
    const bool bi = form == UnitigForm::Bidirected;
    const u64 n = u.n, nu = u.n_unitigs, K = c->P.K;
    t.n_unitigs = nu;
    t.bytes = n + nu * K;
    if (!fits(t.bytes) || n == 0) return;
    if (!d_out) { t.text = Buf<u8>(c->pool, t.bytes); d_out = t.text.get(); }
    Buf<u32> unitig(c->pool, n), offset(c->pool, n), length(c->pool, nu), line(c->pool, nu);
    Buf<u8> reversed;
    if (bi) reversed = Buf<u8>(c->pool, n);
    Buf<u64> base(c->pool, nu);
    unitig_number(c, u, unitig.get(), offset.get(), reversed.get(), nullptr, length.get(), nullptr);
    u = UnitigRun();  // the ranking's arrays go back to the pool
    hipLaunchKernelGGL(k_unitig_line_bytes, grid1(nu, 256), dim3(256), 0, c->stream, length.get(), nu, (u32)K, line.get());
    CBLX_HIP(hipGetLastError());
    if (exclusive_scan<u64>(c, line.get(), nu, base.get()) != t.bytes) throw Error(CBLX_EDEVICE, "unitig lengths do not add up (internal error)");
    unitig_lines(c, n, unitig.get(), offset.get(), reversed.get(), length.get(), base.get(), d_out);  // the table dies behind its sync
}
// `cbl unitigs`: the text is built once on the device and leaves through the two pinned buffers of the list
void unitigs_to_fd(cblx_ctx* c, UnitigForm form, int fd, u64 chunk_bytes, u64* n_unitigs, u64* bytes) {
    UnitigText t;
    unitig_text(c, form, t, nullptr, [](u64) { return true; });
    if (n_unitigs) *n_unitigs = t.n_unitigs;
    if (bytes) *bytes = t.bytes;
    if (t.bytes == 0) return;
    if (chunk_bytes == 0) chunk_bytes = LIST_CHUNK_DEFAULT * (c->P.K + 1);
    const u64 cbytes = std::min<u64>(chunk_bytes, t.bytes);
    stream_chunks_to_fd(c, fd, t.bytes, cbytes, "unitigs", [&](u64 i, u64) -> const u8* { return t.text.get() + i * cbytes; });
}

// ---- links between unitigs and the GFA text (kernels_gfa.hpp) ----------------------------------------------------------
// The form follows the index. What a call holds between its steps: the table's per-k-mer arrays and lengths, the masks the compaction kept, and
// link_start, the CSR over the 2 U slots (2 U + 1 entries, the last one L).
struct GfaRun {
    UnitigForm form = UnitigForm::Plain;
    u64 n = 0, n_unitigs = 0, n_links = 0;
    Buf<u32> unitig, offset, length;
    Buf<u8> reversed, masks;  // reversed: bidirected form only
    Buf<u64> link_start;
    u64 slots() const { return 2 * n_unitigs; }
};
UnitigForm gfa_form(const cblx_ctx* c) { return c->P.canonical ? UnitigForm::Bidirected : UnitigForm::Plain; }
// The compaction with its masks kept, the table, the links per slot and their scan: the counts and link_start. An empty index: U = L = 0, link_start = {0}.
void gfa_count(cblx_ctx* c, GfaRun& g) {
    UnitigRun u;
    g.form = gfa_form(c);
    unitig_compute(c, u, g.form, true);
    const u64 n = g.n = u.n, nu = g.n_unitigs = u.n_unitigs;
    g.link_start = Buf<u64>(c->pool, 2 * nu + 1);
    if (n == 0) {
        CBLX_HIP(hipMemsetAsync(g.link_start.get(), 0, 8, c->stream));
        CBLX_HIP(hipStreamSynchronize(c->stream));
        return;
    }
    g.unitig = Buf<u32>(c->pool, n); g.offset = Buf<u32>(c->pool, n); g.length = Buf<u32>(c->pool, nu);
    if (g.form == UnitigForm::Bidirected) g.reversed = Buf<u8>(c->pool, n);
    unitig_number(c, u, g.unitig.get(), g.offset.get(), g.reversed.get(), nullptr, g.length.get(), nullptr);
    g.masks = std::move(u.masks);
    u = UnitigRun();  // the ranking's arrays go back to the pool
    Buf<u32> cnt(c->pool, 2 * nu);
    CBLX_HIP(hipMemsetAsync(cnt.get(), 0, 2 * nu * 4, c->stream));
    hipLaunchKernelGGL(k_gfa_link_counts, grid1(n, 256), dim3(256), 0, c->stream, g.unitig.get(), g.offset.get(), g.reversed.get(), g.length.get(), g.masks.get(), n, cnt.get());
    CBLX_HIP(hipGetLastError());
    g.n_links = exclusive_scan<u64>(c, cnt.get(), 2 * nu, g.link_start.get());
    h2d(c, g.link_start.get() + 2 * nu, &g.n_links, 1);
    CBLX_HIP(hipStreamSynchronize(c->stream));  // cnt dies here
}
// link_to / link_rev (device arrays of g.n_links elements; either may be null) over export passes; g.n != 0
void gfa_fill(cblx_ctx* c, const GfaRun& g, u32* d_to, u8* d_rev) {
    const u64* a_hi = c->P.wide_suffix() ? c->res.a_hi.get() : (const u64*)nullptr;
    const bool bi = g.form == UnitigForm::Bidirected;
    export_passes(c, 0, g.n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64* res_off) {
        dispatch(c->P, [&](auto cfg) {
            typedef decltype(cfg) C;
            const u64 step = 1ull << 27;  // bidirected: 2 QL lanes per k-mer, 2^31 work items per launch
            for (u64 b = 0; b < m; b += step) {
                const u64 mb = std::min(step, m - b);
                hipLaunchKernelGGL((k_gfa_link_fill<C::WIDE>), grid1((bi ? 2 : 1) * mb * QL, 256), dim3(256), 0, c->stream, k_lo + b, k_hi ? k_hi + b : k_hi, a + b, mb,
                                   g.masks.get(), g.unitig.get(), g.offset.get(), g.reversed.get(), g.length.get(), c->P, c->res.view(), c->res.a_lo.get(), a_hi, res_off,
                                   g.link_start.get(), d_to, d_rev);
            }
        });
        CBLX_HIP(hipGetLastError());
    });
}
// The GFA text in device memory: the header, the S lines, the L lines of the links that are written (of a mirror pair one). `d_out` and fits(need)
// as in unitig_text; t.n_links = the L lines.
struct GfaText {
    Buf<u8> text;
    u64 bytes = 0, n_unitigs = 0, n_links = 0;
};
// `tags`: what a caller adds to the S lines (abundance.hpp, section 6p). s_bytes(c, g, bytes) fills bytes[u] of its own S lines, or returns false: the plain
// ones. s_tags(c, g, s_base, d_out) is queued behind the letters.
struct GfaNoTags {
    bool s_bytes(cblx_ctx*, const GfaRun&, u32*) { return false; }
    void s_tags(cblx_ctx*, const GfaRun&, const u64*, u8*) {}
};
template <typename Fits, typename Tags = GfaNoTags> void gfa_text(cblx_ctx* c, GfaText& t, u8* d_out, Fits&& fits, Tags&& tags = Tags()) {
    GfaRun g;
    gfa_count(c, g);
    const u64 n = g.n, nu = g.n_unitigs, ns = g.slots(), K = c->P.K;
    const bool bi = g.form == UnitigForm::Bidirected;
    const dim3 b256(256);
    t.n_unitigs = nu;
    Buf<u32> link_to(c->pool, g.n_links + 1), bytes(c->pool, std::max(ns, nu) + 1), lines(c->pool, ns + 1);
    Buf<u8> link_rev(c->pool, g.n_links + 1);
    Buf<u64> s_base(c->pool, nu + 1), l_base(c->pool, ns + 1);
    u64 s_bytes = 0, l_bytes = 0;
    if (n) {
        if (g.n_links) gfa_fill(c, g, link_to.get(), link_rev.get());
        g.masks.reset();
        hipLaunchKernelGGL(k_gfa_l_bytes, grid1(ns, 256), b256, 0, c->stream, (const u64*)g.link_start.get(), (const u32*)link_to.get(), (const u8*)link_rev.get(), ns, bi,
                           (u32)(K - 1), bytes.get(), lines.get());
        CBLX_HIP(hipGetLastError());
        t.n_links = exclusive_scan<u64>(c, lines.get(), ns, l_base.get());
        l_bytes = exclusive_scan<u64>(c, bytes.get(), ns, l_base.get());
        if (!tags.s_bytes(c, g, bytes.get())) hipLaunchKernelGGL(k_gfa_s_bytes, grid1(nu, 256), b256, 0, c->stream, (const u32*)g.length.get(), nu, (u32)K, bytes.get());
        CBLX_HIP(hipGetLastError());
        s_bytes = exclusive_scan<u64>(c, bytes.get(), nu, s_base.get());
    }
    t.bytes = GFA_HEADER_BYTES + s_bytes + l_bytes;
    if (!fits(t.bytes)) return;
    if (!d_out) { t.text = Buf<u8>(c->pool, t.bytes); d_out = t.text.get(); }
    hipLaunchKernelGGL(k_gfa_s_prefix, grid1(nu, 256), b256, 0, c->stream, s_base.get(), nu, (u64)GFA_HEADER_BYTES, d_out);
    if (n) hipLaunchKernelGGL(k_gfa_l_text, grid1(ns, 256), b256, 0, c->stream, (const u64*)g.link_start.get(), (const u32*)link_to.get(), (const u8*)link_rev.get(),
                              (const u64*)l_base.get(), ns, bi, (u32)(K - 1), GFA_HEADER_BYTES + s_bytes, d_out);
    CBLX_HIP(hipGetLastError());
    if (n) unitig_lines(c, n, g.unitig.get(), g.offset.get(), g.reversed.get(), g.length.get(), s_base.get(), d_out);
    if (n) tags.s_tags(c, g, s_base.get(), d_out);
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the tables die here
}
// `cbl unitigs --gfa`: the text is built once on the device and leaves as the unitig text does
void gfa_to_fd(cblx_ctx* c, int fd, u64 chunk_bytes, u64* n_unitigs, u64* n_links, u64* bytes) {
    GfaText t;
    gfa_text(c, t, nullptr, [](u64) { return true; });
    if (n_unitigs) *n_unitigs = t.n_unitigs;
    if (n_links) *n_links = t.n_links;
    if (bytes) *bytes = t.bytes;
    if (chunk_bytes == 0) chunk_bytes = LIST_CHUNK_DEFAULT * (c->P.K + 1);
    const u64 cbytes = std::min<u64>(chunk_bytes, t.bytes);
    stream_chunks_to_fd(c, fd, t.bytes, cbytes, "GFA", [&](u64 i, u64) -> const u8* { return t.text.get() + i * cbytes; });
}

// ---- tip clipping (kernels_tips.hpp) -------------------------------------------------------------------------------------
// The form follows the index, as in section 6m. What a call holds between its steps: per k-mer `unitig`, per unitig `length` and the degrees at its two
// ends; the offsets, `reversed` and the masks the compaction kept only until the ends are made.
struct TipRun {
    UnitigForm form = UnitigForm::Plain;
    u64 n = 0, n_unitigs = 0;
    Buf<u32> unitig, offset, length;
    Buf<u8> reversed, masks, left, right;
};
// The compaction with its masks kept, and the table: the counts. The ranking's arrays are back in the pool on return.
void tip_table(cblx_ctx* c, TipRun& t) {
    UnitigRun u;
    t.form = gfa_form(c);
    unitig_compute(c, u, t.form, true);
    const u64 n = t.n = u.n, nu = t.n_unitigs = u.n_unitigs;
    if (n == 0) return;
    t.unitig = Buf<u32>(c->pool, n); t.offset = Buf<u32>(c->pool, n); t.length = Buf<u32>(c->pool, nu);
    if (t.form == UnitigForm::Bidirected) t.reversed = Buf<u8>(c->pool, n);
    unitig_number(c, u, t.unitig.get(), t.offset.get(), t.reversed.get(), nullptr, t.length.get(), nullptr);
    t.masks = std::move(u.masks);
}
// left / right (device arrays of t.n_unitigs elements; either may be null); t.n != 0. The offsets, `reversed` and the masks go back to the pool.
void tip_ends(cblx_ctx* c, TipRun& t, u8* d_left, u8* d_right) {
    hipLaunchKernelGGL(k_tip_ends, grid1(t.n, 256), dim3(256), 0, c->stream, t.unitig.get(), t.offset.get(), t.reversed.get(), t.length.get(), t.masks.get(), t.n, d_left, d_right);
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));
    t.offset.reset(); t.reversed.reset(); t.masks.reset();
}
// kind (a device array of t.n_unitigs elements, or null) and the four counts: tips, their k-mers, isolated unitigs, their k-mers; t.n != 0. The ends
// are made into t.left / t.right first.
void tip_mark(cblx_ctx* c, TipRun& t, u64 max_kmers, u8* d_kind, u64 counts[4]) {
    const u64 nu = t.n_unitigs;
    t.left = Buf<u8>(c->pool, nu); t.right = Buf<u8>(c->pool, nu);
    tip_ends(c, t, t.left.get(), t.right.get());
    Buf<u64> d_counts(c->pool, 4);
    CBLX_HIP(hipMemsetAsync(d_counts.get(), 0, 4 * 8, c->stream));
    hipLaunchKernelGGL(k_tip_mark, grid1(nu, 256), dim3(256), 0, c->stream, (const u32*)t.length.get(), (const u8*)t.left.get(), (const u8*)t.right.get(), nu, max_kmers, d_kind,
                       d_counts.get());
    CBLX_HIP(hipGetLastError());
    const std::vector<u64> h = d2h_vec<u64>(c, d_counts.get(), 4);
    for (int k = 0; k < 4; ++k) counts[k] = h[k];
}
// One round of clip_tips: compact, mark, select the k-mers of the wanted kinds in iteration order, and remove their words as one WordSet::remove_batch.
// Returns the selected k-mers (0: nothing was removed); counts as in tip_mark. Everything the compaction and the marks held is back in the pool before
// remove_words takes its workspace: only the batch of selected k-mers, then its words, survive.
u64 clip_round(cblx_ctx* c, u64 max_kmers, bool isolated, u64 counts[4]) {
    const bool wide = c->P.wide_kmer();
    Buf<u64> s_lo, s_hi;
    u64 ns = 0;
    {
        TipRun t;
        tip_table(c, t);
        for (int k = 0; k < 4; ++k) counts[k] = 0;
        if (t.n == 0) return 0;
        const u64 n = t.n;
        Buf<u8> kind(c->pool, t.n_unitigs);
        tip_mark(c, t, max_kmers, kind.get(), counts);
        if (counts[0] + (isolated ? counts[2] : 0) == 0) return 0;
        t.left.reset(); t.right.reset(); t.length.reset();
        Buf<u32> sel(c->pool, n), pos(c->pool, n);
        hipLaunchKernelGGL(k_tip_select, grid1(n, 256), dim3(256), 0, c->stream, (const u32*)t.unitig.get(), (const u8*)kind.get(), n,
                           (1u << TIP_TIP) | (isolated ? 1u << TIP_ISOLATED : 0u), sel.get());
        CBLX_HIP(hipGetLastError());
        ns = exclusive_scan<u32>(c, sel.get(), n, pos.get());
        if (ns != counts[1] + (isolated ? counts[3] : 0)) throw Error(CBLX_EDEVICE, "the selected k-mers and the marked lengths do not add up (internal error)");
        t.unitig.reset(); kind.reset();
        s_lo = Buf<u64>(c->pool, ns + 2);
        if (wide) s_hi = Buf<u64>(c->pool, ns + 2);
        export_passes(c, 0, n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64*) {
            hipLaunchKernelGGL(k_tip_gather, grid1(m, 256), dim3(256), 0, c->stream, k_lo, k_hi, a, m, (const u32*)sel.get(), (const u32*)pos.get(), s_lo.get(), s_hi.get());
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
    return ns;
}
// stats: rounds, tips, tip_kmers, isolated, isolated_kmers, kmers_left, fixpoint (cblx_clip_stats). max_rounds = 0: until nothing is selected.
void clip_tips(cblx_ctx* c, u64 max_kmers, bool isolated, u32 max_rounds, u64 stats[7]) {
    for (int k = 0; k < 7; ++k) stats[k] = 0;
    for (u32 r = 0;; ++r) {
        u64 counts[4];
        const u64 ns = clip_round(c, max_kmers, isolated, counts);
        ++stats[0];
        if (ns == 0) { stats[6] = 1; break; }
        stats[1] += counts[0]; stats[2] += counts[1];
        if (isolated) { stats[3] += counts[2]; stats[4] += counts[3]; }
        if (r + 1 == max_rounds) break;
    }
    stats[5] = c->res.count;
}

// ---- connected components (kernels_components.hpp) ---------------------------------------------------------------------------
// The form follows the index, as in section 6m. What a call holds on return: per k-mer `unitig`, per unitig `component`, per component first / unitigs /
// kmers (the k-mer sums on the host too); the link table, the lengths and the labelling's arrays are back in the pool.
struct ComponentRun {
    UnitigForm form = UnitigForm::Plain;
    u64 n = 0, n_unitigs = 0, n_links = 0, n_components = 0, largest_kmers = 0;
    u32 rounds = 0, largest = 0;  // hook rounds, the last one (which hooks nothing) included; the number of the largest component
    Buf<u32> unitig, component, first, unitigs;
    Buf<u64> kmers;
    std::vector<u64> h_kmers;
};
// The link table, the rounds of hook and compress, the numbering and the sizes. An empty index: everything 0, no round.
void component_table(cblx_ctx* c, ComponentRun& r) {
    Buf<u32> length, link_to, par;
    Buf<u64> link_start;
    {
        GfaRun g;
        gfa_count(c, g);
        r.form = g.form;
        r.n = g.n; r.n_unitigs = g.n_unitigs; r.n_links = g.n_links;
        if (g.n == 0) return;
        if (g.n_unitigs >= (1ull << 31)) throw Error(CBLX_ERANGE, "the index has " + std::to_string(g.n_unitigs) + " unitigs: components need fewer than 2^31");
        link_to = Buf<u32>(c->pool, g.n_links + 1);
        if (g.n_links) gfa_fill(c, g, link_to.get(), nullptr);
        r.unitig = std::move(g.unitig); length = std::move(g.length); link_start = std::move(g.link_start);
    }  // the masks, the offsets and `reversed` go back to the pool
    const u64 nu = r.n_unitigs, ns = 2 * nu;
    const dim3 gu = grid1(nu, 256), gs = grid1(ns, 256), b256(256);
    const u32 MAX_ROUNDS = 128, MAX_JUMPS = 33;  // a chain of fewer than 2^31 unitigs is compressed by 31 jumps; one more finds nothing open
    Buf<u32> nxt(c->pool, nu), tmp(c->pool, nu);
    Buf<u64> counters(c->pool, MAX_ROUNDS * (1 + MAX_JUMPS));  // [r] the slots that hooked in round r; behind them one word per jump launch
    CBLX_HIP(hipMemsetAsync(counters.get(), 0, MAX_ROUNDS * (1 + MAX_JUMPS) * 8, c->stream));
    par = Buf<u32>(c->pool, nu);
    hipLaunchKernelGGL(k_cc_init, gu, b256, 0, c->stream, nu, par.get());
    CBLX_HIP(hipGetLastError());
    u64 jumps = 0;
    for (u32 rd = 0;; ++rd) {
        if (rd >= MAX_ROUNDS) throw Error(CBLX_EDEVICE, "component labelling did not end (internal error)");
        CBLX_HIP(hipMemcpyAsync(nxt.get(), par.get(), nu * 4, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_cc_hook, gs, b256, 0, c->stream, (const u64*)link_start.get(), (const u32*)link_to.get(), (const u32*)par.get(), ns, nxt.get(),
                           counters.get() + rd);
        CBLX_HIP(hipGetLastError());
        ++r.rounds;
        if (d2h<u64>(c, counters.get() + rd) == 0) break;  // nothing hooked: nxt == par, and every link joins equal labels
        for (u32 j = 0;; ++j) {
            if (j >= MAX_JUMPS) throw Error(CBLX_EDEVICE, "component compression did not end (internal error)");
            u64* open = counters.get() + MAX_ROUNDS + jumps++;
            hipLaunchKernelGGL(k_cc_jump, gu, b256, 0, c->stream, (const u32*)nxt.get(), nu, tmp.get(), open);
            CBLX_HIP(hipGetLastError());
            std::swap(nxt, tmp);
            if (d2h<u64>(c, open) == 0) break;
        }
        std::swap(par, nxt);
    }
    link_to.reset(); link_start.reset(); tmp.reset();
    // numbering: root flags -> exclusive scan -> component[u], first[c]
    Buf<u32> scan(c->pool, nu);
    hipLaunchKernelGGL(k_cc_roots, gu, b256, 0, c->stream, (const u32*)par.get(), nu, nxt.get());
    CBLX_HIP(hipGetLastError());
    const u64 nc = r.n_components = exclusive_scan<u32>(c, nxt.get(), nu, scan.get());
    if (nc == 0 || nc > nu) throw Error(CBLX_EDEVICE, "the component roots do not add up (internal error)");
    r.component = Buf<u32>(c->pool, nu); r.first = Buf<u32>(c->pool, nc); r.unitigs = Buf<u32>(c->pool, nc); r.kmers = Buf<u64>(c->pool, nc);
    hipLaunchKernelGGL(k_cc_number, gu, b256, 0, c->stream, (const u32*)par.get(), (const u32*)scan.get(), nu, r.component.get(), r.first.get());
    CBLX_HIP(hipMemsetAsync(r.unitigs.get(), 0, nc * 4, c->stream));
    CBLX_HIP(hipMemsetAsync(r.kmers.get(), 0, nc * 8, c->stream));
    hipLaunchKernelGGL(k_cc_sizes, gu, b256, 0, c->stream, (const u32*)r.component.get(), (const u32*)length.get(), nu, r.unitigs.get(), r.kmers.get());
    CBLX_HIP(hipGetLastError());
    r.h_kmers = d2h_vec<u64>(c, r.kmers.get(), nc);  // (the sync: par, scan, nxt and the lengths die here)
    u64 total = 0;
    for (u64 k = 0; k < nc; ++k) {
        total += r.h_kmers[k];
        if (r.h_kmers[k] > r.largest_kmers) { r.largest_kmers = r.h_kmers[k]; r.largest = (u32)k; }  // a tie goes to the lower number
    }
    if (total != r.n) throw Error(CBLX_EDEVICE, "the component sizes do not add up (internal error)");
}
// kmer_component (a device array of r.n elements); r.n != 0
void component_kmers(cblx_ctx* c, const ComponentRun& r, u32* d_kmer_component) {
    hipLaunchKernelGGL(k_cc_kmer, grid1(r.n, 256), dim3(256), 0, c->stream, (const u32*)r.unitig.get(), (const u32*)r.component.get(), r.n, d_kmer_component);
    CBLX_HIP(hipGetLastError());
}
// cblx_components_filter: the table, the keep bytes, the k-mers of the dropped components in iteration order, and their words removed as one
// WordSet::remove_batch. stats: components, removed_components, removed_kmers, kmers_left, largest_kmers (before the removal), rounds
// (cblx_component_stats). `largest`: keep the largest component only (min_kmers is 0 then). Everything the table held is back in the pool before
// remove_words takes its workspace: only the batch of selected k-mers, then its words, survive.
void component_filter(cblx_ctx* c, u64 min_kmers, bool largest, u64 stats[6]) {
    const bool wide = c->P.wide_kmer();
    Buf<u64> s_lo, s_hi;
    u64 ns = 0;
    for (int k = 0; k < 6; ++k) stats[k] = 0;
    {
        ComponentRun r;
        component_table(c, r);
        if (r.n == 0) return;
        const u64 n = r.n, nc = r.n_components;
        stats[0] = nc; stats[3] = n; stats[4] = r.largest_kmers; stats[5] = r.rounds;
        for (u64 k = 0; k < nc; ++k)
            if (largest ? k != r.largest : r.h_kmers[k] < min_kmers) { ++stats[1]; stats[2] += r.h_kmers[k]; }
        if (stats[2] == 0) return;
        r.first.reset(); r.unitigs.reset();
        Buf<u8> keep(c->pool, nc);
        hipLaunchKernelGGL(k_cc_keep, grid1(nc, 256), dim3(256), 0, c->stream, (const u64*)r.kmers.get(), nc, min_kmers, largest ? r.largest : 0xFFFFFFFFu, keep.get());
        Buf<u32> sel(c->pool, n), pos(c->pool, n);
        hipLaunchKernelGGL(k_cc_select, grid1(n, 256), dim3(256), 0, c->stream, (const u32*)r.unitig.get(), (const u32*)r.component.get(), (const u8*)keep.get(), n, sel.get());
        CBLX_HIP(hipGetLastError());
        ns = exclusive_scan<u32>(c, sel.get(), n, pos.get());
        if (ns != stats[2]) throw Error(CBLX_EDEVICE, "the selected k-mers and the component sizes do not add up (internal error)");
        r = ComponentRun();
        keep.reset();
        s_lo = Buf<u64>(c->pool, ns + 2);
        if (wide) s_hi = Buf<u64>(c->pool, ns + 2);
        export_passes(c, 0, n, [&](u64 a, u64 m, const u64* k_lo, const u64* k_hi, const u64*) {
            hipLaunchKernelGGL(k_cc_gather, grid1(m, 256), dim3(256), 0, c->stream, k_lo, k_hi, a, m, (const u32*)sel.get(), (const u32*)pos.get(), s_lo.get(), s_hi.get());
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
    stats[3] = c->res.count;
}

}  // namespace
