// query.hpp — the query side on the host: membership flags of device words (contains_words), the join of a big query batch with the resident index through
// pipeline.hpp's front end and partition (query_join, the tagged records that keep their positions), per-sequence tallies, query_device, and a batch against a
// panel of indexes (panel_join, query_panel_device). Kernels: kernels_kmer.hpp, k_contains in kernels_bucket.hpp. Included by cblx.cpp only.
#pragma once
#include "pipeline.hpp"

namespace {

// membership flags of n device words against the resident index (WordSet::contains_batch)
// (`res`: the index asked, on c's stream — c's own, or another operand's of a panel query)
template <typename C> void contains_words(cblx_ctx* c, const Resident& res, const u64* w_lo, const typename C::HiT* w_hi, u64 n, u8* d_out) {
    typedef typename C::HiT HiT;
    const u64 step = 1ull << 28;  // QL lanes per query: 2^31 work items per launch
    for (u64 a = 0; a < n; a += step) {
        const u64 m = std::min(step, n - a);
        hipLaunchKernelGGL(k_contains<HiT>, grid1(m * QL, 256), dim3(256), 0, c->stream, w_lo + a, HiTraits<HiT>::has ? w_hi + a : w_hi, m, c->P.SB, c->P.PB, res.view(),
                           res.a_lo.get(), c->P.wide_suffix() ? res.a_hi.get() : (const u64*)nullptr, d_out + a);
    }
    CBLX_HIP(hipGetLastError());
}
template <typename C> void contains_words(cblx_ctx* c, const u64* w_lo, const typename C::HiT* w_hi, u64 n, u8* d_out) {
    contains_words<C>(c, c->res, w_lo, w_hi, n, d_out);
}
// Tallies of a big query batch by join (k_query_join): KRN-1 + the stable partition of the query words + one workgroup per
// prefix run. CBLX_QUERY_JOIN_MIN overrides the batch size (k-mers) from which it replaces the per-query kernel.
u64 query_join_min() {  // read per call: tests switch it
    const char* e = std::getenv("CBLX_QUERY_JOIN_MIN");
    return e ? std::strtoull(e, nullptr, 10) : (u64)(4u << 20);
}
// as insert_device: KRN-1 accumulates the first partition pass's tile histogram (countsA: zero-filled here, it goes to the partition)
inline EncHist query_hist(cblx_ctx* c, u64 nk, Buf<u32>& countsA) {
    const Consts& P = c->P;
    EncHist eh{};
    const size_t ntmax = (size_t)ceil_div(nk, RDX_TILE) + 256;
    countsA = Buf<u32>(c->pool, 256 * ntmax);
    CBLX_HIP(hipMemsetAsync(countsA.get(), 0, 256 * ntmax * 4, c->stream));
    const u32 nA = std::min(8u, P.PB);
    eh.counts = countsA.get();
    eh.shift = P.SB + (P.PB - nA);
    eh.nbits = nA;
    return eh;
}
// Queries that keep their positions (words of at most 96 bits, narrow suffix): 16-byte records (lo, ordinal << 32 | hi bits) through the
// partition of the 64-bit-hi layout. rec.lo / rec.hi end up as the partitioned records, qd as the batch's directory (prefixes, run starts).
// the four buffers of nk tagged records (rec.hi / hi2 hold 64-bit hi parts)
inline void begin_tagged_records(cblx_ctx* c, Records& rec, u64 nk) {
    rec.lo = Buf<u64>(c->pool, nk + 2);
    rec.lo2 = Buf<u64>(c->pool, nk + 2);
    rec.hi = Buf<u8>(c->pool, (nk + 2) * 8);
    rec.hi2 = Buf<u8>(c->pool, (nk + 2) * 8);
}
// nk tagged records in rec.lo / rec.hi, already encoded (by KRN-1 + k_query_tag, or by k_neighbor_words), through the partition. `countsA`: the first pass's
// tile histogram where the encoder accumulated it (KRN-1), empty where it did not: the partition then counts it itself.
template <typename C> void partition_tagged(cblx_ctx* c, Records& rec, u64 nk, Buf<u32>&& countsA, Resident& qd) {
    typedef Cfg<C::WIDE, u64, false> QC;
    partition_and_directory<QC>(c, rec, nk, std::move(countsA), qd);
}
template <typename C> void query_partition_tagged(cblx_ctx* c, const u8* d_bases, const ChunkPlan& pl, Buf<u32>&& countsA, const EncHist& eh, Records& rec, Resident& qd) {
    typedef typename C::HiT HiT;
    const Consts& P = c->P;
    const u64 nk = pl.n_kmers;
    begin_tagged_records(c, rec, nk);
    {
        Buf<u8> hi_tmp(c->pool, (nk + 2) * std::max<size_t>(1, hi_elem_size(P)));
        encode<C>(c, d_bases, pl, rec.lo.get(), (HiT*)hi_tmp.get(), 0, eh);
        hipLaunchKernelGGL(k_query_tag<HiT>, grid1(nk, 256), dim3(256), 0, c->stream, nk, (const HiT*)hi_tmp.get(), (u64*)rec.hi.get());
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // hi_tmp dies here
    }
    partition_tagged<C>(c, rec, nk, std::move(countsA), qd);
}
// One workgroup per prefix run of the partitioned query records (rec, directory qd) against c's resident index: pos[0] (device, zeroed by the caller) += the
// queries found; `flags` (zero-filled, or null) takes flag 1 at the ordinal of every query found — tagged records, H = u64, only.
template <typename C, typename H> void join_runs(cblx_ctx* c, const Records& rec, const Resident& qd, u8* flags, u64* pos) {
    const Consts& P = c->P;
    const u64 step = 1ull << 23;  // workgroups per launch (x 256 threads < 2^32 work items)
    Buf<u32> per_run(c->pool, qd.nb + 1);
    CBLX_HIP(hipMemsetAsync(per_run.get(), 0, (qd.nb + 1) * 4, c->stream));
    for (u64 b0 = 0; b0 < qd.nb; b0 += step)
        hipLaunchKernelGGL((k_query_join<C::WS, H>), dim3((unsigned)std::min(step, qd.nb - b0)), dim3(JOIN_THREADS), 0, c->stream, qd.nb, b0, qd.prefix.get(),
                           qd.start.get(), rec.lo.get(), (const H*)rec.hi.get(), P.SB, c->res.view(), c->res.a_lo.get(),
                           P.wide_suffix() ? c->res.a_hi.get() : (const u64*)nullptr, per_run.get(), flags);
    hipLaunchKernelGGL(k_sum_u32, dim3((unsigned)std::min<u64>(2048, std::max<u64>(1, ceil_div(qd.nb, 256)))), dim3(256), 0, c->stream, per_run.get(), qd.nb, pos);
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));  // per_run dies here
}
// The flag join on records that are already encoded and tagged (rec.lo / rec.hi of begin_tagged_records, ordinals 0 .. nk - 1 in the upper halves): partition,
// then one workgroup per run. d_flags: nk bytes, zero-filled by the caller; returns the number of records found. Narrow suffixes only (query_flags_by_join).
template <typename C> u64 join_tagged_records(cblx_ctx* c, Records& rec, u64 nk, Buf<u32>&& countsA, u8* d_flags) {
    if constexpr (!C::WS) {
        Resident qd;  // directory of the query batch: prefixes and run starts
        Buf<u64> pos(c->pool, 1);
        CBLX_HIP(hipMemsetAsync(pos.get(), 0, 8, c->stream));
        partition_tagged<C>(c, rec, nk, std::move(countsA), qd);
        join_runs<C, u64>(c, rec, qd, d_flags, pos.get());
        return d2h<u64>(c, pos.get());  // also: the temporaries may go back to the pool
    } else {
        throw Error(CBLX_EDEVICE, "flag join of a wide suffix (internal error)");
    }
}
template <typename C> u64 query_join(cblx_ctx* c, const u8* d_bases /* as left by plan_chunks */, const ChunkPlan& pl, u8* d_flags /* nk bytes or null */) {
    typedef typename C::HiT HiT;
    const u64 nk = pl.n_kmers;
    if (d_flags && nk) CBLX_HIP(hipMemsetAsync(d_flags, 0, nk, c->stream));
    if (nk == 0 || c->res.count == 0) return 0;
    Buf<u32> countsA;
    const EncHist eh = query_hist(c, nk, countsA);
    Records rec;
    Resident qd;  // directory of the query batch: prefixes and run starts
    Buf<u64> pos(c->pool, 1);
    CBLX_HIP(hipMemsetAsync(pos.get(), 0, 8, c->stream));
    if constexpr (!C::WS) {
        if (d_flags) {
            query_partition_tagged<C>(c, d_bases, pl, std::move(countsA), eh, rec, qd);
            join_runs<C, u64>(c, rec, qd, d_flags, pos.get());
            return d2h<u64>(c, pos.get());
        }
    }
    begin_records<C>(c, rec, nk);
    encode<C>(c, d_bases, pl, rec.lo.get(), (HiT*)rec.hi.get(), 0, eh);
    partition_and_directory<C>(c, rec, nk, std::move(countsA), qd);
    join_runs<C, HiT>(c, rec, qd, (u8*)nullptr, pos.get());
    return d2h<u64>(c, pos.get());  // also: the temporaries may go back to the pool
}
// words whose hi part leaves 32 bits for the query's ordinal, and whose suffix fits 64 bits: flags can come from the join
inline bool query_flags_by_join(const Consts& P) { return !P.wide_suffix() && P.WB <= 96; }
// Per-sequence tallies from the flags of a planned batch (kernels_kmer.hpp): seq_total[s] / seq_pos[s] for every sequence of the plan
// (pl.seq_chunk kept). The flags stay on the device.
void seq_tallies(cblx_ctx* c, const ChunkPlan& pl, u64 nseq, const u8* d_flags, u32* d_seq_total, u32* d_seq_pos) {
    Buf<u32> chunk_pos(c->pool, pl.nchunks + 1);
    const u32 long_cap = (u32)std::min<u64>(nseq, pl.nchunks / (SEQ_TALLY_LANE_MAX + 1) + 1);  // sequences of more than SEQ_TALLY_LANE_MAX chunks
    Buf<u32> long_list(c->pool, long_cap), long_n(c->pool, 1);
    CBLX_HIP(hipMemsetAsync(long_n.get(), 0, 4, c->stream));
    if (d_seq_pos)
        for (u64 c0 = 0; c0 < pl.nchunks; c0 += 1ull << 25)  // one wave per chunk, fewer than 2^32 work items per launch
            hipLaunchKernelGGL(k_chunk_tally, grid1(std::min<u64>(1ull << 25, pl.nchunks - c0) * 64, 256), dim3(256), 0, c->stream, d_flags, (const u64*)pl.kmer_off.get(), c0,
                               pl.nchunks, chunk_pos.get());
    hipLaunchKernelGGL(k_seq_tally, grid1(nseq, 256), dim3(256), 0, c->stream, (const u64*)pl.seq_chunk.get(), (const u64*)pl.kmer_off.get(), (const u32*)chunk_pos.get(), nseq,
                       d_seq_total, d_seq_pos, long_list.get(), long_n.get(), long_cap);
    if (d_seq_pos && pl.nchunks > SEQ_TALLY_LANE_MAX)  // else no sequence is long
        hipLaunchKernelGGL(k_seq_tally_long, dim3(long_cap), dim3(SEQ_TALLY_LONG_THREADS), 0, c->stream, (const u32*)long_list.get(), (const u32*)long_n.get(),
                           (const u64*)pl.seq_chunk.get(), (const u32*)chunk_pos.get(), d_seq_pos);
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));  // chunk_pos and the list die here
}
// CBL::contains_seq over a batch of device-resident sequences: KRN-1, then one membership flag per k-mer (sequence after
// sequence, each in get_seq_words order) into d_out[cap] when given; *total / *positive count the flags.
// d_seq_total / d_seq_pos (device, nseq entries each, either may be null): k-mers queried and k-mers found of every sequence. They are
// tallied on the device from the flags, which then go to scratch unless d_out takes them: by the join with ordinals where
// query_flags_by_join holds and the batch is big enough, by k_contains otherwise — the routes of a query with d_out.
void query_device(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, u8* d_out, u64 cap, u64* total, u64* positive, u32* d_seq_total = nullptr,
                  u32* d_seq_pos = nullptr) {
    if (total) *total = 0;
    if (positive) *positive = 0;
    if (nseq == 0) return;
    check_aligned16(d_bases, "d_bases");
    const bool per_seq = d_seq_total || d_seq_pos;
    dispatch(c->P, [&](auto cfg) {
        typedef decltype(cfg) C;
        typedef typename C::HiT HiT;
        ChunkPlan pl;
        pl.keep_seq_chunk = per_seq;
        plan_chunks(c, d_bases, d_offsets, nseq, pl);
        const u64 nk = pl.n_kmers;
        if (total) *total = nk;
        if (nk == 0) {  // (not with nseq > 0 today: every chunk holds at least its first k-mer)
            if (d_seq_total) CBLX_HIP(hipMemsetAsync(d_seq_total, 0, nseq * 4, c->stream));
            if (d_seq_pos) CBLX_HIP(hipMemsetAsync(d_seq_pos, 0, nseq * 4, c->stream));
            return;
        }
        if (nk >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "too many k-mers in one query batch");
        if (d_out && nk > cap) throw Error(CBLX_ERANGE, "output capacity too small: " + std::to_string(nk) + " k-mers");
        Buf<u8> flags;
        if (d_seq_pos && !d_out) { flags = Buf<u8>(c->pool, nk + 16); d_out = flags.get(); }
        if (nk >= query_join_min() && (!d_out || query_flags_by_join(c->P))) {  // big batch: join instead of one bucket read per query
            const u64 p = query_join<C>(c, d_bases, pl, d_out);
            if (positive) *positive = p;
        } else {
            Buf<u64> w_lo(c->pool, nk + 2);
            Buf<u8> w_hi(c->pool, (nk + 2) * std::max<size_t>(1, hi_elem_size(c->P)));
            if (!d_out) { flags = Buf<u8>(c->pool, nk + 8); d_out = flags.get(); }
            Buf<u32> zeros(c->pool, 1);
            CBLX_HIP(hipMemsetAsync(zeros.get(), 0, 4, c->stream));
            encode<C>(c, d_bases, pl, w_lo.get(), (HiT*)w_hi.get(), 0);
            contains_words<C>(c, w_lo.get(), (const HiT*)w_hi.get(), nk, d_out);
            hipLaunchKernelGGL(k_count_zero_u8, dim3((unsigned)std::min<u64>(4096, ceil_div(nk, 256))), dim3(256), 0, c->stream, (const u8*)d_out, nk, zeros.get());
            CBLX_HIP(hipGetLastError());
            const u64 z = d2h<u32>(c, zeros.get());  // also: the temporaries may go back to the pool
            if (positive) *positive = nk - z;
        }
        if (per_seq) seq_tallies(c, pl, nseq, d_out, d_seq_total, d_seq_pos);
    });
    collect_events(c);
}

// ---- a batch against a PANEL of indexes (cblx_contains_seqs_counts_many*) ---------------------------------------------------
// The panel join: plan, KRN-1, ordinal tags and the partition of the query words run ONCE (query_join's flag branch); k_panel_join then takes every
// query run through its bucket in each index. d_mask: nk words, zero-filled. srcs[j] with an empty index keeps its place (bit j stays 0).
template <typename C> void panel_join(cblx_ctx* c, cblx_ctx* const* srcs, u32 n, const u8* d_bases, const ChunkPlan& pl, u64* d_mask) {
    if constexpr (!C::WS) {
        const Consts& P = c->P;
        const u64 nk = pl.n_kmers;
        Buf<u32> countsA;
        const EncHist eh = query_hist(c, nk, countsA);
        Records rec;
        Resident qd;
        query_partition_tagged<C>(c, d_bases, pl, std::move(countsA), eh, rec, qd);
        std::vector<PanelEntry> h(n);
        for (u32 j = 0; j < n; ++j) {
            const Resident& r = srcs[j]->res;
            h[j] = r.count ? PanelEntry{r.view(), r.a_lo.get(), (const u64*)nullptr} : PanelEntry{DirView{nullptr, nullptr, nullptr, nullptr, nullptr, 0}, nullptr, nullptr};
        }
        Buf<PanelEntry> d_panel(c->pool, n);
        h2d(c, d_panel.get(), h.data(), n);
        const u64 step = 1ull << 23;  // workgroups per launch (x 256 threads < 2^32 work items)
        for (u64 b0 = 0; b0 < qd.nb; b0 += step)
            hipLaunchKernelGGL(k_panel_join, dim3((unsigned)std::min(step, qd.nb - b0)), dim3(JOIN_THREADS), 0, c->stream, qd.nb, b0, (const u32*)qd.prefix.get(),
                               (const u64*)qd.start.get(), (const u64*)rec.lo.get(), (const u64*)rec.hi.get(), P.SB, (const PanelEntry*)d_panel.get(), n, d_mask);
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the records, the directory and the panel table die here (h was read by then)
    } else {
        throw Error(CBLX_EDEVICE, "panel join of a wide suffix (internal error)");
    }
}
// The two tally levels from masks (kernels_kmer.hpp): d_seq_pos[j * nseq + s] for every index j and sequence s of the plan (pl.seq_chunk kept).
void mask_tallies(cblx_ctx* c, const ChunkPlan& pl, u64 nseq, u32 n, const u64* d_mask, u32* d_seq_pos) {
    Buf<u32> chunk_pos(c->pool, (size_t)pl.nchunks * n + 1);
    const u32 long_cap = (u32)std::min<u64>(nseq, pl.nchunks / (SEQ_TALLY_LANE_MAX + 1) + 1);  // sequences of more than SEQ_TALLY_LANE_MAX chunks
    Buf<u32> long_list(c->pool, long_cap), long_n(c->pool, 1);
    CBLX_HIP(hipMemsetAsync(long_n.get(), 0, 4, c->stream));
    for (u64 c0 = 0; c0 < pl.nchunks; c0 += 1ull << 25)  // one wave per chunk, fewer than 2^32 work items per launch
        hipLaunchKernelGGL(k_chunk_tally_mask, grid1(std::min<u64>(1ull << 25, pl.nchunks - c0) * 64, 256), dim3(256), 0, c->stream, d_mask, (const u64*)pl.kmer_off.get(), c0,
                           pl.nchunks, n, chunk_pos.get());
    const u64 per = (1ull << 31) / n;  // sequences per launch: fewer than 2^32 lanes
    for (u64 s0 = 0; s0 < nseq; s0 += per) {
        const u64 m = std::min(per, nseq - s0);
        hipLaunchKernelGGL(k_seq_tally_mask, grid1(m * n, 256), dim3(256), 0, c->stream, (const u64*)pl.seq_chunk.get(), (const u32*)chunk_pos.get(), s0, s0 + m, nseq, n,
                           d_seq_pos, long_list.get(), long_n.get(), long_cap);
    }
    if (pl.nchunks > SEQ_TALLY_LANE_MAX)  // else no sequence is long
        hipLaunchKernelGGL(k_seq_tally_long_mask, dim3(long_cap, n), dim3(SEQ_TALLY_LONG_THREADS), 0, c->stream, (const u32*)long_list.get(), (const u32*)long_n.get(),
                           (const u64*)pl.seq_chunk.get(), (const u32*)chunk_pos.get(), nseq, n, d_seq_pos);
    CBLX_HIP(hipGetLastError());
    CBLX_HIP(hipStreamSynchronize(c->stream));  // chunk_pos and the list die here
}
// contains_seq of a device-resident batch against n indexes at once: d_seq_total[nseq], d_seq_pos[n * nseq] (row j = srcs[j]) and one membership mask per
// k-mer in d_mask[cap] (bit j = srcs[j] holds it), any of them null; *total k-mers, positive[j] = the sum of row j (host, n entries, or null).
// `c`: the first non-empty operand (srcs[0] when all are empty) — its stream, pool and mailbox; every operand is flushed and idle.
// Routes: at most one non-empty operand -> query_device on it (byte for byte today's result); the panel join where query_flags_by_join holds and the batch
// is big enough; else KRN-1 once and k_contains per non-empty operand (only the encode is shared).
void query_panel_device(cblx_ctx* c, cblx_ctx* const* srcs, u32 n, const u8* d_bases, const u64* d_offsets, u64 nseq, u32* d_seq_total, u32* d_seq_pos, u64* d_mask,
                        u64 cap, u64* total, u64* positive) {
    if (total) *total = 0;
    if (positive) for (u32 j = 0; j < n; ++j) positive[j] = 0;
    if (nseq == 0) return;
    check_aligned16(d_bases, "d_bases");
    u32 nlive = 0, j0 = 0;
    for (u32 j = n; j-- > 0;)
        if (srcs[j]->res.count) { ++nlive; j0 = j; }  // j0: the first non-empty one
    if (nlive <= 1) {
        Buf<u8> flags;
        u64 fcap = 0;
        if (d_mask) {  // the flags of the one index, then bit j0 of every mask word
            fcap = std::min(kmers_upper_bound(c, d_offsets, 0, nseq), cap);
            flags = Buf<u8>(c->pool, fcap + 16);
        }
        u64 tot = 0, pos = 0;
        query_device(c, d_bases, d_offsets, nseq, d_mask ? flags.get() : nullptr, fcap, &tot, &pos, d_seq_total, d_seq_pos ? d_seq_pos + (size_t)j0 * nseq : nullptr);
        if (total) *total = tot;
        if (positive) positive[j0] = pos;
        if (d_seq_pos)
            for (u32 j = 0; j < n; ++j)
                if (j != j0) CBLX_HIP(hipMemsetAsync(d_seq_pos + (size_t)j * nseq, 0, nseq * 4, c->stream));
        if (d_mask && tot) {
            CBLX_HIP(hipMemsetAsync(d_mask, 0, tot * 8, c->stream));
            if (nlive) hipLaunchKernelGGL(k_mask_or_flags, grid1(tot, 256), dim3(256), 0, c->stream, (const u8*)flags.get(), tot, j0, d_mask);
            CBLX_HIP(hipGetLastError());
        }
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the flags die here
        return;
    }
    dispatch(c->P, [&](auto cfg) {
        typedef decltype(cfg) C;
        typedef typename C::HiT HiT;
        ChunkPlan pl;
        pl.keep_seq_chunk = true;
        plan_chunks(c, d_bases, d_offsets, nseq, pl);
        const u64 nk = pl.n_kmers;
        if (total) *total = nk;
        if (nk == 0) {  // (not with nseq > 0 today: every chunk holds at least its first k-mer)
            if (d_seq_total) CBLX_HIP(hipMemsetAsync(d_seq_total, 0, nseq * 4, c->stream));
            if (d_seq_pos) CBLX_HIP(hipMemsetAsync(d_seq_pos, 0, (size_t)n * nseq * 4, c->stream));
            return;
        }
        if (nk >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "too many k-mers in one query batch");
        if (d_mask && nk > cap) throw Error(CBLX_ERANGE, "mask capacity too small: " + std::to_string(nk) + " k-mers");
        Buf<u64> mask_tmp;
        if (!d_mask) { mask_tmp = Buf<u64>(c->pool, nk + 2); d_mask = mask_tmp.get(); }
        CBLX_HIP(hipMemsetAsync(d_mask, 0, nk * 8, c->stream));
        if (query_flags_by_join(c->P) && nk >= query_join_min()) {
            panel_join<C>(c, srcs, n, d_bases, pl, d_mask);
        } else {  // wide suffix, a word of more than 96 bits, or a small batch: one k_contains per non-empty index on the words encoded once
            Buf<u64> w_lo(c->pool, nk + 2);
            Buf<u8> w_hi(c->pool, (nk + 2) * std::max<size_t>(1, hi_elem_size(c->P))), flags(c->pool, nk + 8);
            encode<C>(c, d_bases, pl, w_lo.get(), (HiT*)w_hi.get(), 0);
            for (u32 j = 0; j < n; ++j) {
                if (!srcs[j]->res.count) continue;
                contains_words<C>(c, srcs[j]->res, w_lo.get(), (const HiT*)w_hi.get(), nk, flags.get());
                hipLaunchKernelGGL(k_mask_or_flags, grid1(nk, 256), dim3(256), 0, c->stream, (const u8*)flags.get(), nk, j, d_mask);
            }
            CBLX_HIP(hipGetLastError());
            CBLX_HIP(hipStreamSynchronize(c->stream));  // the words and the flags die here
        }
        Buf<u32> pos_tmp;
        u32* rows = d_seq_pos;
        if (!rows && positive) { pos_tmp = Buf<u32>(c->pool, (size_t)n * nseq); rows = pos_tmp.get(); }
        if (d_seq_total) {  // k_seq_tally with no positives to sum: the totals alone
            hipLaunchKernelGGL(k_seq_tally, grid1(nseq, 256), dim3(256), 0, c->stream, (const u64*)pl.seq_chunk.get(), (const u64*)pl.kmer_off.get(), (const u32*)nullptr, nseq,
                               d_seq_total, (u32*)nullptr, (u32*)nullptr, (u32*)nullptr, 0u);
            CBLX_HIP(hipGetLastError());
        }
        if (rows) mask_tallies(c, pl, nseq, n, d_mask, rows);
        if (positive) {
            Buf<u64> sums(c->pool, n);
            CBLX_HIP(hipMemsetAsync(sums.get(), 0, n * 8, c->stream));
            for (u32 j = 0; j < n; ++j)
                hipLaunchKernelGGL(k_sum_u32, dim3((unsigned)std::min<u64>(2048, std::max<u64>(1, ceil_div(nseq, 256)))), dim3(256), 0, c->stream, (const u32*)rows + (size_t)j * nseq,
                                   nseq, sums.get() + j);
            CBLX_HIP(hipGetLastError());
            const std::vector<u64> s = d2h_vec<u64>(c, sums.get(), n);
            for (u32 j = 0; j < n; ++j) positive[j] = s[j];
        }
        CBLX_HIP(hipStreamSynchronize(c->stream));  // the scratch mask and rows die here
    });
    collect_events(c);
}

}  // namespace
