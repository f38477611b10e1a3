// host_input.hpp — a batch that arrives from the HOST: the sliced insert behind a PCIe transfer (insert_device_sliced, insert_device_streamed),
// a big host batch as bit planes (ingest_seqs_planes) and the parallel FASTA / FASTQ reader (fastx_parallel_planes). PCIe ingest, not the
// wire: it lives behind comm.hpp because a slice that has landed takes the one-rank routes of the sharded insert. Included by cblx.cpp only.
#pragma once
#include "comm.hpp"

namespace {
// flush() of a batch sent from pinned host memory in slices (ingest_seqs): KRN-1 and the first partition pass of slice k run
// as soon as the slice has landed, while the later slices are still crossing PCIe; when the last one is in, what is left is
// the remaining passes and the bucket kernels. Same result as insert_device (the slices are pieces of the pass-A segments in
// stream order, exactly what the receiver of the multi-GPU build gets from its senders).
// `ready(s)`: returns once the ctx's stream may read slice s (s = ~0u: the offsets) — it makes the stream wait on the transfer's
// events, blocking the host first if they are not recorded yet
template <typename Ready>
void insert_device_sliced(cblx_ctx* c, const BaseView& bases, const u64* d_offsets, u64 nseq, const std::vector<u64>& seq_cuts, Ready&& ready) {
    const u32 ns = (u32)seq_cuts.size() - 1;
    {   // PREFIX_BITS > 24 on an empty index: the FINE-bins build (insert_device_fine's plan: one rank, two groups, a fixed cut) slice by slice as
        // the batch lands — two LSD passes behind the first one for the dense part of the prefix space instead of three for everything (round 6)
        if (c->P.PB > 24 && c->res.count == 0 && nseq && ns && fine_bins_enabled()) {
            cblx_comm cm;
            fine_local_comm(cm, c->P.PB);
            Replica rep;
            rep.src.resize(1);
            rep.src[0].view = bases;
            rep.src[0].d_off = d_offsets + seq_cuts[0];
            rep.src[0].nseq = seq_cuts[ns] - seq_cuts[0];
            for (u64 x : seq_cuts) rep.src[0].cuts.push_back(x - seq_cuts[0]);
            rep.per_slice = true;
            rep.ready = [&](u32 s) { ready(s); };
            bool done = false;
            dispatch(c->P, [&](auto cfg) { done = sharded_insert_grouped<decltype(cfg)>(c, &cm, nullptr, d_offsets, nseq, seq_cuts.data(), ns, nullptr, true, &rep); });
            if (done) { ++c->fine_builds; collect_events(c); return; }
        }
    }
    LocalTransport T;
    u32 none = 0;
    dispatch(c->P, [&](auto cfg) { sharded_insert_bins<decltype(cfg)>(c, T, bases, d_offsets, nseq, seq_cuts.data(), ns, &none, ready); });
    collect_events(c);
}
void insert_device_streamed(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, const Ingest::Streamed& plan) {
    auto wait_for = [&](const std::vector<hipEvent_t>& evs) { for (hipEvent_t e : evs) CBLX_HIP(hipStreamWaitEvent(c->stream, e, 0)); };
    if (c->P.PB < 9 || nseq == 0) {  // no LSD pass behind pass A: the plain path, once everything is there
        wait_for(plan.offsets_ready);
        for (auto& v : plan.ready) wait_for(v);
        insert_device(c, d_bases, d_offsets, nseq);
        return;
    }
    check_aligned16(d_bases, "d_bases");
    const bool trace = std::getenv("CBLX_TRACE_H2D") != nullptr;  // dev: when every slice had landed / was handed to the kernels
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    insert_device_sliced(c, ascii_view(d_bases), d_offsets, nseq, plan.seq_cuts, [&](u32 s) {
        if (s == ~0u) { wait_for(plan.offsets_ready); return; }
        if (trace) {
            const double a = ms();
            for (hipEvent_t e : plan.ready[s]) CBLX_HIP(hipEventSynchronize(e));
            fprintf(stderr, "[cblx h2d] slice %u: host arrives %.2f ms, landed %.2f ms\n", s, a, ms());
        }
        wait_for(plan.ready[s]);
    });
    if (trace) { CBLX_HIP(hipStreamSynchronize(c->stream)); fprintf(stderr, "[cblx h2d] done %.2f ms\n", ms()); }
}

// A big host batch as BIT PLANES (3 bits per base over PCIe instead of 8: the link is the bound of the host-input path). Host
// threads pack the caller's ASCII bases unit by unit (xfer.hpp: pack_planes) into pinned staging, an issuer thread copies every
// finished unit to the device on two streams, and THIS thread runs the sliced insert right behind them: slice s = the sequences
// that end inside the units landed so far. The index is built when the call returns (the caller's buffers are borrowed for the call
// only). Pageable or pinned source alike. Returns false when the batch does not qualify (the caller takes the other paths).
// check_slice(i0, i1): throws unless sequences [i0, i1) of the batch are well-formed (offsets non-decreasing, every length >= K)
template <typename V> bool ingest_seqs_planes(cblx_ctx* c, const u8* bases, const u64* offsets, u64 n, V&& check_slice) {
    Ingest& g = c->ing;
    const bool trace = std::getenv("CBLX_TRACE_H2D") != nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    const u64 o0 = offsets[0], len = offsets[n] >= o0 ? offsets[n] - o0 : 0;
    const char* pk = std::getenv("CBLX_H2D_PACK");  // 0 off, 1 on, default: by core count (read per call: tests switch it)
    const int mode = pk ? std::atoi(pk) : -1;
    const unsigned hc = std::thread::hardware_concurrency();
    if (mode == 0 || (mode < 0 && hc < 16)) return false;
    if (g.nseq || g.nbytes || g.query || g.staged || c->P.PB < 9 || len < (64u << 20) || n < 1024 || len >= ingest_flush_bytes()) return false;
    // transfer units = slices of the insert. Few: every slice costs fixed work (chunk plan, column scans, piece: ~0.5 ms). Measured at
    // cfg 2 with equal units: 4 / 6 / 8 / 12 / 16 / 32 units 38.8 / 37.6 / 37.8 / 39.2 / 40.5 / 46.5 ms. The kernel time line of that
    // (tools/dev_h2d_timeline.py): the wire is the bound while the units arrive (0.64 GB = 11.7 ms; KRN-1 + pass A of all of them
    // take 10.2), in front of it the packing of the first unit, behind it the kernels of the last — so the six default units
    // are 1, 3, 4, 4, 3, 1 sixteenths of the batch: a short first one (the wire starts early) and a short last one.
    const char* eu = std::getenv("CBLX_H2D_UNITS");
    const u32 NU = eu && std::atoi(eu) > 0 ? (u32)std::min(std::atoi(eu), 64) : 6u;
    std::vector<u64> ub(1, 0);  // unit k = bases [ub[k], ub[k + 1]), multiples of 1024
    {
        std::vector<u32> w;  // relative sizes (CBLX_H2D_TAPER="1,3,4,4,3,1" overrides; CBLX_H2D_UNITS = that many equal units)
        if (const char* et = std::getenv("CBLX_H2D_TAPER")) {
            for (const char* p = et; *p;) { char* q; const unsigned long v = std::strtoul(p, &q, 10); if (q == p) break; if (v) w.push_back((u32)v); p = *q ? q + 1 : q; }
        }
        if (w.empty()) { if (eu) w.assign(NU, 1u); else w = {1, 3, 4, 4, 3, 1}; }
        u64 tot = 0, acc = 0;
        for (u32 v : w) tot += v;
        for (size_t k = 0; k < w.size(); ++k) {
            acc += w[k];
            const u64 b = k + 1 == w.size() ? len : std::min<u64>(len, ((u64)((double)len * (double)acc / (double)tot) + 1023) & ~(u64)1023);
            if (b > ub.back()) ub.push_back(b);
        }
        if (ub.back() < len) ub.push_back(len);
    }
    const u32 nu = (u32)ub.size() - 1;
    auto unit_at = [&](u64 base) -> u32 { return (u32)(std::upper_bound(ub.begin(), ub.end(), base) - ub.begin()) - 1u; };
    const u64 ng = (len + 15) / 16;                                      // groups of 16 bases
    // device planes, offsets, pinned staging (kept between calls)
    if (g.d_codes.n < ng + 8) g.d_codes = Buf<u32>(c->pool, ng + 8);
    if (g.d_valid.n < ng + 8) g.d_valid = Buf<u16>(c->pool, ng + 8);
    ingest_reserve(c, 0, n);
    const size_t need = (size_t)(ng + 8) * 6;
    if (g.pin_cap < need) {
        if (g.pin) { u8* old = g.pin; g.pin = nullptr; g.pin_cap = 0; CBLX_HIP(hipHostFree(old)); }
        CBLX_HIP(hipHostMalloc((void**)&g.pin, need, hipHostMallocDefault));
        g.pin_cap = need;
    }
    u32* h_codes = (u32*)g.pin;
    u16* h_valid = (u16*)(g.pin + (size_t)(ng + 8) * 4);
    Xfer& x = xfer(c);
    hipStream_t cs[2] = {x.lane_stream(0), x.lane_stream(1)};
    // offsets (relative to the batch's first base): straight from the caller's array when pinned and zero-based, else transformed
    hipEvent_t off_ev = nullptr;
    // pinned and zero-based: the offsets of a slice travel in front of its unit (all of them up front are 80 MB at cfg 2 — 1.4 ms of
    // wire before the first base); only the last one, which sizes the arena, goes ahead
    const bool off_by_slice = o0 == 0 && Xfer::is_pinned(offsets) && Xfer::is_pinned(offsets + n);
    if (off_by_slice) x.h2d_pinned_lane0(g.d_off.get() + n, offsets + n, 8, off_ev);
    else {
        x.h2d(g.d_off.get() + 1, n * 8, [&](u8* dst, size_t off, size_t nb) {
            u64* d = (u64*)dst;
            const u64* src = offsets + off / 8 + 1;
            for (size_t j = 0; j < nb / 8; ++j) d[j] = src[j] - o0;
        });
        x.sync();
    }
    // slices: slice k = the sequences that end inside units 0 .. k
    std::vector<u64> cuts(1, 0);
    std::vector<u32> unit_of;  // the last unit a slice needs
    for (u32 k = 0; k < nu; ++k) {
        const u64 lim = ub[k + 1];
        const u64 i = k + 1 == nu ? n : (u64)(std::upper_bound(offsets + 1, offsets + n + 1, o0 + lim) - (offsets + 1));
        if (i > cuts.back()) { cuts.push_back(i); unit_of.push_back(k); }
    }
    // packers: sub-blocks of a unit in order, so that the units complete one after the other
    const u64 SB = 2u << 20;  // bases per sub-block (a multiple of 16)
    const u64 nsb = (len + SB - 1) / SB;
    std::vector<std::atomic<u32>> left(nu);
    for (u32 k = 0; k < nu; ++k) {
        const u64 a = ub[k], b = ub[k + 1];
        left[k].store((u32)((b + SB - 1) / SB - a / SB) , std::memory_order_relaxed);
    }
    // (a unit boundary is a multiple of SB only by accident: a sub-block may straddle units — it then counts for each of them)
    std::vector<std::atomic<u8>> dirty(nu);  // a base outside ACGTacgt in the unit: only then its validity plane is sent
    for (u32 k = 0; k < nu; ++k) dirty[k].store(0, std::memory_order_relaxed);
    std::atomic<u64> next_sb{0};
    std::atomic<u32> issued{0};
    std::atomic<bool> failed{false};
    std::mutex mu;
    std::condition_variable cv;
    std::vector<hipEvent_t> ev(nu, nullptr);
    const int T = (int)std::max(2u, std::min(32u, hc / 2));
    auto pack_worker = [&] {
        for (u64 sb; (sb = next_sb.fetch_add(1)) < nsb;) {
            const u64 a = sb * SB, b = std::min<u64>(len, a + SB);
            const bool clean = pack_planes(bases + o0 + a, b - a, h_codes + a / 16, h_valid + a / 16);
            for (u32 k = unit_at(a), k1 = unit_at(b - 1); k <= k1; ++k) {
                if (!clean) dirty[k].store(1, std::memory_order_relaxed);
                if (left[k].fetch_sub(1, std::memory_order_acq_rel) == 1) { std::lock_guard<std::mutex> l(mu); cv.notify_all(); }
            }
        }
    };
    auto issuer = [&] {
        try {
            CBLX_HIP(hipSetDevice(c->device));
            for (u32 k = 0; k < nu; ++k) {
                { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return left[k].load(std::memory_order_acquire) == 0; }); }
                const u64 g0 = ub[k] / 16, g1 = k + 1 == nu ? ng : ub[k + 1] / 16;
                if (off_by_slice)
                    for (size_t sl = 0; sl < unit_of.size(); ++sl)
                        if (unit_of[sl] == k && cuts[sl + 1] > cuts[sl])
                            CBLX_HIP(hipMemcpyAsync(g.d_off.get() + 1 + cuts[sl], offsets + 1 + cuts[sl], (cuts[sl + 1] - cuts[sl]) * 8, hipMemcpyHostToDevice, cs[k & 1]));
                CBLX_HIP(hipMemcpyAsync(g.d_codes.get() + g0, h_codes + g0, (g1 - g0) * 4, hipMemcpyHostToDevice, cs[k & 1]));
                if (dirty[k].load(std::memory_order_relaxed)) {
                    CBLX_HIP(hipMemcpyAsync(g.d_valid.get() + g0, h_valid + g0, (g1 - g0) * 2, hipMemcpyHostToDevice, cs[k & 1]));
                } else {
                    // every base of the unit is valid: its validity plane is all ones and is filled in on the device (a third of
                    // the unit's bytes stays off the link); the batch's last, partly filled word comes from the host
                    CBLX_HIP(hipMemsetAsync(g.d_valid.get() + g0, 0xFF, (g1 - g0) * 2, cs[k & 1]));
                    if (k + 1 == nu && (len & 15)) CBLX_HIP(hipMemcpyAsync(g.d_valid.get() + ng - 1, h_valid + ng - 1, 2, hipMemcpyHostToDevice, cs[k & 1]));
                }
                hipEvent_t e;
                CBLX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                CBLX_HIP(hipEventRecord(e, cs[k & 1]));
                ev[k] = e;
                { std::lock_guard<std::mutex> l(mu); issued.store(k + 1, std::memory_order_release); }
                cv.notify_all();
            }
        } catch (...) {
            { std::lock_guard<std::mutex> l(mu); failed = true; issued.store(nu, std::memory_order_release); }
            cv.notify_all();
        }
    };
    std::vector<std::thread> th;
    for (int t = 0; t < T; ++t) th.emplace_back(pack_worker);
    th.emplace_back(issuer);
    struct Join {
        std::vector<std::thread>& th; std::vector<hipEvent_t>& ev; hipEvent_t& off_ev; Xfer& x;
        ~Join() {
            for (auto& t : th) if (t.joinable()) t.join();
            try { x.sync(); } catch (...) {}
            for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            if (off_ev) (void)hipEventDestroy(off_ev);
        }
    } join{th, ev, off_ev, x};
    if (trace) fprintf(stderr, "[cblx h2d planes] threads started %.2f ms\n", ms());
    const BaseView view{nullptr, g.d_codes.get(), g.d_valid.get()};
    insert_device_sliced(c, view, g.d_off.get(), n, cuts, [&](u32 s) {
        if (s == ~0u) { if (off_ev) CBLX_HIP(hipStreamWaitEvent(c->stream, off_ev, 0)); return; }
        // The slice's offsets are checked before a kernel reads them (the resident index is not touched before the last slice is
        // in: a failure here leaves it as it was), while its unit is on its way and the slices in front of it run.
        check_slice(cuts[s], cuts[s + 1]);
        const u32 k = unit_of[s];
        const double a = trace ? ms() : 0;
        { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return issued.load(std::memory_order_acquire) > k; }); }
        if (failed) throw Error(CBLX_EDEVICE, "host-to-device transfer of the batch failed");
        CBLX_HIP(hipStreamWaitEvent(c->stream, ev[k], 0));               // units are copied in order on two streams:
        if (k) CBLX_HIP(hipStreamWaitEvent(c->stream, ev[k - 1], 0));    // the last one on each of them
        if (trace) fprintf(stderr, "[cblx h2d planes] slice %u (unit %u): host arrives %.2f ms, issued %.2f ms\n", s, k, a, ms());
    });
    if (trace) { CBLX_HIP(hipStreamSynchronize(c->stream)); fprintf(stderr, "[cblx h2d planes] done %.2f ms\n", ms()); }
    CBLX_HIP(hipStreamSynchronize(c->stream));
    return true;
}

// ---- a plain FASTA / FASTQ file as bit planes: the parser threads pack the sequence lines themselves -------------------------------
// The file path was bound by its host side: every region's sequence lines were copied into pinned slots and sent as ASCII (1.5 GB
// for cfg 2, 65 - 97 ms), then inserted window by window. Here a region's thread appends its lines to the batch's bit planes IN
// PLACE (PlaneSink: 16 bytes -> three 16-bit words by SSE2 movemask, shifted to the region's bit offset; only the first and the last
// word of a region are shared with its neighbours and take an atomic OR), the slices (groups of consecutive regions) are copied as
// they complete, and the calling thread runs the sliced insert right behind them, as ingest_seqs_planes does for a host batch.
bool fastx_parallel_planes(cblx_ctx* c, const char* path, u64* nrec_out) {
    Ingest& g = c->ing;
    const char* pk = std::getenv("CBLX_H2D_PACK");
    const int mode = pk ? std::atoi(pk) : -1;
    const unsigned hc = std::thread::hardware_concurrency();
    if (mode == 0 || (mode < 0 && hc < 16)) return false;
    if (g.nseq || g.nbytes || g.query || g.staged || c->P.PB < 9) return false;
    const size_t MIN_BYTES = fastx_env_bytes("CBLX_FASTX_PARALLEL_MIN", 32u << 20), REGION = fastx_env_bytes("CBLX_FASTX_REGION_BYTES", 16u << 20);
    const bool trace = std::getenv("CBLX_INGEST_TRACE") != nullptr;
    const auto t00 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t00).count(); };
    FastxMap m;
    if (!m.open(path, MIN_BYTES)) return false;
    std::vector<FastxRegion> regs;
    fx_make_regions(m, m.first, m.size, REGION, regs);
    if (trace) fprintf(stderr, "[fastx planes] mapped, %zu regions at %.2f ms\n", regs.size(), ms());
    const unsigned TP = (unsigned)fastx_env_bytes("CBLX_FASTX_THREADS", std::min(32u, std::max(2u, hc / 2)));  // parser threads (both passes)
    if (!fx_count_regions(m, regs, c->P.K, TP)) return false;
    if (trace) fprintf(stderr, "[fastx planes] counted at %.2f ms\n", ms());
    const u32 K = c->P.K;
    const u64 window = std::min<u64>(ingest_flush_bytes(), 0x78000000ull);  // bases per batch (one batch = fewer than 2^32 words)
    u64 total_rec = 0;
    Xfer& x = xfer(c);
    hipStream_t cs[2] = {x.lane_stream(0), x.lane_stream(1)};
    for (size_t w0 = 0; w0 < regs.size();) {
        size_t w1 = w0;
        u64 nbases = 0, nrec = 0;
        while (w1 < regs.size() && (w1 == w0 || nbases + regs[w1].nbases <= window)) { nbases += regs[w1].nbases; nrec += regs[w1].nrec; ++w1; }
        const size_t nr = w1 - w0;
        if (nrec == 0) { w0 = w1; continue; }
        const u64 ng = (nbases + 15) / 16;
        if (g.d_codes.n < ng + 8) g.d_codes = Buf<u32>(c->pool, ng + 8);
        if (g.d_valid.n < ng + 8) g.d_valid = Buf<u16>(c->pool, ng + 8);
        ingest_reserve(c, 0, nrec);
        const size_t need = (size_t)(ng + 8) * 6 + (size_t)nrec * 8 + 64;
        if (g.pin_cap < need) {
            if (g.pin) { u8* old = g.pin; g.pin = nullptr; g.pin_cap = 0; CBLX_HIP(hipHostFree(old)); }
            CBLX_HIP(hipHostMalloc((void**)&g.pin, need, hipHostMallocDefault));
            g.pin_cap = need;
        }
        u32* h_codes = (u32*)g.pin;
        u16* h_valid = (u16*)(g.pin + (size_t)(ng + 8) * 4);
        u64* h_ends = (u64*)(g.pin + (((size_t)(ng + 8) * 6 + 63) & ~(size_t)63));
        // the last offset (= the window's bases, known from the count) goes ahead of everything: the sliced insert sizes its arena
        // from it before the first slice (the offsets themselves travel with their slices)
        CBLX_HIP(hipMemcpy(g.d_off.get() + nrec, &nbases, 8, hipMemcpyHostToDevice));
        std::vector<u64> base(nr + 1, 0), rec0(nr + 1, 0);
        for (size_t i = 0; i < nr; ++i) { base[i + 1] = base[i] + regs[w0 + i].nbases; rec0[i + 1] = rec0[i] + regs[w0 + i].nrec; }
        fx_planes_prezero(base, ng + 8, h_codes, h_valid);
        // slices = groups of consecutive regions of about 1 / NS of the bases
        const u32 NS = 6;
        std::vector<size_t> sl(1, 0);
        for (u32 k = 1; k <= NS; ++k) {
            size_t i = sl.back();
            while (i < nr && base[i] < nbases * k / NS) ++i;
            if (k == NS) i = nr;
            if (i > sl.back()) sl.push_back(i);
        }
        const u32 ns = (u32)sl.size() - 1;
        std::vector<u64> cuts(ns + 1);
        for (u32 k = 0; k <= ns; ++k) cuts[k] = rec0[sl[k]];
        std::vector<u32> slice_of(nr);
        std::vector<std::atomic<u32>> left(ns);
        for (u32 k = 0; k < ns; ++k) { left[k].store((u32)(sl[k + 1] - sl[k])); for (size_t i = sl[k]; i < sl[k + 1]; ++i) slice_of[i] = k; }
        std::atomic<size_t> next{0};
        std::atomic<u32> issued{0};
        std::atomic<bool> failed{false};
        std::mutex mu;
        std::condition_variable cv;
        std::vector<hipEvent_t> ev(ns, nullptr);
        const u8* d = m.d;
        const char fmt = m.fmt;
        auto worker = [&] {
            for (size_t i; (i = next.fetch_add(1)) < nr;) {
                const FastxRegion& r = regs[w0 + i];
                PlaneSink sink(h_codes, h_valid, base[i], h_ends + rec0[i], r.nrec, base[i + 1]);
                if (!fx_walk(d, r, fmt, K, sink) || sink.overflow || sink.pos != base[i + 1] || sink.nrec != r.nrec) failed = true;
                sink.finish();
                if (left[slice_of[i]].fetch_sub(1, std::memory_order_acq_rel) == 1) { std::lock_guard<std::mutex> l(mu); cv.notify_all(); }
            }
        };
        auto issuer = [&] {
            try {
                CBLX_HIP(hipSetDevice(c->device));
                for (u32 k = 0; k < ns; ++k) {
                    { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return left[k].load(std::memory_order_acquire) == 0; }); }
                    // the slice's groups, its last, possibly shared word included. A slice that STARTS inside a group shares that
                    // word with its predecessor, whose copy of it (taken before this slice's bits were all there) runs on the other
                    // stream: two DMA writes of one word with nothing between them — whichever lands last stays. So the word this
                    // slice shares with its predecessor is copied separately, BEHIND the predecessor's event; the bulk does not wait.
                    const bool shared_front = k > 0 && (base[sl[k]] & 15) != 0;
                    const u64 g0 = base[sl[k]] >> 4, g1 = std::min<u64>(ng, (base[sl[k + 1]] + 15) >> 4), gb = std::min(g1, g0 + (shared_front ? 1 : 0));
                    hipStream_t st = cs[k & 1];
                    if (g1 > gb) {
                        CBLX_HIP(hipMemcpyAsync(g.d_codes.get() + gb, h_codes + gb, (g1 - gb) * 4, hipMemcpyHostToDevice, st));
                        CBLX_HIP(hipMemcpyAsync(g.d_valid.get() + gb, h_valid + gb, (g1 - gb) * 2, hipMemcpyHostToDevice, st));
                    }
                    if (gb > g0) {
                        CBLX_HIP(hipStreamWaitEvent(st, ev[k - 1], 0));
                        CBLX_HIP(hipMemcpyAsync(g.d_codes.get() + g0, h_codes + g0, 4, hipMemcpyHostToDevice, st));
                        CBLX_HIP(hipMemcpyAsync(g.d_valid.get() + g0, h_valid + g0, 2, hipMemcpyHostToDevice, st));
                    }
                    if (cuts[k + 1] > cuts[k]) CBLX_HIP(hipMemcpyAsync(g.d_off.get() + 1 + cuts[k], h_ends + cuts[k], (cuts[k + 1] - cuts[k]) * 8, hipMemcpyHostToDevice, st));
                    hipEvent_t e;
                    CBLX_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
                    CBLX_HIP(hipEventRecord(e, st));
                    ev[k] = e;
                    { std::lock_guard<std::mutex> l(mu); issued.store(k + 1, std::memory_order_release); }
                    cv.notify_all();
                }
            } catch (...) {
                { std::lock_guard<std::mutex> l(mu); failed = true; issued.store(ns, std::memory_order_release); }
                cv.notify_all();
            }
        };
        const int T = (int)std::max<size_t>(1, std::min<size_t>(TP, nr));
        std::vector<std::thread> th;
        for (int t = 0; t < T; ++t) th.emplace_back(worker);
        th.emplace_back(issuer);
        struct Join {
            std::vector<std::thread>& th; std::vector<hipEvent_t>& ev; Xfer& x;
            ~Join() {
                for (auto& t : th) if (t.joinable()) t.join();
                try { x.sync(); } catch (...) {}
                for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
            }
        } join{th, ev, x};
        const BaseView view{nullptr, g.d_codes.get(), g.d_valid.get()};
        insert_device_sliced(c, view, g.d_off.get(), nrec, cuts, [&](u32 s) {
            if (s == ~0u) s = 0;  // the offsets of a slice travel with it: the first read needs slice 0
            { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&] { return issued.load(std::memory_order_acquire) > s; }); }
            if (failed) throw Error(CBLX_EDEVICE, "fastx: the file changed while it was being read");
            CBLX_HIP(hipStreamWaitEvent(c->stream, ev[s], 0));
            if (s) CBLX_HIP(hipStreamWaitEvent(c->stream, ev[s - 1], 0));
            if (trace) fprintf(stderr, "[fastx planes] slice %u handed over at %.2f ms\n", s, ms());
        });
        CBLX_HIP(hipStreamSynchronize(c->stream));
        if (failed) throw Error(CBLX_EDEVICE, "fastx: the file changed while it was being read");
        total_rec += nrec;
        if (trace) fprintf(stderr, "[fastx planes] window of %llu records done at %.2f ms\n", (unsigned long long)nrec, ms());
        w0 = w1;
    }
    if (nrec_out) *nrec_out = total_rec;
    return true;
}

}  // namespace
