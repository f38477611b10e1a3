// pipeline.hpp — one batch of words into the resident index: KRN-2 stable partition and KRN-4 directory (partition_and_directory), the batch through them and
// the bucket stage into an empty or a non-empty index (pipeline, pipeline_group), the KRN-1 front end (chunk plan + encode), the first partition pass of a piece
// of reads, insert_device, and the sorted batches of the multi-GPU build. The KRN-3 driver is bucket_stage.hpp, the query side query.hpp; set algebra and
// removal build on this file in setops.hpp. Included by cblx.cpp only.
#pragma once
#include "bucket_stage.hpp"
#include "ctx.hpp"
#include "kernels_kmer.hpp"

namespace {

// ---- the sort + directory + per-bucket pipeline over N records (lo/hi), resident records first -------------
struct Records {
    Buf<u64> lo, lo2;
    Buf<u8> hi, hi2;  // raw bytes; element size = hi_elem_size
    const u64* ext_lo = nullptr;  // optional caller-owned source of the FIRST pass (no resident words in front)
    const void* ext_hi = nullptr;
};

// Records that arrive with the first partition pass already done and in PIECES (receiver of the multi-GPU build, comm.hpp):
// rec.lo (and rec.hi for words that keep their hi part) is the receive arena; piece p = what one (slice, source rank) sent,
// sorted by the pass-A segment, cnt[p][256] records per segment from arena position pbase[p]; stream order = piece order.
struct PieceInput {
    u32 np = 0;
    const u32* cnt = nullptr;    // host [np][256]
    const u32* pbase = nullptr;  // host [np]
    Buf<u8>* dig = nullptr;      // the first LSD pass's digit of every record (same positions), owned by the caller; reused as the side channel
    // ... or, for ONE GROUP of a receive log that other groups still need (comm.hpp, grouped receiver): the digits are read where they
    // are and the later passes' side channel goes to a buffer of the group's own (at least N + 64 bytes)
    const u8* dig_in = nullptr;
    u8* dig_out = nullptr;
    // FINE bins (cuts.hpp: make_fine_plan): the "segments" are bins of the senders' first pass that lie inside aligned blocks of
    // 2^sort_bits prefixes — the passes sort that many prefix bits (16: two passes, 24: three) and a record's prefix is
    // seg_prefix[segment] | its low sort_bits bits (host array of 256; 0 / null: segment = top 8 prefix bits, PREFIX_BITS - 8 bits sorted)
    u32 sort_bits = 0;
    const u32* seg_prefix = nullptr;
};

// A group of the grouped receiver works on its WINDOW [w_lo, w_hi) of the prefix space (both multiples of 64; its records hold no
// other prefix): start_dense, the popcounts and the bucket table cover the window only, the bitvector words are written straight
// into the final bitvector `bv` (2^PB bits, zeroed by the caller; windows of different groups share no word), and the directory
// that comes back is the window's: nr.nb buckets, nr.prefix (absolute values), nr.start (positions relative to the group's records),
// nr.rank_dir relative to the window. nr.bv stays empty.
struct DirWindow {
    u32 w_lo = 0, w_hi = 0;
    u64* bv = nullptr;
};

// the LSD passes behind pass A: digit widths and shifts (relative to SUFFIX_BITS) of the remaining prefix bits
struct LsdPlan {
    u32 npass = 0, wid[4] = {0, 0, 0, 0}, sh[5] = {0, 0, 0, 0, 0};
    u32 xb = 0;  // lowest prefix bits left to k_prefix_split (the passes sort the PB - xb bits above them)
    u32 total() const { return npass + (xb ? 1u : 0u); }  // times the records change buffers behind pass A
};
// `split_ok` = false: records that arrive in pieces (the receiver of the multi-GPU build, and its senders, whose side channel carries
// the first pass's digit): at the bucket depth of a many-GPU job a run of equal 24-bit prefix holds tens of thousands of records, which
// k_prefix_split has to read twice (12 ms per 1.5 G records against 6.2 for a scatter pass, profiles/r04_wire_emulated.md): three passes.
inline LsdPlan lsd_plan(const Consts& P, bool split_ok = true) {
    // Up to two passes: 8 bits, then the rest (the group-cut tiles of the last pass are built for that shape). PREFIX_BITS > 24:
    // 8 + 8 bits by two passes with the directory of 2^24 "super-prefixes" from the second one's tables, and the last 1 .. 4 bits
    // by k_prefix_split (a run of equal 24-bit prefix staged in LDS, written back in order: copy speed, DESIGN_HISTORY.md §3.11). Three passes
    // of 7 + 7 + 6 bits before that, and still without `split_ok`: a pass costs nearly the same whatever its width.
    LsdPlan L;
    const u32 RB = P.PB - std::min(8u, P.PB);
    if (split_ok && P.PB > 24) {
        L.xb = P.PB - 24;
        L.npass = 2;
        L.wid[0] = L.wid[1] = 8;
        L.sh[0] = L.xb; L.sh[1] = L.xb + 8; L.sh[2] = L.xb + 16;
        return L;
    }
    L.npass = (RB + 7) / 8;
    for (u32 i = 0; i < L.npass; ++i) {
        L.wid[i] = L.npass <= 2 ? std::min(8u, RB - 8 * i) : RB / L.npass + (i < RB % L.npass ? 1u : 0u);
        L.sh[i + 1] = L.sh[i] + L.wid[i];
    }
    return L;
}
// FINE bins: `bits` (16 or 24) prefix bits in passes of 8 from the bottom — the first digit is the same for every group, so the senders'
// side channel does not depend on who receives a record
inline LsdPlan lsd_plan_bits(u32 bits) {
    LsdPlan L;
    L.npass = (bits + 7) / 8;
    for (u32 i = 0; i < L.npass; ++i) { L.wid[i] = std::min(8u, bits - 8 * i); L.sh[i + 1] = L.sh[i] + L.wid[i]; }
    return L;
}

// KRN-2 + KRN-4 over N records: stable partition by prefix, then the directory (bitvector, rank directory, bucket table
// with the RAW run of every prefix; nr.cnt / nr.kind are allocated, not filled). The sorted records end up in rec.lo/hi.
// `countsA`: histogram of the first pass already accumulated by KRN-1 (empty Buf = compute it here)
template <typename C> void partition_and_directory(cblx_ctx* c, Records& rec, u64 N, Buf<u32> countsA, Resident& nr, const PieceInput* pin = nullptr, const DirWindow* win = nullptr) {
    typedef typename C::HiT HiT;
    const Consts& P = c->P;
    if (N >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "a single batch takes fewer than 2^32-16 words (callers cut larger inserts into sub-batches)");
    // ping-pong: A = rec.lo/hi, B = rec.lo2/hi2. With an external source pass 0 reads it and writes A.
    const u64* lo = rec.ext_lo ? rec.ext_lo : rec.lo.get();
    const HiT* hi = rec.ext_lo ? (const HiT*)rec.ext_hi : (const HiT*)rec.hi.get();
    u64* lo2 = rec.ext_lo ? rec.lo.get() : rec.lo2.get();
    HiT* hi2 = rec.ext_lo ? (HiT*)rec.hi.get() : (HiT*)rec.hi2.get();
    u64* lo_other = rec.ext_lo ? rec.lo2.get() : rec.lo.get();   // the buffer that becomes the destination after pass 0
    HiT* hi_other = rec.ext_lo ? (HiT*)rec.hi2.get() : (HiT*)rec.hi.get();
    auto advance = [&]() { const u64* nl = lo2; const HiT* nh = hi2; lo2 = lo_other; hi2 = hi_other; lo_other = const_cast<u64*>(nl); hi_other = const_cast<HiT*>(nh); lo = nl; hi = nh; };
    // -- KRN-2: stable radix partition on the PREFIX_BITS above SUFFIX_BITS.
    //    Pass A sorts by the MOST significant 8 prefix bits (the skewed digit: long output runs) and cuts the array into
    //    <= 256 segments; the remaining bits are sorted by stable LSD passes INSIDE every segment (tiles never straddle a
    //    segment). For 65..72-bit words (K = 31) the bits the hi byte held are implied by the segment after pass A, so
    //    it is dropped there: every later pass, the boundary scan and KRN-3 move 8-byte records only.
    //    Per pass: tile histogram, column scan, per-segment adjust, LDS-staged scatter.
    constexpr bool DROP_HI = std::is_same<HiT, u8>::value;
    Buf<u32> seg_start(c->pool, 257);
    // PREFIX_BITS > 24: the passes sort the top PBs = 24 prefix bits ("super-prefixes": the xb bits below them count as suffix here,
    // SBs), their directory comes from the last pass's tables, and k_prefix_split finishes the job run by run (below)
    const bool fine = pin && pin->sort_bits != 0;
    const LsdPlan LP = fine ? lsd_plan_bits(pin->sort_bits) : lsd_plan(P, pin == nullptr);
    const u32 xb = LP.xb, PBs = P.PB - xb, SBs = P.SB + xb;
    const u32 nA = std::min(8u, PBs), RB = fine ? pin->sort_bits : PBs - nA;  // bits of pass A, bits left for the LSD passes
    Buf<u32> d_segp;  // FINE bins: first prefix of every segment's aligned block
    if (fine) { d_segp = Buf<u32>(c->pool, 256); h2d(c, d_segp.get(), pin->seg_prefix, 256); }
    const u32* segp = d_segp.get();
    const u32 w_lo = win ? win->w_lo : 0u;
    const u64 nprefix = win ? (u64)win->w_hi - win->w_lo : 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    if (win && ((win->w_lo | win->w_hi) & 63u)) throw Error(CBLX_EINVAL, "a directory window must be cut at multiples of 64 (internal error)");
    // the directory the PASSES produce: of the prefixes (xb = 0), or of the super-prefixes of the window
    const u32 sw_lo = w_lo >> xb;
    const u64 sw_hi = win ? ((u64)win->w_hi + ((1u << xb) - 1u)) >> xb : 1ull << PBs, nsuper = sw_hi - sw_lo;
    Buf<u32> start_dense(c->pool, std::max<u64>(nsuper, 1));
    u32* sd = start_dense.get() - sw_lo;  // indexed by the absolute (super-)prefix
    bool have_dense = false;
    {
        // pieces: every (segment, piece) may end in a partly filled tile
        const u32 ntiles = (u32)ceil_div(N, RDX_TILE), nt_max = ntiles + 256 * (pin ? std::max(1u, pin->np) : 1u);
        const u32 npassL = LP.npass, nseg = 1u << nA;
        const u32 (&wid)[4] = LP.wid;
        const u32 (&sh)[5] = LP.sh;
        if (pin && (npassL == 0 || nA != 8)) throw Error(CBLX_EINVAL, "records in pieces need PREFIX_BITS >= 9 (internal error)");
        // The last LSD pass cuts its tiles at (segment x lower digits) groups when there are few enough of them; the
        // bucket directory then comes from that pass's tables (k_dir_gather) instead of a scan of the sorted records.
        const u32 low_bits = npassL ? sh[npassL - 1] - xb : 0, last_bits = RB - low_bits;
        const bool tbl_dir = npassL >= 1 && nA + low_bits <= 16;
        const bool grp_tiles = tbl_dir && low_bits > 0;  // low_bits = 0: the groups are the segments (existing tile table)
        const u32 G = nseg << low_bits, nt_maxC = grp_tiles ? ntiles + G + 256 : nt_max;
        const bool haveA = countsA.get() != nullptr;
        Buf<u32> counts = haveA ? std::move(countsA) : (pin ? Buf<u32>() : Buf<u32>(c->pool, (size_t)256 * nt_max));  // pass A's tile histogram
        // column prefixes: two levels (colprefix.hpp) in pass A and in every LSD pass fed by the digit side channel; an LSD pass that
        // has to count from the records (pieces that came without their digits) keeps the flat matrix, allocated when it is needed
        SupPrefix sp;
        sp.reserve(c, std::max(nt_max, nt_maxC));
        Buf<u32> colpre, scratch, coltot(c->pool, 256),
            adj(c->pool, 256 * 256), seg_first(c->pool, 257), nt_dev(c->pool, 1), t_start(c->pool, nt_max), t_count(c->pool, nt_max);
        Buf<u16> t_seg(c->pool, nt_max);
        Buf<u32> grp_start, grp_first, seg_firstC, nt_devC, t_startC, t_countC;
        Buf<u16> t_segC;
        if (grp_tiles) {
            grp_start = Buf<u32>(c->pool, G + 1);
            grp_first = Buf<u32>(c->pool, G + 1);
            seg_firstC = Buf<u32>(c->pool, 257);
            nt_devC = Buf<u32>(c->pool, 1);
            t_startC = Buf<u32>(c->pool, nt_maxC);
            t_countC = Buf<u32>(c->pool, nt_maxC);
            t_segC = Buf<u16>(c->pool, nt_maxC);
        }
        // digit side channel: a scatter also writes the NEXT pass's digit of every record (1 byte, same order). (When the
        // hi byte is dropped by pass A the remaining digits all lie in the lo word: the word has <= 72 bits.)
        Buf<u8> dig;
        const u8* dig_rd = nullptr;  // what this pass's histogram reads ...
        u8* dig_wr = nullptr;        // ... and where its scatter leaves the next pass's digits (the same array unless the caller split them)
        Buf<u32> seg_tot;  // pieces: records per pass-A segment
        bool have_dig = false;
        auto next_digit = [&](u32 next_pass) -> DigitBits {
            if (next_pass >= npassL) return DigitBits{0, 0};
            return DigitBits{P.SB + sh[next_pass], wid[next_pass]};
        };
        if (pin && pin->dig_in) { dig_rd = pin->dig_in; dig_wr = pin->dig_out; have_dig = true; }
        else if (pin && pin->dig) { dig = std::move(*pin->dig); have_dig = dig.get() != nullptr; dig_rd = dig_wr = dig.get(); }
        else if (next_digit(0).nbits) { dig = Buf<u8>(c->pool, N + 64); dig_rd = dig_wr = dig.get(); }
        if (pin) {
            // pass A ran on the senders: segment and tile tables of the first LSD pass from the piece table
            StageTimer t(c, ST_SCAN);
            const u32 np = pin->np;
            seg_tot = Buf<u32>(c->pool, 256);
            Buf<u32> d_cnt(c->pool, (size_t)np * 256), d_pbase(c->pool, np), pfirst(c->pool, (size_t)np * 256), ppos(c->pool, (size_t)np * 256);
            h2d(c, d_cnt.get(), pin->cnt, (size_t)np * 256);
            h2d(c, d_pbase.get(), pin->pbase, np);
            hipLaunchKernelGGL(k_piece_tables, dim3(1), dim3(256), 0, c->stream, d_cnt.get(), d_pbase.get(), np, seg_start.get(), seg_first.get(), nt_dev.get(), pfirst.get(), ppos.get(),
                               seg_tot.get());
            hipLaunchKernelGGL(k_piece_tile_table, grid1(nt_max, 256), dim3(256), 0, c->stream, d_cnt.get(), np, seg_first.get(), nt_dev.get(), pfirst.get(), ppos.get(), t_start.get(),
                               t_count.get(), t_seg.get());
            CBLX_HIP(hipGetLastError());
            // the piece tables are released here. (A group of the grouped receiver skips the host wait: everything that could reuse the
            // blocks is queued on this stream behind the kernels that read them, and eight groups pay every idle gap eight times)
            if (!win) CBLX_HIP(hipStreamSynchronize(c->stream));
        } else {   // pass A
            const TileView tv{nullptr, nullptr, nullptr, nullptr, ntiles, N};
            const DigitBits dfn{SBs + RB, nA};
            const DigitBits nd = next_digit(0);
            u8* ndp = nd.nbits ? dig_wr : nullptr;
            if (!haveA) { StageTimer t(c, ST_HIST);
              hipLaunchKernelGGL((k_radix_hist<HiT, DigitBits>), dim3(xcd_grid(ntiles)), dim3(RDX_THREADS), 0, c->stream, lo, hi, tv, dfn, counts.get()); }
            { StageTimer t(c, ST_SCAN);
              hipLaunchKernelGGL(k_colscan_sup, dim3(std::max(1u, sup_count(ntiles))), dim3(128), 0, c->stream, (const u32*)counts.get(), ntiles, sp.local.get(), sp.sup.get());
              sp.scan(c, false, ntiles, coltot.get());
              hipLaunchKernelGGL(k_seg_adjust, dim3(1), dim3(256), 0, c->stream, sp.view(), coltot.get(), (const u32*)nullptr, (const u32*)nullptr,
                                 (const u32*)nullptr, ntiles, 1u, adj.get(), (u32*)nullptr);
              hipLaunchKernelGGL(k_seg_table, dim3(1), dim3(256), 0, c->stream, coltot.get(), seg_start.get(), seg_first.get(), nt_dev.get());
              hipLaunchKernelGGL(k_tile_table, grid1(nt_max, 256), dim3(256), 0, c->stream, seg_start.get(), seg_first.get(), nt_dev.get(), t_start.get(),
                                 t_count.get(), t_seg.get()); }
            { StageTimer t(c, ST_SCATTER);
              c->stages[ST_SCATTER].units += N;  // (records through a partition pass: cblx_stage_units — the passes a record takes vary with the route)
              if constexpr (DROP_HI)
                  hipLaunchKernelGGL((k_radix_scatter<HiT, NoHi, DigitBits>), dim3(xcd_grid(ntiles)), dim3(RDX_THREADS), 0, c->stream, lo, hi, tv, dfn, sp.view(),
                                     adj.get(), lo2, (NoHi*)nullptr, nd, ndp);
              else
                  hipLaunchKernelGGL((k_radix_scatter<HiT, HiT, DigitBits>), dim3(xcd_grid(ntiles)), dim3(RDX_THREADS), 0, c->stream, lo, hi, tv, dfn, sp.view(),
                                     adj.get(), lo2, hi2, nd, ndp); }
            have_dig = ndp != nullptr;
            advance();
        }
        counts.reset();  // pass A's count matrix: the LSD passes count in LDS
        const TileView tvL{t_start.get(), t_count.get(), t_seg.get(), nt_dev.get(), nt_max, N};
        const TileView tvC{t_startC.get(), t_countC.get(), t_segC.get(), nt_devC.get(), nt_maxC, N};
        for (u32 pass = 0; pass < npassL; ++pass) {
            const DigitBits dfn{P.SB + sh[pass], wid[pass]};
            const bool last = pass + 1 == npassL;
            const bool cut = last && grp_tiles;  // this pass runs on the group-cut tiles
            const TileView& tv = cut ? tvC : tvL;
            const u32 ntm = cut ? nt_maxC : nt_max;
            const u32 *ntd = cut ? nt_devC.get() : nt_dev.get(), *sf = cut ? seg_firstC.get() : seg_first.get();
            auto run = [&](auto hi_tag) {
                typedef decltype(hi_tag) H;  // record layout of the LSD passes: no hi once it was dropped
                const H* hin = (const H*)hi;
                H* hout = (H*)hi2;
                const DigitBits nd = next_digit(pass + 1);
                u8* ndp = nd.nbits && dig_wr ? dig_wr : nullptr;
                const bool two_level = have_dig;
                if (!two_level && colpre.n < (size_t)256 * ntm) { counts = Buf<u32>(c->pool, (size_t)256 * ntm); colpre = Buf<u32>(c->pool, (size_t)256 * ntm); }
                const ColPre cp = two_level ? sp.view() : ColPre(colpre.get());
                { StageTimer t(c, ST_HIST);
                  if (two_level)
                      hipLaunchKernelGGL(k_radix_hist_bytes, dim3(std::max(1u, sup_count(ntm))), dim3(64 * SUP_TILES), 0, c->stream, dig_rd, tv, sp.local.get(), sp.sup.get(), sp.nst_dev.get());
                  else
                      hipLaunchKernelGGL((k_radix_hist<H, DigitBits>), dim3(xcd_grid(ntm)), dim3(RDX_THREADS), 0, c->stream, lo, hin, tv, dfn, counts.get()); }
                { StageTimer t(c, ST_SCAN);
                  if (two_level) sp.scan(c, true, ntm, coltot.get());
                  else colscan(c, counts.get(), ntd, ntm, colpre.get(), coltot.get(), scratch);
                  hipLaunchKernelGGL(k_seg_adjust, dim3(nseg), dim3(256), 0, c->stream, cp, coltot.get(), sf, seg_start.get(), ntd, ntm, nseg, adj.get(),
                                     (grp_tiles && pass + 2 == npassL) ? grp_start.get() : (u32*)nullptr);
                  if (grp_tiles && pass + 2 == npassL) {  // the next pass is the last one: cut its tiles at the groups this pass creates
                      hipLaunchKernelGGL(k_grp_table, dim3(1), dim3(1024), 0, c->stream, G, low_bits, grp_start.get(), seg_start.get(), (u32)N, grp_first.get(), seg_firstC.get(),
                                         nt_devC.get());
                      hipLaunchKernelGGL(k_tile_table_grp, grid1(nt_maxC, 256), dim3(256), 0, c->stream, G, low_bits, grp_start.get(), seg_start.get(), (u32)N, grp_first.get(), nt_devC.get(),
                                         t_startC.get(), t_countC.get(), t_segC.get());
                  } }
                // more groups than the table method takes: the last pass finds the bucket starts itself (fused directory)
                const bool fused_dir = last && !tbl_dir;
                const u32 amb_stride = 1u << dfn.nbits;
                Buf<u32> amb;
                if (fused_dir) {
                    amb = Buf<u32>(c->pool, (size_t)ntm * amb_stride);
                    CBLX_HIP(hipMemsetAsync(start_dense.get(), 0xFF, nsuper * 4, c->stream));
                }
                { StageTimer t(c, ST_SCATTER);
                  c->stages[ST_SCATTER].units += N;
                  hipLaunchKernelGGL((k_radix_scatter<H, H, DigitBits>), dim3(xcd_grid(ntm)), dim3(RDX_THREADS), 0, c->stream, lo, hin, tv, dfn, cp,
                                     adj.get(), lo2, hout, nd, ndp, fused_dir ? sd : (u32*)nullptr, SBs, RB, low_bits, amb.get(), amb_stride,
                                     OwnWindow{0, 0, nullptr, nullptr, nullptr}, (const u64*)nullptr, segp); }
                if (fused_dir) {
                    StageTimer t(c, ST_DIR);
                    hipLaunchKernelGGL(k_dir_resolve<H>, grid1((u64)ntm * amb_stride, 256), dim3(256), 0, c->stream, ntd, amb_stride, (const u32*)amb.get(), tv.seg,
                                       (const u32*)seg_start.get(), (const u64*)lo2, (const H*)hout, SBs, RB, sd, segp);
                    CBLX_HIP(hipStreamSynchronize(c->stream));  // amb is released at the end of this scope
                    have_dense = true;
                }
                have_dig = ndp != nullptr;
                if (have_dig) dig_rd = dig_wr;  // the next pass reads what this one wrote
                if (pin && pass == 0 && !last) {
                    // the piece tiles described the arena; from here on the segments are contiguous: the plain tile table
                    // (the column totals of the pass that made the segments were kept aside: this pass's scan overwrote coltot)
                    StageTimer t(c, ST_SCAN);
                    hipLaunchKernelGGL(k_seg_table, dim3(1), dim3(256), 0, c->stream, (const u32*)seg_tot.get(), seg_start.get(), seg_first.get(), nt_dev.get());
                    hipLaunchKernelGGL(k_tile_table, grid1(nt_max, 256), dim3(256), 0, c->stream, seg_start.get(), seg_first.get(), nt_dev.get(), t_start.get(), t_count.get(), t_seg.get());
                }
                if (last && tbl_dir) {
                    StageTimer t(c, ST_DIR);
                    // FINE bins: the segments' blocks need not cover the window (the last group's reaches up to 2^PREFIX_BITS, its bins do not)
                    if (fine) CBLX_HIP(hipMemsetAsync(start_dense.get(), 0xFF, nsuper * 4, c->stream));
                    hipLaunchKernelGGL(k_dir_gather, dim3(G), dim3(256), 0, c->stream, low_bits, last_bits, grp_tiles ? grp_first.get() : seg_first.get(), seg_start.get(), ntd,
                                       cp, coltot.get(), adj.get(), sd, sw_lo, win ? (u32)std::min<u64>(sw_hi, 0xFFFFFFFFull) : 0xFFFFFFFFu, segp);
                    if (grp_tiles)  // cold segments kept plain tiles: their boundaries come from their (few) records, now in lo2
                        hipLaunchKernelGGL(k_boundaries_cold<H>, dim3(nseg, 32), dim3(256), 0, c->stream, (const u64*)lo2, (const H*)hout, SBs, RB, seg_start.get(), sd, segp);
                    have_dense = true;
                }
            };
            if constexpr (DROP_HI) run(NoHi()); else run(HiT());
            advance();
        }
        CBLX_HIP(hipGetLastError());
        if (!win) CBLX_HIP(hipStreamSynchronize(c->stream));  // the pass tables are released here (a group: see above)
    }
    bool dir_done = false;
    if (xb) {
        // -- the last xb prefix bits: every run of equal super-prefix split in LDS, written to the other buffer in final order; the
        //    directory comes from the runs' own small tables (k_prefix_split, k_split_table) — nothing walks the 2^PREFIX_BITS prefixes
        if (!have_dense) throw Error(CBLX_EDEVICE, "prefix split without a super-prefix directory (internal error)");
        if (win) throw Error(CBLX_EINVAL, "prefix split inside a directory window (internal error)");
        const u64 swords = std::max<u64>(1, (nsuper + 63) / 64);
        Buf<u32> spopc(c->pool, swords), sprefix;
        Buf<u64> sbv(c->pool, swords), srank(c->pool, swords + 1), sstart;
        u64 nruns = 0;
        { StageTimer t(c, ST_DIR);
          CBLX_HIP(hipMemsetAsync(spopc.get(), 0, swords * 4, c->stream));
          CBLX_HIP(hipMemsetAsync(sbv.get(), 0, swords * 8, c->stream));
          hipLaunchKernelGGL(k_bitvector, grid1(std::max<u64>(nsuper, 64), 256), dim3(256), 0, c->stream, start_dense.get(), nsuper, sbv.get(), spopc.get());
          nruns = exclusive_scan<u64>(c, spopc.get(), swords, srank.get());
          sprefix = Buf<u32>(c->pool, nruns + 1);
          sstart = Buf<u64>(c->pool, nruns + 1);
          hipLaunchKernelGGL(k_bucket_table, grid1(std::max<u64>(nsuper, 1), 256), dim3(256), 0, c->stream, start_dense.get(), nsuper, sbv.get(), srank.get(), sprefix.get(), sstart.get(), sw_lo);
          hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, sstart.get() + nruns, N); }
        if (nruns >= 0xFFFFFFF0ull / 16) throw Error(CBLX_ERANGE, "too many runs for the prefix split");
        Buf<u32> sub_start(c->pool, 16 * nruns + 16), sub_nz(c->pool, nruns + 1);
        Buf<u16> sub_mask(c->pool, nruns + 1);
        Buf<u64> rank_base(c->pool, nruns + 1);
        if (nruns) {
            StageTimer t(c, ST_SCATTER);
            c->stages[ST_SCATTER].units += N;
            Buf<SplitRun> lists(c->pool, SPLIT_CLASSES * nruns);
            Buf<u32> list_n(c->pool, SPLIT_CLASSES);
            CBLX_HIP(hipMemsetAsync(list_n.get(), 0, SPLIT_CLASSES * 4, c->stream));
            hipLaunchKernelGGL(k_split_classify, grid1(nruns, 1024), dim3(1024), 0, c->stream, nruns, sstart.get(), lists.get(), list_n.get());
            const std::vector<u32> ln = d2h_vec<u32>(c, list_n.get(), SPLIT_CLASSES);
            auto launch = [&](auto h_tag, const auto* hin, auto* hout) {
                typedef decltype(h_tag) H;
                if (ln[0]) hipLaunchKernelGGL((k_prefix_split<H, 64>), dim3(ln[0]), dim3(64), 0, c->stream, lists.get(), lo, hin, lo2, hout, P.SB, xb, sub_start.get(), sub_mask.get(), sub_nz.get());
                if (ln[1]) hipLaunchKernelGGL((k_prefix_split<H, 128>), dim3(ln[1]), dim3(128), 0, c->stream, lists.get() + nruns, lo, hin, lo2, hout, P.SB, xb, sub_start.get(), sub_mask.get(), sub_nz.get());
                if (ln[2]) hipLaunchKernelGGL((k_prefix_split<H, 256>), dim3(ln[2]), dim3(256), 0, c->stream, lists.get() + 2 * nruns, lo, hin, lo2, hout, P.SB, xb, sub_start.get(), sub_mask.get(), sub_nz.get());
                if (ln[3]) hipLaunchKernelGGL((k_prefix_split<H, 512>), dim3(ln[3]), dim3(512), 0, c->stream, lists.get() + 3 * nruns, lo, hin, lo2, hout, P.SB, xb, sub_start.get(), sub_mask.get(), sub_nz.get());
            };
            if constexpr (DROP_HI || !HiTraits<HiT>::has) launch(NoHi(), (const NoHi*)nullptr, (NoHi*)nullptr);
            else launch(HiT(), hi, hi2);
            CBLX_HIP(hipGetLastError());
            advance();
        }
        {   // KRN-4 from the runs' tables: bucket table rows by rank, bitvector bits run by run, rank directory by one popcount scan
            StageTimer t(c, ST_DIR);
            nr.nb = nruns ? exclusive_scan<u64>(c, sub_nz.get(), nruns, rank_base.get()) : 0;
            nr.bv = Buf<u64>(c->pool, nwords);
            nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
            nr.prefix = Buf<u32>(c->pool, nr.nb + 1);
            nr.start = Buf<u64>(c->pool, nr.nb + 1);
            nr.cnt = Buf<u32>(c->pool, nr.nb + 1);
            nr.kind = Buf<u8>(c->pool, nr.nb + 1);
            Buf<u32> popc(c->pool, nwords);
            CBLX_HIP(hipMemsetAsync(nr.bv.get(), 0, nwords * 8, c->stream));
            if (nruns)
                hipLaunchKernelGGL(k_split_table, grid1(nruns * 16, 256), dim3(256), 0, c->stream, nruns, (const u32*)sprefix.get(), (const u32*)sub_start.get(), (const u16*)sub_mask.get(),
                                   (const u64*)rank_base.get(), xb, nr.prefix.get(), nr.start.get(), nr.bv.get());
            hipLaunchKernelGGL(k_popc_words, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, (const u64*)nr.bv.get(), popc.get());
            const u64 nb2 = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
            if (nb2 != nr.nb) throw Error(CBLX_EDEVICE, "prefix split: the runs hold " + std::to_string(nr.nb) + " buckets, the bitvector " + std::to_string(nb2) + " (internal error)");
            hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, nr.start.get() + nr.nb, N);
            CBLX_HIP(hipGetLastError());
            CBLX_HIP(hipStreamSynchronize(c->stream));  // the run tables are released here
        }
        dir_done = true;
    }
    if (lo == rec.lo2.get()) { std::swap(rec.lo, rec.lo2); std::swap(rec.hi, rec.hi2); }  // final data -> rec.lo/hi
    rec.lo2.reset();
    rec.hi2.reset();
    // -- KRN-4: bitvector, rank directory, bucket table (of the whole prefix space, or of the caller's window of it)
    if (!dir_done) {
        StageTimer t(c, ST_DIR);
        Buf<u32> popc(c->pool, nwords);
        u64* bvp;
        if (win) bvp = win->bv + (w_lo >> 6);
        else { nr.bv = Buf<u64>(c->pool, nwords); bvp = nr.bv.get(); CBLX_HIP(hipMemsetAsync(bvp, 0, nwords * 8, c->stream)); }
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        CBLX_HIP(hipMemsetAsync(popc.get(), 0, nwords * 4, c->stream));
        if (!have_dense) {  // boundaries from a scan of the sorted records (more groups than the table method takes)
            if (win) throw Error(CBLX_EINVAL, "a directory window needs PREFIX_BITS >= 9 (internal error)");
            CBLX_HIP(hipMemsetAsync(start_dense.get(), 0xFF, nprefix * 4, c->stream));
            if constexpr (DROP_HI)
                hipLaunchKernelGGL(k_boundaries_seg, grid1(ceil_div(N, 4), 256), dim3(256), 0, c->stream, lo, N, P.SB, RB, seg_start.get(), start_dense.get());
            else
                hipLaunchKernelGGL(k_boundaries<HiT>, grid1(ceil_div(N, 4), 256), dim3(256), 0, c->stream, lo, hi, N, P.SB, P.PB, start_dense.get());
        }
        if (nprefix) hipLaunchKernelGGL(k_bitvector, grid1(std::max<u64>(nprefix, 64), 256), dim3(256), 0, c->stream, start_dense.get(), nprefix, bvp, popc.get());
        nr.nb = nprefix ? exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get()) : 0;
        nr.prefix = Buf<u32>(c->pool, nr.nb + 1);
        nr.start = Buf<u64>(c->pool, nr.nb + 1);
        nr.cnt = Buf<u32>(c->pool, nr.nb + 1);
        nr.kind = Buf<u8>(c->pool, nr.nb + 1);
        if (nprefix) hipLaunchKernelGGL(k_bucket_table, grid1(nprefix, 256), dim3(256), 0, c->stream, start_dense.get(), nprefix, bvp, nr.rank_dir.get(), nr.prefix.get(), nr.start.get(), w_lo);
        hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, nr.start.get() + nr.nb, N);
        CBLX_HIP(hipGetLastError());
    }
}

// rows of k_merge_table's `other` side for a freshly partitioned batch: every run is a Vec of its raw length
__global__ void k_run_lengths(u64 nb, const u64* __restrict__ start, u32* __restrict__ cnt, u8* __restrict__ kind) {
    const u64 r = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nb) return;
    cnt[r] = (u32)(start[r + 1] - start[r]);
    kind[r] = KIND_VEC;
}

// One batch of N new words (rec, first n_pre slots unused = 0) into the index.
//   Empty index: partition + buckets, the sorted record array becomes the arena.
//   Non-empty index: only the NEW words are partitioned; the resident buckets are already grouped by prefix, so the merged
//   directory is the OR of the two bitvectors and every merged run = [resident suffixes as stored][new words of the
//   prefix] is gathered straight from the two arrays (the resident words are never expanded and re-partitioned).
template <typename C> void pipeline(cblx_ctx* c, Records& rec, u64 N, Buf<u32> countsA = Buf<u32>(), const PieceInput* pin = nullptr) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    Resident nb_;  // directory of the batch
    partition_and_directory<C>(c, rec, N, std::move(countsA), nb_, pin);
    auto adopt_arena = [&](Resident& nr) {
        nr.a_lo = std::move(rec.lo);
        if (WS) {  // arena hi lives in the records' hi buffer (u64 elements in this configuration)
            nr.a_hi.pool = rec.hi.pool; nr.a_hi.p = (u64*)rec.hi.p; nr.a_hi.n = rec.hi.n / 8;
            rec.hi.p = nullptr; rec.hi.n = 0;
        } else {
            rec.hi.reset();
        }
    };
    if (c->res.count == 0) {
        adopt_arena(nb_);
        bucket_stage<C>(c, nb_, c->res.view());
        c->res = std::move(nb_);
        return;
    }
    const Resident& s = c->res;
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    hipLaunchKernelGGL(k_run_lengths, grid1(nb_.nb, 256), dim3(256), 0, c->stream, nb_.nb, nb_.start.get(), nb_.cnt.get(), nb_.kind.get());
    adopt_arena(nb_);  // the sorted batch plays `other` in the gather below
    Resident nr;
    Buf<u32> raw, m_cs;
    Buf<u64> m_sstart, m_ostart;
    Buf<u8> m_skind, m_okind;
    u64 T = 0;
    {
        StageTimer t(c, ST_DIR);
        Buf<u32> popc(c->pool, nwords);
        nr.bv = Buf<u64>(c->pool, nwords);
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        hipLaunchKernelGGL(k_setop_bv, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, s.bv.get(), nb_.bv.get(), SETOP_OR, nr.bv.get(), popc.get());
        nr.nb = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
        const u64 nb = nr.nb;
        nr.prefix = Buf<u32>(c->pool, nb + 1);
        nr.start = Buf<u64>(c->pool, nb + 1);
        nr.cnt = Buf<u32>(c->pool, nb + 1);
        nr.kind = Buf<u8>(c->pool, nb + 1);
        raw = Buf<u32>(c->pool, nb + 1);
        m_cs = Buf<u32>(c->pool, nb + 1);
        m_sstart = Buf<u64>(c->pool, nb + 1);
        m_ostart = Buf<u64>(c->pool, nb + 1);
        m_skind = Buf<u8>(c->pool, nb + 1);
        m_okind = Buf<u8>(c->pool, nb + 1);
        hipLaunchKernelGGL(k_merge_table, grid1(nprefix, 256), dim3(256), 0, c->stream, nprefix, nr.bv.get(), nr.rank_dir.get(), s.view(), nb_.view(), nr.prefix.get(),
                           raw.get(), m_cs.get(), m_sstart.get(), m_ostart.get(), m_skind.get(), m_okind.get());
        T = exclusive_scan<u64>(c, raw.get(), nb, nr.start.get());
        hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, nr.start.get() + nb, T);
        CBLX_HIP(hipGetLastError());
    }
    if (T != s.count + N) throw Error(CBLX_EDEVICE, "insert: run lengths do not match the index and the batch (internal error)");
    nr.a_lo = Buf<u64>(c->pool, T + 2);
    if (WS) nr.a_hi = Buf<u64>(c->pool, T + 2);
    {
        StageTimer t(c, ST_EXPAND);
        with_lpb(T, nr.nb, [&](auto lpb) {
            constexpr int LPB = decltype(lpb)::value;
            hipLaunchKernelGGL((k_merge_gather<WS, LPB>), lpb_grid(nr.nb, LPB), dim3(256), 0, c->stream, nr.nb, nr.start.get(), m_cs.get(), m_sstart.get(), m_ostart.get(),
                               s.a_lo.get(), s.a_hi.get(), nb_.a_lo.get(), nb_.a_hi.get(), nr.a_lo.get(), nr.a_hi.get());
        });
        CBLX_HIP(hipGetLastError());
    }
    bucket_stage<C>(c, nr, s.view());
    CBLX_HIP(hipStreamSynchronize(c->stream));  // the batch and the table buffers are released at scope exit
    c->res = std::move(nr);
}

// ---- one GROUP of the grouped receiver (comm.hpp: sharded_insert_grouped) ----------------------------------------------------------
// The records of the group's prefix window lie in pieces of the receive log (pass A done by the senders; `pin` describes the group's
// share of every piece). They go through the LSD passes, the window's directory and the bucket kernels while later groups are still
// on the wire, and end up in the group's SLOT of the final arena (`fin`, the slot's first element); `scr` is a scratch area of at
// least N + 2 elements that plays the other ping-pong buffer (and the twin of the long-run path). Positions in `out.start` are
// relative to the slot. A non-owning Buf (pool = nullptr) stands for a region of somebody else's allocation.
template <typename T> Buf<T> alias_buf(T* p, size_t n) { Buf<T> b; b.pool = nullptr; b.p = p; b.n = n; return b; }
struct GroupRegions {
    const u64* log_lo = nullptr; const void* log_hi = nullptr;   // receive log (hi: words that keep their hi part behind pass A)
    u64* fin_lo = nullptr; u64* fin_hi = nullptr;                // the group's slot in the final arena (hi: 8-byte elements)
    u64* scr_lo = nullptr; u64* scr_hi = nullptr;                // scratch, >= N + 2 elements
};
template <typename C> void pipeline_group(cblx_ctx* c, const GroupRegions& R, const PieceInput& pin, u64 N, const DirWindow& win, Resident& out) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    constexpr bool DROP_HI = std::is_same<HiT, u8>::value;
    constexpr bool KEEP_HI = HiTraits<HiT>::has && !DROP_HI;  // 16-byte records through the LSD passes
    const Consts& P = c->P;
    const u32 npass = pin.sort_bits ? lsd_plan_bits(pin.sort_bits).total() : lsd_plan(P, false).total();  // buffer changes behind pass A (records in pieces: LSD passes only, no prefix split)
    // DEEP group (thousands of words per possible prefix: the dense low ranges of a many-GPU job at PREFIX_BITS <= 24): nearly every run
    // takes the long-run path, whose output is the twin — so the LSD passes end in the scratch area and the twin IS the slot.
    // (CBLX_GROUP_DEEP = 0 / 1 forces the choice: tests run small groups through both layouts)
    const char* deep_env = std::getenv("CBLX_GROUP_DEEP");
    const bool deep = msd_takes<WS>(P.SB) && (deep_env ? deep_env[0] == '1' : N / std::max<u64>(1, (u64)win.w_hi - win.w_lo) >= 2048);
    u64* last_lo = deep ? R.scr_lo : R.fin_lo;   // where the last LSD pass writes
    u64* last_hi = deep ? R.scr_hi : R.fin_hi;
    u64* oth_lo = deep ? R.fin_lo : R.scr_lo;
    u64* oth_hi = deep ? R.fin_hi : R.scr_hi;
    Records rec;
    rec.ext_lo = R.log_lo;
    rec.ext_hi = R.log_hi;
    // with an external source the passes write rec.lo, rec.lo2, rec.lo, ...: the last of `npass` lands in rec.lo iff npass is odd
    const bool last_is_first = (npass & 1u) != 0;
    rec.lo = alias_buf<u64>(last_is_first ? last_lo : oth_lo, N + 2);
    rec.lo2 = alias_buf<u64>(last_is_first ? oth_lo : last_lo, N + 2);
    if (KEEP_HI) {
        rec.hi = alias_buf<u8>((u8*)(last_is_first ? last_hi : oth_hi), (N + 2) * 8);
        rec.hi2 = alias_buf<u8>((u8*)(last_is_first ? oth_hi : last_hi), (N + 2) * 8);
    }
    partition_and_directory<C>(c, rec, N, Buf<u32>(), out, &pin, &win);
    if (rec.lo.get() != last_lo) throw Error(CBLX_EDEVICE, "grouped receiver: the last pass landed in the wrong buffer (internal error)");
    out.a_lo = alias_buf<u64>(last_lo, N + 2);
    if (WS) out.a_hi = alias_buf<u64>(last_hi, N + 2);
    Twin tw;
    tw.lo = alias_buf<u64>(oth_lo, N + 2);
    if (WS) tw.hi = alias_buf<u64>(oth_hi, N + 2);
    bucket_stage<C>(c, out, DirView{nullptr, nullptr, nullptr, nullptr, nullptr, 0}, &tw, deep ? 1 : 0);
    if (out.a_lo.get() != R.fin_lo) throw Error(CBLX_EDEVICE, "grouped receiver: a group did not end in its slot (internal error)");
    out.a_lo = Buf<u64>();  // the slot belongs to the final arena
    out.a_hi = Buf<u64>();
}

// record buffers (ping-pong) for a batch of n_new words
template <typename C> void begin_records(cblx_ctx* c, Records& rec, u64 n_new) {
    const size_t hs = hi_elem_size(c->P);
    rec.lo = Buf<u64>(c->pool, n_new + 2);
    rec.lo2 = Buf<u64>(c->pool, n_new + 2);
    rec.hi = Buf<u8>(c->pool, hs ? (n_new + 2) * hs : 8);
    rec.hi2 = Buf<u8>(c->pool, hs ? (n_new + 2) * hs : 8);
}

// KRN-1 front end: chunk table + validity + encode. Returns the number of new words written at rec[out_base..).
struct ChunkPlan {
    u64 nchunks = 0, n_kmers = 0, total_bases = 0;
    u32 ndirty = 0;
    u64 bias = 0;  // bytes skipped in front of the slice (multiple of 16)
    Buf<u64> chunk_start, kmer_off;
    Buf<u32> chunk_len, tile_first;
    Buf<u8> dirty;
    Buf<u32> dirty_list;  // the dirty chunks, any order (ndirty of them)
    // sequence -> chunk map: sequence s owns the chunks [seq_chunk[s], seq_chunk[s + 1]) (nseq + 1 entries). Kept only when the caller sets
    // keep_seq_chunk before the plan (the per-sequence query tallies); everyone else lets it die with the plan's temporaries.
    bool keep_seq_chunk = false;
    Buf<u64> seq_chunk;
    // Arithmetic plan (uniform_plan.hpp). A caller that reads the plan through encode() alone sets allow_uniform before the plan; plan_chunks
    // then probes the batch first and, for reads of one length without an invalid byte, sets `uni` and allocates no table at all.
    bool allow_uniform = false;
    UniformPlan uni;
};
inline bool uniform_plan_enabled() {  // read per call: tests switch it
    const char* e = std::getenv("CBLX_UNIFORM_PLAN");
    return !(e && e[0] == '0');
}
// what a SLICE of a plan needs (sequences [seq_a, seq_b) of the planned ones): its chunks, k-mers and tiles
struct PlanSlice { u64 c_lo = 0, c_hi = 0, k_lo = 0, k_hi = 0, t_lo = 0, t_hi = 0; };
__global__ void k_plan_marks(const u64* __restrict__ chunk_base, const u64* __restrict__ marks, u32 n, u64 nchunks, const u64* __restrict__ chunk_start, const u64* __restrict__ kmer_off,
                             u64* __restrict__ out /* [n][3]: chunk, its first k-mer, its first base */) {
    const u32 i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const u64 ch = chunk_base[marks[i]];
    out[3 * i] = ch;
    out[3 * i + 1] = kmer_off[ch];                     // (kmer_off[nchunks] = all k-mers)
    out[3 * i + 2] = ch < nchunks ? chunk_start[ch] : ~0ull;
}
// `ends`: offsets[0] and offsets[nseq] when the caller has read them already (each read is a host round trip)
// `B`: where the bases live (ASCII bytes, or the bit planes a big host batch crossed PCIe as); advanced to the slice's aligned start
// `seq_marks` / `slices`: sequence indices m[0] <= m[1] <= ... (relative to d_offsets) -> the slices [m[i], m[i+1]) of the plan, so that a caller
// that works slice by slice plans ONCE (a plan costs half a dozen host round trips)
// bases between the first and the last offset of a batch read back from the device
inline u64 offsets_span(u64 first, u64 last) {
    if (last < first) throw Error(CBLX_EINVAL, "offsets must be non-decreasing");
    return last - first;
}
// upper bound on the k-mers of sequences [n0, n1) of a batch: its bases less K - 1 per sequence
inline u64 kmers_upper_bound(cblx_ctx* c, const u64* d_offsets, u64 n0, u64 n1) {
    if (n1 <= n0) return 0;
    const u64 first = d2h<u64>(c, d_offsets + n0), last = d2h<u64>(c, d_offsets + n1);
    const u64 span = offsets_span(first, last), sub = (n1 - n0) * (u64)(c->P.K - 1);
    return span > sub ? span - sub : 0;
}
void plan_chunks(cblx_ctx* c, BaseView& d_bases, const u64* d_offsets, u64 nseq, ChunkPlan& pl, const u64* ends = nullptr, const std::vector<u64>* seq_marks = nullptr,
                 std::vector<PlanSlice>* slices = nullptr) {
    StageTimer t(c, ST_CHUNKS);
    const Consts& P = c->P;
    // offsets may start anywhere in the buffer (a slice of a larger batch): work relative to the 16-byte aligned
    // position below offsets[0] so that the tile grid and the validity scan cover only this slice
    u64 first, last;
    if (ends) { first = ends[0]; last = ends[1]; }
    else {  // one wait for the two
        ReadGroup rg(c);
        const size_t h_first = rg.add(d_offsets), h_last = rg.add(d_offsets + nseq);
        rg.wait();
        first = rg.get<u64>(h_first); last = rg.get<u64>(h_last);
    }
    pl.bias = first & ~(u64)15;
    pl.total_bases = offsets_span(first, last) + (first - pl.bias);
    d_bases.advance16(pl.bias);
    bool probed_clean = false;  // the probe ran and found every byte of the batch valid
    if (pl.allow_uniform && !pl.keep_seq_chunk && !seq_marks && nseq && uniform_plan_enabled()) {
        const u64 span = last - first, L = span / nseq;
        if (span % nseq == 0 && uniform_plan_shape(nseq, L, P.K, CHUNK_KMERS)) {  // (else some length differs, or the tables are needed: no probe)
            Buf<u32> flags(c->pool, 2);
            CBLX_HIP(hipMemsetAsync(flags.get(), 0, 8, c->stream));
            const u32 s0 = (u32)(first - pl.bias);
            hipLaunchKernelGGL(k_uniform_probe, grid1(std::max<u64>(nseq, ceil_div(pl.total_bases, 16)), 256), dim3(256), 0, c->stream, d_bases, pl.total_bases, s0, d_offsets, nseq, L,
                               flags.get());
            CBLX_HIP(hipGetLastError());
            const std::vector<u32> f = d2h_vec<u32>(c, flags.get(), 2);  // steers the work: tables or none
            if (!f[0] && !f[1]) {
                pl.uni.uniform = 1; pl.uni.L = (u32)L; pl.uni.nk0 = (u32)(L - P.K + 1); pl.uni.s0 = s0; pl.uni.n = nseq;
                pl.nchunks = nseq;
                pl.n_kmers = nseq * pl.uni.nk0;
                ++c->uniform_plans;
                return;
            }
            probed_clean = !f[1];
        }
    }
    Buf<u32> nch(c->pool, nseq + 1);
    Buf<u64> err(c->pool, 2), chunk_base(c->pool, nseq + 1);
    CBLX_HIP(hipMemsetAsync(err.get(), 0, 16, c->stream));
    hipLaunchKernelGGL(k_seq_chunk_count, grid1(nseq, 256), dim3(256), 0, c->stream, d_offsets, nseq, P.K, nch.get(), err.get());
    pl.nchunks = exclusive_scan<u64>(c, nch.get(), nseq, chunk_base.get());
    std::vector<u64> e = d2h_vec<u64>(c, err.get(), 2);
    if (e[0]) throw Error(CBLX_ESHORT, "Sequence size (" + std::to_string(e[1] - 1) + ") is smaller than K (" + std::to_string(P.K) + ")");
    if (pl.nchunks >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "too many chunks in one batch");
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, chunk_base.get() + nseq, pl.nchunks);
    pl.chunk_start = Buf<u64>(c->pool, pl.nchunks + 1);
    pl.chunk_len = Buf<u32>(c->pool, pl.nchunks + 1);
    Buf<u32> chunk_nk(c->pool, pl.nchunks + 1);
    pl.dirty = Buf<u8>(c->pool, pl.nchunks + 8);
    Buf<u32> ndirty(c->pool, 1);
    hipLaunchKernelGGL(k_chunk_fill, grid1(pl.nchunks, 256), dim3(256), 0, c->stream, d_offsets, chunk_base.get(), nseq, pl.nchunks, P.K, pl.bias,
                       pl.chunk_start.get(), pl.chunk_len.get(), chunk_nk.get());
    CBLX_HIP(hipMemsetAsync(pl.dirty.get(), 0, pl.nchunks + 8, c->stream));
    CBLX_HIP(hipMemsetAsync(ndirty.get(), 0, 4, c->stream));
    if (!probed_clean) {  // (the probe's scan covered the same bytes: nothing is dirty)
        hipLaunchKernelGGL(k_scan_invalid, grid1(ceil_div(pl.total_bases, 16), 256), dim3(256), 0, c->stream, d_bases, pl.total_bases,
                           pl.chunk_start.get(), pl.chunk_len.get(), pl.nchunks, pl.dirty.get(), ndirty.get());
        pl.ndirty = d2h<u32>(c, ndirty.get());  // a flag so far
    }
    if (pl.ndirty) {
        pl.dirty_list = Buf<u32>(c->pool, pl.nchunks + 1);
        CBLX_HIP(hipMemsetAsync(ndirty.get(), 0, 4, c->stream));
        hipLaunchKernelGGL(k_dirty_list, grid1(pl.nchunks, DIRTY_LIST_THREADS), dim3(DIRTY_LIST_THREADS), 0, c->stream, pl.dirty.get(), pl.nchunks, pl.dirty_list.get(), ndirty.get());
        pl.ndirty = d2h<u32>(c, ndirty.get());  // the number of dirty chunks
        hipLaunchKernelGGL(k_dirty_count_wave, dim3((pl.ndirty + 3) / 4), dim3(256), 0, c->stream, d_bases, pl.chunk_start.get(), pl.chunk_len.get(), pl.dirty_list.get(), pl.ndirty, P.K,
                           chunk_nk.get());
    }
    pl.kmer_off = Buf<u64>(c->pool, pl.nchunks + 1);
    pl.n_kmers = exclusive_scan<u64>(c, chunk_nk.get(), pl.nchunks, pl.kmer_off.get());
    hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, pl.kmer_off.get() + pl.nchunks, pl.n_kmers);
    const u64 ntiles = ceil_div(pl.total_bases, ENC_TILE_BYTES);
    pl.tile_first = Buf<u32>(c->pool, ntiles + 2);
    hipLaunchKernelGGL(k_tile_first_chunk, grid1(ntiles + 1, 256), dim3(256), 0, c->stream, pl.chunk_start.get(), pl.nchunks, ntiles, pl.tile_first.get());
    CBLX_HIP(hipGetLastError());
    if (seq_marks && slices) {
        const u32 nm = (u32)seq_marks->size();
        Buf<u64> d_marks(c->pool, nm), d_out(c->pool, 3 * (size_t)nm);
        h2d(c, d_marks.get(), seq_marks->data(), nm);
        hipLaunchKernelGGL(k_plan_marks, grid1(nm, 64), dim3(64), 0, c->stream, (const u64*)chunk_base.get(), (const u64*)d_marks.get(), nm, pl.nchunks, (const u64*)pl.chunk_start.get(),
                           (const u64*)pl.kmer_off.get(), d_out.get());
        const std::vector<u64> o = d2h_vec<u64>(c, d_out.get(), 3 * (size_t)nm);
        slices->assign(nm ? nm - 1 : 0, PlanSlice());
        for (u32 i = 0; i + 1 < nm; ++i) {
            PlanSlice& S = (*slices)[i];
            S.c_lo = o[3 * i]; S.c_hi = o[3 * (i + 1)]; S.k_lo = o[3 * i + 1]; S.k_hi = o[3 * (i + 1) + 1];
            if (S.c_hi > S.c_lo) {  // tiles of the base stream (4 KiB each) that hold the slice's chunk starts
                const std::vector<u64> last = d2h_vec<u64>(c, pl.chunk_start.get() + (S.c_hi - 1), 1);
                S.t_lo = o[3 * i + 2] / ENC_TILE_BYTES;
                S.t_hi = last[0] / ENC_TILE_BYTES + 1;
            }
        }
    }
    CBLX_HIP(hipStreamSynchronize(c->stream));  // temporaries (nch, err, chunk_base, chunk_nk, ndirty) die here
    if (pl.keep_seq_chunk) pl.seq_chunk = std::move(chunk_base);
}
void plan_chunks(cblx_ctx* c, const u8*& d_bases, const u64* d_offsets, u64 nseq, ChunkPlan& pl, const u64* ends = nullptr) {
    BaseView B = ascii_view(d_bases);
    plan_chunks(c, B, d_offsets, nseq, pl, ends);
    d_bases = B.ascii;
}
// `sl`: only that slice of the plan (its outputs start at out_base: k-mer k of the plan goes to out_base + k - sl->k_lo)
template <typename C> void encode(cblx_ctx* c, const BaseView& d_bases, const ChunkPlan& pl, u64* out_lo, typename C::HiT* out_hi, u64 out_base,
                                  EncHist eh = EncHist{}, const PlanSlice* sl = nullptr) {
    typedef typename C::HiT HiT;
    StageTimer t(c, ST_ENCODE);
    if (sl) {
        if (pl.uni.uniform) throw Error(CBLX_EDEVICE, "a slice of an arithmetic chunk plan (internal error)");
        if (sl->c_hi <= sl->c_lo) return;
        const u64 nt = sl->t_hi - sl->t_lo, ob = out_base - sl->k_lo;  // (modulo 2^64: the kernels add a chunk's k-mer offset back)
        hipLaunchKernelGGL((k_encode<C::WIDE, HiT>), dim3((unsigned)nt), dim3(ENC_THREADS), (eh.counts && eh.cut_tab) ? 8192 : 0, c->stream, d_bases, pl.total_bases, pl.chunk_start.get(),
                           pl.chunk_len.get(), pl.kmer_off.get(), pl.ndirty ? pl.dirty.get() : (const u8*)nullptr, pl.tile_first.get() + sl->t_lo, c->P, out_lo, out_hi, ob, eh, (u32)sl->c_lo,
                           (u32)sl->c_hi);
        if (pl.ndirty)
            hipLaunchKernelGGL((k_encode_dirty_wave<C::WIDE, HiT>), dim3((pl.ndirty + 3) / 4), dim3(256), 0, c->stream, d_bases, pl.chunk_start.get(), pl.chunk_len.get(),
                               pl.kmer_off.get(), pl.dirty_list.get(), pl.ndirty, c->P, out_lo, out_hi, ob, eh, (u32)sl->c_lo, (u32)sl->c_hi);
        CBLX_HIP(hipGetLastError());
        return;
    }
    const u64 ntiles = ceil_div(pl.total_bases, ENC_TILE_BYTES);
    if (ntiles)  // (dynamic LDS: the cut table of the fused histogram's bins, when there is one — 8 KB more per workgroup cost the kernel nothing, measured)
        hipLaunchKernelGGL((k_encode<C::WIDE, HiT>), dim3((unsigned)ntiles), dim3(ENC_THREADS), (eh.counts && eh.cut_tab) ? 8192 : 0, c->stream, d_bases, pl.total_bases, pl.chunk_start.get(),
                           pl.chunk_len.get(), pl.kmer_off.get(), pl.ndirty ? pl.dirty.get() : (const u8*)nullptr, pl.tile_first.get(), c->P, out_lo, out_hi, out_base, eh, 0u, 0xFFFFFFFFu,
                           pl.uni);
    if (pl.ndirty)
        hipLaunchKernelGGL((k_encode_dirty_wave<C::WIDE, HiT>), dim3((pl.ndirty + 3) / 4), dim3(256), 0, c->stream, d_bases, pl.chunk_start.get(), pl.chunk_len.get(),
                           pl.kmer_off.get(), pl.dirty_list.get(), pl.ndirty, c->P, out_lo, out_hi, out_base, eh);
    CBLX_HIP(hipGetLastError());
}
template <typename C> void encode(cblx_ctx* c, const u8* d_bases, const ChunkPlan& pl, u64* out_lo, typename C::HiT* out_hi, u64 out_base,
                                  EncHist eh = EncHist{}) {
    encode<C>(c, ascii_view(d_bases), pl, out_lo, out_hi, out_base, eh);
}

// ---- the FIRST partition pass of one piece of reads (a slice of a sharded build, a part of a peer's reads, a whole batch): KRN-1 with the
// pass's histogram fused in, the column prefixes, and the scatter on the digit the caller chose. The workspace lives until the stream is
// past the scatter (callers that queue the next piece's kernels meanwhile keep it in a `prev` of theirs). `coltot` (the 256 bin totals)
// stays on the device: the CALLER decides when it is read back — a read between KRN-1 and the scatter is a host round trip on the stream.
struct FirstPass {
    ChunkPlan pl;  // (the piece's own plan, where it has one)
    Buf<u64> t_lo;  // the words KRN-1 wrote ...
    Buf<u8> t_hi;
    Buf<u32> counts, colpre, scratch, adj, coltot;  // ... their count matrix [tile][256], its column prefixes, what the scatter adds, the bin totals
    u64 n = 0;
    u32 ntiles = 0;
};
inline void first_pass_prefixes(cblx_ctx* c, FirstPass& wk) {
    StageTimer t(c, ST_SCAN);
    colscan(c, wk.counts.get(), nullptr, wk.ntiles, wk.colpre.get(), wk.coltot.get(), wk.scratch);
    hipLaunchKernelGGL(k_seg_adjust, dim3(1), dim3(256), 0, c->stream, wk.colpre.get(), wk.coltot.get(), (const u32*)nullptr, (const u32*)nullptr,
                       (const u32*)nullptr, wk.ntiles, 1u, wk.adj.get());
}
// count: the N words of (a slice `sl` of) the plan into wk.t_lo / wk.t_hi, binned by `eh` (its `counts` is set here); N > 0
template <typename C> void first_pass_count(cblx_ctx* c, FirstPass& wk, const BaseView& bases, const ChunkPlan& pl, u64 N, EncHist eh, const PlanSlice* sl = nullptr) {
    typedef typename C::HiT HiT;
    const size_t hs = hi_elem_size(c->P);
    wk.n = N;
    wk.ntiles = (u32)ceil_div(N, RDX_TILE);
    wk.coltot = Buf<u32>(c->pool, 256); wk.adj = Buf<u32>(c->pool, 256);
    wk.t_lo = Buf<u64>(c->pool, N + 2); wk.t_hi = Buf<u8>(c->pool, hs ? (N + 2) * hs : 8);
    wk.counts = Buf<u32>(c->pool, (size_t)256 * (wk.ntiles + 2)); wk.colpre = Buf<u32>(c->pool, (size_t)256 * wk.ntiles);
    CBLX_HIP(hipMemsetAsync(wk.counts.get(), 0, (size_t)256 * (wk.ntiles + 2) * 4, c->stream));
    eh.counts = wk.counts.get();
    encode<C>(c, bases, pl, wk.t_lo.get(), (HiT*)wk.t_hi.get(), 0, eh, sl);
    first_pass_prefixes(c, wk);
    CBLX_HIP(hipGetLastError());
}
// scatter of `lo` / `hi` (wk.n records: the words of first_pass_count, or a caller's) by `fn`. REDIR: positions [ow.a, ow.b) of the output
// order go to the own window's arrays, the rest closes up in out_* (null: dropped). `tally`: the records count as a pass of a build.
template <typename HiT, typename OutH, typename Fn, bool REDIR = false>
void first_pass_scatter(cblx_ctx* c, const FirstPass& wk, const u64* lo, const HiT* hi, const Fn& fn, u64* out_lo, OutH* out_hi, bool tally = false,
                        DigitBits nextd = DigitBits{0, 0}, u8* out_next = nullptr, OwnWindow ow = OwnWindow{0, 0, nullptr, nullptr, nullptr}) {
    const TileView tv{nullptr, nullptr, nullptr, nullptr, wk.ntiles, wk.n};
    StageTimer t(c, ST_SCATTER);
    if (tally) c->stages[ST_SCATTER].units += wk.n;
    hipLaunchKernelGGL((k_radix_scatter<HiT, OutH, Fn, REDIR>), dim3(xcd_grid(wk.ntiles)), dim3(RDX_THREADS), 0, c->stream, lo, hi, tv, fn, (const u32*)wk.colpre.get(),
                       (const u32*)wk.adj.get(), out_lo, out_hi, nextd, out_next, (u32*)nullptr, 0u, 0u, 0u, (u32*)nullptr, 0u, ow);
    CBLX_HIP(hipGetLastError());
}

void check_aligned16(const void* p, const char* what) {
    if (((uintptr_t)p) & 15) throw Error(CBLX_EINVAL, std::string(what) + " must be 16-byte aligned");
}

// One call of the kernels takes fewer than 2^32 words (32-bit positions inside a batch: tile tables, start_dense). A larger
// insert is cut at sequence boundaries into sub-batches that go in one after the other: the result is the same (batch
// boundaries do not change what an insert-only history builds), the resident index itself has
// 64-bit positions throughout. CBLX_BATCH_MAX_BASES overrides the cut (tests use a tiny value).
u64 batch_max_bases() {
    const char* e = std::getenv("CBLX_BATCH_MAX_BASES");
    const u64 x = e ? std::strtoull(e, nullptr, 10) : 0;
    return x ? x : (1ull << 31);
}
void insert_device_one(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, const u64* ends = nullptr);
// PREFIX_BITS > 24 on an empty index: the build on FINE bins (comm.hpp; false = not taken, nothing was touched)
bool insert_device_fine(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq);
void insert_device(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq) {
    if (nseq == 0) return;
    check_aligned16(d_bases, "d_bases");
    const u64 cap = batch_max_bases();
    ReadGroup rg(c);  // first + last: one wait
    const size_t h_first = rg.add(d_offsets), h_last = rg.add(d_offsets + nseq);
    rg.wait();
    const u64 first = rg.get<u64>(h_first), last = rg.get<u64>(h_last);
    if (offsets_span(first, last) <= cap) {
        const u64 ends[2] = {first, last};
        insert_device_one(c, d_bases, d_offsets, nseq, ends);
        return;
    }
    u64 a = 0, oa = first;
    while (a < nseq) {
        u64 lo = a + 1, hi = nseq;  // largest b in [a + 1, nseq] with offsets[b] - oa <= cap (a + 1 if even one sequence is longer)
        if (d2h<u64>(c, d_offsets + hi) - oa <= cap) lo = hi;
        else {
            while (hi - lo > 1) {  // offsets[hi] - oa > cap
                const u64 mid = lo + (hi - lo) / 2;
                if (d2h<u64>(c, d_offsets + mid) - oa <= cap) lo = mid; else hi = mid;
            }
        }
        insert_device_one(c, d_bases, d_offsets + a, lo - a);
        a = lo;
        oa = d2h<u64>(c, d_offsets + a);
    }
}
void insert_device_one(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, const u64* ends) {
    if (c->res.count == 0 && c->P.PB > 24 && insert_device_fine(c, d_bases, d_offsets, nseq)) { collect_events(c); return; }
    dispatch(c->P, [&](auto cfg) {
        typedef decltype(cfg) C;
        ChunkPlan pl;
        pl.allow_uniform = true;  // the plan is read by encode() alone
        plan_chunks(c, d_bases, d_offsets, nseq, pl, ends);
        if (pl.n_kmers == 0) return;
        if (pl.n_kmers >= 0xFFFFFFF0ull) throw Error(CBLX_ERANGE, "one sequence of 2^32-16 k-mers or more is not supported");
        Records rec;
        begin_records<C>(c, rec, pl.n_kmers);
        const u64 base = 0;
        Buf<u32> countsA;
        EncHist eh{};
        {   // KRN-1 also accumulates the first partition pass's tile histogram
            static_assert(ENC_HIST_WINDOW == RDX_TILE, "fused histogram windows must be the partition tiles");
            const size_t ntmax = (size_t)ceil_div(pl.n_kmers, RDX_TILE) + 256;
            countsA = Buf<u32>(c->pool, 256 * ntmax);
            CBLX_HIP(hipMemsetAsync(countsA.get(), 0, 256 * ntmax * 4, c->stream));
            const u32 nA = std::min(8u, c->P.PB);
            eh.counts = countsA.get();
            eh.shift = c->P.SB + (c->P.PB - nA);
            eh.nbits = nA;
        }
        encode<C>(c, d_bases, pl, rec.lo.get(), (typename C::HiT*)rec.hi.get(), base, eh);
        pipeline<C>(c, rec, base + pl.n_kmers, std::move(countsA));
        c->kmers_inserted += pl.n_kmers;
    });
    collect_events(c);
}

// ---- sorted batches (multi-GPU build, include/cblx.h) -------------------------------------------------------------
// sender: KRN-1 + the full partition of the words of nseq sequences; the batch stays in c->batch
template <typename C> void sorted_batch_begin(cblx_ctx* c, const u8* d_bases, const u64* d_offsets, u64 nseq, const u32* bounds, u32 nd, u64* bucket_split,
                                              u64* word_split) {
    c->batch = SortedBatch();
    for (u32 d = 0; d <= nd; ++d) bucket_split[d] = word_split[d] = 0;
    if (nseq == 0) return;
    ChunkPlan pl;
    plan_chunks(c, d_bases, d_offsets, nseq, pl);
    if (pl.n_kmers == 0) return;
    const u64 N = pl.n_kmers;
    Records rec;
    begin_records<C>(c, rec, N);
    const size_t ntmax = (size_t)ceil_div(N, RDX_TILE) + 256;
    Buf<u32> countsA(c->pool, 256 * ntmax);
    CBLX_HIP(hipMemsetAsync(countsA.get(), 0, 256 * ntmax * 4, c->stream));
    const u32 nA = std::min(8u, c->P.PB);
    EncHist eh{};
    eh.counts = countsA.get();
    eh.shift = c->P.SB + (c->P.PB - nA);
    eh.nbits = nA;
    encode<C>(c, d_bases, pl, rec.lo.get(), (typename C::HiT*)rec.hi.get(), 0, eh);
    Resident dir;
    partition_and_directory<C>(c, rec, N, std::move(countsA), dir);
    SortedBatch& b = c->batch;
    b.n = N;
    b.nb = dir.nb;
    b.prefix = std::move(dir.prefix);
    b.start = std::move(dir.start);
    b.lo = std::move(rec.lo);
    b.hi = std::move(rec.hi);
    bucket_split[nd] = b.nb;
    word_split[nd] = N;
    if (nd > 1) {
        Buf<u32> d_bounds(c->pool, nd);
        Buf<u64> d_bs(c->pool, nd), d_ws(c->pool, nd);
        h2d(c, d_bounds.get(), bounds, nd - 1);
        hipLaunchKernelGGL(k_batch_split, grid1(nd - 1, 64), dim3(64), 0, c->stream, b.nb, b.prefix.get(), b.start.get(), nd - 1, d_bounds.get(), d_bs.get(), d_ws.get());
        CBLX_HIP(hipGetLastError());
        std::vector<u64> bs = d2h_vec<u64>(c, d_bs.get(), nd - 1), ws = d2h_vec<u64>(c, d_ws.get(), nd - 1);
        for (u32 d = 1; d < nd; ++d) { bucket_split[d] = bs[d - 1]; word_split[d] = ws[d - 1]; }
    }
    CBLX_HIP(hipStreamSynchronize(c->stream));
}
template <typename C> void sorted_batch_export(cblx_ctx* c, u32* d_prefix, u32* d_count, u8* d_suffix) {
    typedef typename C::HiT HiT;
    SortedBatch& b = c->batch;
    if (b.nb) {
        CBLX_HIP(hipMemcpyAsync(d_prefix, b.prefix.get(), b.nb * 4, hipMemcpyDeviceToDevice, c->stream));
        hipLaunchKernelGGL(k_batch_counts, grid1(b.nb, 256), dim3(256), 0, c->stream, b.nb, b.start.get(), d_count);
        // the hi part matters only for suffixes wider than 64 bits (then it was carried through every pass)
        hipLaunchKernelGGL((k_batch_pack<C::WS, HiT>), dim3((unsigned)ceil_div(b.n, PACK_TILE)), dim3(PACK_THREADS), (size_t)PACK_TILE * c->P.BYTES, c->stream, b.n, b.lo.get(),
                           C::WS ? (const HiT*)b.hi.get() : (const HiT*)nullptr, c->P.SB, c->P.BYTES, d_suffix);
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));
    }
    c->batch = SortedBatch();
}
// receiver: WordSet::insert_batch over sorted batches, stream order = batch order; the resident index (if any) comes first
template <typename C> void insert_sorted_batches(cblx_ctx* c, const cblx_batch_view* bt, u32 nbt) {
    typedef typename C::HiT HiT;
    constexpr bool WS = C::WS;
    const Consts& P = c->P;
    const Resident& s = c->res;
    u64 add = 0;
    for (u32 b = 0; b < nbt; ++b) {
        if (bt[b].n_buckets && (!bt[b].d_prefix || !bt[b].d_count)) throw Error(CBLX_EINVAL, "null batch arrays");
        if (bt[b].n_words && !bt[b].d_suffix) throw Error(CBLX_EINVAL, "null batch suffixes");
        add += bt[b].n_words;
    }
    if (add == 0) return;
    const u64 nprefix = 1ull << P.PB, nwords = std::max<u64>(1, nprefix / 64);
    Resident nr;
    Buf<u32> raw, m_cs, bad(c->pool, 1);
    Buf<u64> m_sstart, m_ostart;
    Buf<u8> m_skind, m_okind;
    std::vector<Buf<u32>> off_in_run(nbt);
    std::vector<Buf<u64>> src_off(nbt);
    u64 T = 0;
    {
        StageTimer t(c, ST_DIR);
        Buf<u32> popc(c->pool, nwords);
        nr.bv = Buf<u64>(c->pool, nwords);
        nr.rank_dir = Buf<u64>(c->pool, nwords + 1);
        if (s.count) CBLX_HIP(hipMemcpyAsync(nr.bv.get(), s.bv.get(), nwords * 8, hipMemcpyDeviceToDevice, c->stream));
        else CBLX_HIP(hipMemsetAsync(nr.bv.get(), 0, nwords * 8, c->stream));
        CBLX_HIP(hipMemsetAsync(bad.get(), 0, 4, c->stream));
        for (u32 b = 0; b < nbt; ++b)
            if (bt[b].n_buckets)
                hipLaunchKernelGGL(k_batch_bits, grid1(bt[b].n_buckets, 256), dim3(256), 0, c->stream, bt[b].n_buckets, bt[b].d_prefix, bt[b].d_count, nprefix, nr.bv.get(), bad.get());
        hipLaunchKernelGGL(k_popc_words, grid1(nwords, 256), dim3(256), 0, c->stream, nwords, nr.bv.get(), popc.get());
        nr.nb = exclusive_scan<u64>(c, popc.get(), nwords, nr.rank_dir.get());
        if (d2h<u32>(c, bad.get())) throw Error(CBLX_EINVAL, "sorted batch: prefixes must be strictly ascending and below 2^PREFIX_BITS, counts non-zero");
        const u64 nb = nr.nb;
        nr.prefix = Buf<u32>(c->pool, nb + 1);
        nr.start = Buf<u64>(c->pool, nb + 1);
        nr.cnt = Buf<u32>(c->pool, nb + 1);
        nr.kind = Buf<u8>(c->pool, nb + 1);
        raw = Buf<u32>(c->pool, nb + 1);
        m_cs = Buf<u32>(c->pool, nb + 1);
        m_sstart = Buf<u64>(c->pool, nb + 1);
        m_ostart = Buf<u64>(c->pool, nb + 1);
        m_skind = Buf<u8>(c->pool, nb + 1);
        m_okind = Buf<u8>(c->pool, nb + 1);
        // the resident part of every merged run (raw = its length), then batch after batch on top of it
        hipLaunchKernelGGL(k_merge_table, grid1(nprefix, 256), dim3(256), 0, c->stream, nprefix, nr.bv.get(), nr.rank_dir.get(), s.view(), DirView{}, nr.prefix.get(),
                           raw.get(), m_cs.get(), m_sstart.get(), m_ostart.get(), m_skind.get(), m_okind.get());
        for (u32 b = 0; b < nbt; ++b) {
            if (!bt[b].n_buckets) continue;
            off_in_run[b] = Buf<u32>(c->pool, bt[b].n_buckets);
            src_off[b] = Buf<u64>(c->pool, bt[b].n_buckets + 1);
            hipLaunchKernelGGL(k_batch_offsets, grid1(bt[b].n_buckets, 256), dim3(256), 0, c->stream, bt[b].n_buckets, bt[b].d_prefix, bt[b].d_count, nr.bv.get(),
                               nr.rank_dir.get(), raw.get(), off_in_run[b].get());
            const u64 nw = exclusive_scan<u64>(c, bt[b].d_count, bt[b].n_buckets, src_off[b].get());
            if (nw != bt[b].n_words) throw Error(CBLX_EINVAL, "sorted batch: n_words does not match the counts");
        }
        T = exclusive_scan<u64>(c, raw.get(), nb, nr.start.get());
        hipLaunchKernelGGL(k_set_u64, dim3(1), dim3(1), 0, c->stream, nr.start.get() + nb, T);
        CBLX_HIP(hipGetLastError());
    }
    if (T != s.count + add) throw Error(CBLX_EDEVICE, "sorted batches: run lengths do not add up (internal error)");
    nr.a_lo = Buf<u64>(c->pool, T + 2);
    if (WS) nr.a_hi = Buf<u64>(c->pool, T + 2);
    {
        StageTimer t(c, ST_EXPAND);
        if (s.count)
            with_lpb(s.count, s.nb, [&](auto lpb) {
                constexpr int LPB = decltype(lpb)::value;
                hipLaunchKernelGGL((k_gather_resident<WS, LPB>), lpb_grid(nr.nb, LPB), dim3(256), 0, c->stream, nr.nb, nr.start.get(), m_cs.get(), m_sstart.get(),
                                   s.a_lo.get(), s.a_hi.get(), nr.a_lo.get(), nr.a_hi.get());
            });
        std::vector<Buf<u64>> dst(nbt);  // released after the bucket stage below has synchronised
        for (u32 b = 0; b < nbt; ++b) {
            if (!bt[b].n_buckets) continue;
            dst[b] = Buf<u64>(c->pool, bt[b].n_buckets);
            hipLaunchKernelGGL(k_batch_dst, grid1(bt[b].n_buckets, 256), dim3(256), 0, c->stream, bt[b].n_buckets, bt[b].d_prefix, off_in_run[b].get(), nr.bv.get(),
                               nr.rank_dir.get(), nr.start.get(), dst[b].get());
            with_lpb(bt[b].n_words, bt[b].n_buckets, [&](auto lpb) {
                constexpr int LPB = decltype(lpb)::value;
                hipLaunchKernelGGL((k_gather_packed<WS, LPB>), lpb_grid(bt[b].n_buckets, LPB), dim3(256), 0, c->stream, bt[b].n_buckets, bt[b].d_count, src_off[b].get(),
                                   dst[b].get(), bt[b].d_suffix, bt[b].n_words * P.BYTES, P.BYTES, nr.a_lo.get(), nr.a_hi.get());
            });
        }
        CBLX_HIP(hipGetLastError());
        CBLX_HIP(hipStreamSynchronize(c->stream));
        CBLX_HIP(hipGetLastError());
    }
    bucket_stage<C>(c, nr, s.view());
    CBLX_HIP(hipStreamSynchronize(c->stream));
    c->res = std::move(nr);
    c->kmers_inserted += add;
}

}  // namespace
