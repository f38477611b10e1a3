// wire_layout.hpp — layout arithmetic of the "bins" protocols (comm.hpp): from the 256 bin totals of a sender's first pass to the
// per-destination header of the count exchange, the ranges of a send buffer, and the receiver's groups and piece tables. Pure
// host code over the plans of cuts.hpp, no HIP in here: tests/host/wire_layout_unit.cpp builds it with g++ and checks it against a
// record-by-record assignment of words to (destination, group, segment).
#pragma once
#include <string>

#include "cuts.hpp"
#include "error.hpp"

namespace cblx {

static const u32 NO_BIN = 0xFFFFFFFFu;
static const size_t WIRE_HDR = 257;  // header of the count exchange, per destination: words, then words per segment / cell of its range
static const int WIRE_EINTERNAL = 4;  // CBLX_EDEVICE (include/cblx.h)

// The bins of sharded_insert_bins (DigitBin): the pass-A segment refined by the destination rank.
struct BinMap {
    u32 v_of[256], d_of[256];  // bin -> segment, destination (0xFFFFFFFF: no such bin)
    bool ok = true;
};
inline BinMap make_bin_map(u32 PB, const u32* bounds, u32 W) {
    BinMap M;
    for (u32 i = 0; i < 256; ++i) M.v_of[i] = M.d_of[i] = NO_BIN;
    const u32 RB = PB - 8;
    auto dest = [&](u64 p) { u32 d = 0; for (u32 i = 0; i + 1 < W; ++i) d += bounds[i] <= p ? 1u : 0u; return d; };
    for (u32 i = 0; i + 1 < W; ++i) if ((u64)bounds[i] > (255ull << RB)) M.ok = false;  // the all-ones segment must belong to one rank
    for (u32 v = 0; v < 128; ++v)
        for (u32 d = dest((u64)v << RB); d <= dest((((u64)v + 1) << RB) - 1); ++d) { M.v_of[v + d] = v; M.d_of[v + d] = d; }
    M.v_of[255] = 255; M.d_of[255] = W - 1;
    return M;
}

// What the header needs of a map: is the bin one a prefix maps to, whose it is, and which entry of its owner's header row counts it
// (BinMap: the segment; CutPlan / FinePlan: the cell = the bin's number inside the owner's consecutive bins).
inline bool bin_mapped(const BinMap& M, u32 bin) { return M.v_of[bin] != NO_BIN; }
inline u32 bin_dest(const BinMap& M, u32 bin) { return M.d_of[bin]; }
inline u32 bin_slot(const BinMap& M, u32 bin) { return M.v_of[bin]; }
inline bool bin_mapped(const CutPlan& M, u32 bin) { return M.iv_of[bin] != NO_BIN; }
inline u32 bin_dest(const CutPlan& M, u32 bin) { return M.dest_of[M.iv_of[bin]]; }
inline u32 bin_slot(const CutPlan& M, u32 bin) { return bin - M.bin_lo[bin_dest(M, bin)]; }

// Bin totals of one first pass over N words -> the header rows send[W][WIRE_HDR] (added to: the caller zeroes them). Returns where
// the own rank's records lie in the pass's output order: [a, a + n). `what`: "slice" or "piece" (the text of the count check).
struct OwnShare { u64 a = 0, n = 0; };
template <typename Map>
OwnShare wire_header(const Map& M, const u32* tot, u32 W, u32 me, u64 N, const char* what, u64* send) {
    for (u32 bin = 0; bin < 256; ++bin) {
        if (!tot[bin]) continue;
        if (!bin_mapped(M, bin)) throw Error(WIRE_EINTERNAL, "sharded build: a word fell into a bin no prefix maps to (internal error)");
        const u32 d = bin_dest(M, bin);
        send[(size_t)d * WIRE_HDR] += tot[bin];
        send[(size_t)d * WIRE_HDR + 1 + bin_slot(M, bin)] += tot[bin];
    }
    u64 sum = 0;
    for (u32 d = 0; d < W; ++d) sum += send[(size_t)d * WIRE_HDR];
    if (sum != N)
        throw Error(WIRE_EINTERNAL, "sharded build: the bin histogram counts " + std::to_string(sum) + " words, the " + what + " has " + std::to_string(N) + " (internal error)");
    OwnShare own;
    for (u32 d = 0; d < me; ++d) own.a += send[(size_t)d * WIRE_HDR];
    own.n = send[(size_t)me * WIRE_HDR];
    return own;
}

// records in front of / inside entries [c0, c1) of a row of counts
inline void count_range(const u32* cnt, u32 c0, u32 c1, u64& before, u64& inside) {
    before = inside = 0;
    for (u32 i = 0; i < c1; ++i) (i < c0 ? before : inside) += cnt[i];
}
// record range [first, first + len) of bins [b0, b1) in a slice's send buffer (the own window is not in it)
inline void send_range(const u32* tot, const OwnShare& own, u32 b0, u32 b1, u64& first, u64& len) {
    u64 before;
    count_range(tot, b0, b1, before, len);
    first = before >= own.a + own.n ? before - own.n : before;  // ranges of other ranks lie wholly before or behind the own window
}
// bins [b0, b1) of (rank d, group k); b0 >= b1: none
inline void group_bins(const CutPlan& M, u32 d, u32 k, u32& b0, u32& b1) {
    b0 = 256; b1 = 0;
    for (u32 bin = M.bin_lo[d]; bin < M.bin_lo[d + 1]; ++bin)
        if (M.iv_of[bin] != NO_BIN && M.grp_of[M.iv_of[bin]] == k) { b0 = std::min(b0, bin); b1 = std::max(b1, bin + 1); }
}
// cells (= bins of the rank, counted from its first) of every one of a rank's groups: group g = cells [gc0[g], gc0[g + 1])
// (a cut that falls exactly on a segment boundary leaves one bin number unused: such a cell holds nothing and belongs nowhere)
inline std::vector<u32> group_cells(const CutPlan& M, u32 me) {
    const u32 my_lo = M.bin_lo[me], my_cells = M.bin_lo[me + 1] - M.bin_lo[me], NG = M.ngroups[me];
    std::vector<u32> gc0(NG + 1, my_cells);
    for (u32 cl = my_cells; cl-- > 0;) if (M.iv_of[my_lo + cl] != NO_BIN) gc0[M.grp_of[M.iv_of[my_lo + cl]]] = cl;
    for (int g = (int)NG - 1; g >= 0; --g) if (gc0[g] > gc0[g + 1]) gc0[g] = gc0[g + 1];
    return gc0;
}
// The pieces of one slice in the log, from the header rows recv[W][WIRE_HDR] the sources sent: the own piece first (the first pass writes it
// there), then the other sources in rank order; the piece table keeps the logical order (slice-major, source-minor).
inline void push_pieces(const u64* recv, u32 W, u32 me, u64 filled, u64 own, std::vector<u32>& pbase, std::vector<u32>& pcnt) {
    u64 ro = 0;  // records of other sources behind the own piece
    for (u32 r = 0; r < W; ++r) {
        pbase.push_back((u32)(r == me ? filled : filled + own + ro));
        if (r != me) ro += recv[(size_t)r * WIRE_HDR];
        for (u32 cl = 0; cl < 256; ++cl) pcnt.push_back((u32)recv[(size_t)r * WIRE_HDR + 1 + cl]);
    }
}
// One group's share of every piece of the log: counts per SEGMENT (inside a group a segment occurs in one cell only) and the
// group's first record in the piece. pcnt[piece][256]: records per cell; seg_of_cell: the rank's cells -> segment (CutPlan::v_of or
// FinePlan::seg_of, from the rank's first bin on).
inline void group_piece_table(const u32* seg_of_cell, u32 c0, u32 c1, const std::vector<u32>& pcnt, const std::vector<u32>& pbase, std::vector<u32>& cnt_g, std::vector<u32>& pb_g) {
    const size_t np = pbase.size();
    cnt_g.assign(np * 256, 0u);
    pb_g.assign(np, 0u);
    for (size_t p = 0; p < np; ++p) {
        u64 before = 0;
        for (u32 cl = 0; cl < c0; ++cl) before += pcnt[p * 256 + cl];
        pb_g[p] = (u32)(pbase[p] + before);
        for (u32 cl = c0; cl < c1; ++cl) {
            const u32 v = seg_of_cell[cl];
            if (v == NO_BIN) { if (pcnt[p * 256 + cl]) throw Error(WIRE_EINTERNAL, "grouped receiver: words in a bin no prefix maps to (internal error)"); continue; }
            if (cnt_g[p * 256 + v] && pcnt[p * 256 + cl]) throw Error(WIRE_EINTERNAL, "grouped receiver: a segment occurs in two cells of one group (internal error)");
            cnt_g[p * 256 + v] += pcnt[p * 256 + cl];
        }
    }
}

}  // namespace cblx
