// Host-side unit check of cbl_amd/csrc/wire_layout.hpp (no HIP): the layout arithmetic of the "bins" protocols against a record-by-record
// brute force. Random rank bounds and group cuts for W in {1, 2, 3, 8} at PREFIX_BITS in {9, 12, 24, 25, 28}; plans from make_bin_map,
// make_cut_plan and make_fine_plan; random words (prefixes), every one assigned to (destination, group, segment) by plain counting of the
// bounds and cuts. Checked: header rows sum to N, own offset and count, the send ranges of all (destination, group) pairs are disjoint and
// tile the send buffer, the groups' cell ranges partition the rank's cells, the groups' piece tables add up to the log's and agree with the
// brute force segment by segment, and a total in an unmapped bin (or a wrong word count) raises the internal error.
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <random>

#include "../../cbl_amd/csrc/wire_layout.hpp"

using namespace cblx;

static long bad = 0;
#define CHECK(c, ...) do { if (!(c)) { ++bad; if (bad < 20) { printf(__VA_ARGS__); printf("\n"); } } } while (0)

struct Word { u32 bin, dest, grp, seg; };
// what a plan says of a prefix, by definition (counting bounds and cuts)
struct Scheme {
    const char* name;
    u32 PB, W;
    const CutPlan* plan;  // null: the BinMap (one group per rank)
    std::function<Word(u32)> word;
};

template <typename Map> static bool raises(const Map& M, const u32* tot, u32 W, u32 me, u64 N) {
    std::vector<u64> send((size_t)W * WIRE_HDR, 0);
    try { wire_header(M, tot, W, me, N, "slice", send.data()); } catch (const Error& e) { return e.code == 4; }
    return false;
}

template <typename Map> static void check_scheme(const Scheme& S, const Map& M, std::mt19937_64& rnd, const u32* seg_of_bin) {
    const u32 W = S.W, PB = S.PB;
    const u32 NP = 3;  // pieces: three senders' first passes over random words
    std::vector<std::vector<Word>> piece(NP);
    std::vector<std::vector<u32>> tots(NP, std::vector<u32>(256, 0u));
    for (u32 p = 0; p < NP; ++p) {
        const u32 nw = 1 + rnd() % 4000;
        for (u32 i = 0; i < nw; ++i) {
            u32 x = (u32)((rnd() % (1ull << (PB - 1))) >> (rnd() % PB));
            if (rnd() % 97 == 0) x = (u32)((1ull << PB) - 1);  // the all-ones word
            const Word w = S.word(x);
            CHECK(w.bin < 256 && w.dest < W, "%s: word of prefix %u: bin %u dest %u", S.name, x, w.bin, w.dest);
            piece[p].push_back(w);
            tots[p][w.bin]++;
        }
        // the pass's output order: by bin (stable)
        std::stable_sort(piece[p].begin(), piece[p].end(), [](const Word& a, const Word& b) { return a.bin < b.bin; });
        for (size_t i = 1; i < piece[p].size(); ++i)
            CHECK(piece[p][i - 1].dest <= piece[p][i].dest && (piece[p][i - 1].dest != piece[p][i].dest || piece[p][i - 1].grp <= piece[p][i].grp), "%s: bins do not ascend with (rank, group)", S.name);
    }
    for (u32 me = 0; me < W; ++me) {
        std::vector<u32> pcnt, pbase;  // the receiver's log: one piece per sender
        u32 at = 17;
        for (u32 p = 0; p < NP; ++p) {
            const std::vector<Word>& ws = piece[p];
            const u64 N = ws.size();
            std::vector<u64> send((size_t)W * WIRE_HDR, 0);
            const OwnShare own = wire_header(M, tots[p].data(), W, me, N, "slice", send.data());
            // header rows against the brute force
            u64 sum = 0, own_a = N, own_n = 0;
            std::vector<u64> per_dest(W, 0);
            for (size_t i = 0; i < ws.size(); ++i) { per_dest[ws[i].dest]++; if (ws[i].dest == me) { own_a = std::min<u64>(own_a, i); ++own_n; } }
            for (u32 d = 0; d < W; ++d) {
                sum += send[(size_t)d * WIRE_HDR];
                u64 slots = 0;
                for (u32 v = 0; v < 256; ++v) slots += send[(size_t)d * WIRE_HDR + 1 + v];
                CHECK(send[(size_t)d * WIRE_HDR] == per_dest[d] && slots == per_dest[d], "%s: header row of rank %u: %llu / %llu, brute force %llu", S.name, d,
                      (unsigned long long)send[(size_t)d * WIRE_HDR], (unsigned long long)slots, (unsigned long long)per_dest[d]);
            }
            CHECK(sum == N, "%s: header rows sum to %llu of %llu", S.name, (unsigned long long)sum, (unsigned long long)N);
            CHECK(own.n == own_n && (own_n == 0 || own.a == own_a), "%s: own share [%llu, +%llu), brute force [%llu, +%llu)", S.name, (unsigned long long)own.a, (unsigned long long)own.n,
                  (unsigned long long)own_a, (unsigned long long)own_n);
            // send ranges of every (destination, group): the send buffer = the records of other ranks in output order
            std::vector<Word> buf;
            for (const Word& w : ws) if (w.dest != me) buf.push_back(w);
            std::vector<std::pair<u64, u64>> ranges;
            for (u32 d = 0; d < W; ++d) {
                if (d == me) continue;
                const u32 ng = S.plan ? S.plan->ngroups[d] : 1u;
                for (u32 k = 0; k < ng; ++k) {
                    u32 b0 = 256, b1 = 0;
                    if (S.plan) group_bins(*S.plan, d, k, b0, b1);
                    else for (u32 bin = 0; bin < 256; ++bin) if (bin_mapped(M, bin) && bin_dest(M, bin) == d) { b0 = std::min(b0, bin); b1 = std::max(b1, bin + 1); }
                    if (b0 >= b1) continue;
                    u64 first, len;
                    send_range(tots[p].data(), own, b0, b1, first, len);
                    CHECK(first + len <= buf.size(), "%s: send range past the buffer", S.name);
                    for (u64 i = first; i < first + len && i < buf.size(); ++i) CHECK(buf[i].dest == d && buf[i].grp == k, "%s: record %llu of the range of (%u, %u) belongs to (%u, %u)", S.name,
                                                                                      (unsigned long long)i, d, k, buf[i].dest, buf[i].grp);
                    if (len) ranges.push_back({first, len});
                }
            }
            std::sort(ranges.begin(), ranges.end());
            u64 end = 0;
            for (const auto& r : ranges) { CHECK(r.first == end, "%s: send ranges leave a gap or overlap at %llu", S.name, (unsigned long long)end); end = r.first + r.second; }
            CHECK(end == buf.size(), "%s: send ranges cover %llu of %zu records", S.name, (unsigned long long)end, buf.size());
            // the receiver's piece: row `me` of the header
            pbase.push_back(at);
            at += (u32)own_n + 5;
            for (u32 v = 0; v < 256; ++v) pcnt.push_back((u32)send[(size_t)me * WIRE_HDR + 1 + v]);
        }
        if (!S.plan) continue;
        // the groups of rank `me`: cells, piece tables
        const CutPlan& P = *S.plan;
        const u32 my_lo = P.bin_lo[me], my_cells = P.bin_lo[me + 1] - my_lo, NG = P.ngroups[me];
        const std::vector<u32> gc0 = group_cells(P, me);
        CHECK(gc0.size() == NG + 1 && gc0[NG] == my_cells && (my_cells == 0 || gc0[0] == 0), "%s: cells of rank %u's groups do not span its %u cells", S.name, me, my_cells);
        for (u32 g = 0; g < NG; ++g) CHECK(gc0[g] <= gc0[g + 1], "%s: group cells not ascending", S.name);
        for (u32 cl = 0; cl < my_cells; ++cl) {
            const u32 iv = P.iv_of[my_lo + cl];
            if (iv != NO_BIN) CHECK(cl >= gc0[P.grp_of[iv]] && cl < gc0[P.grp_of[iv] + 1], "%s: cell %u of group %u outside [%u, %u)", S.name, cl, P.grp_of[iv], gc0[P.grp_of[iv]], gc0[P.grp_of[iv] + 1]);
        }
        std::vector<u64> rows(NP, 0);
        for (u32 g = 0; g < NG; ++g) {
            std::vector<u32> cnt_g, pb_g;
            group_piece_table(seg_of_bin + my_lo, gc0[g], gc0[g + 1], pcnt, pbase, cnt_g, pb_g);
            for (u32 p = 0; p < NP; ++p) {
                std::vector<u32> want(256, 0u);
                u64 before = 0;
                for (const Word& w : piece[p]) if (w.dest == me) { if (w.grp == g) want[w.seg]++; else if (w.grp < g) ++before; }
                for (u32 v = 0; v < 256; ++v) { rows[p] += cnt_g[p * 256 + v]; CHECK(cnt_g[p * 256 + v] == want[v], "%s: rank %u group %u piece %u segment %u: %u records, brute force %u", S.name, me, g, p, v, cnt_g[p * 256 + v], want[v]); }
                CHECK(pb_g[p] == pbase[p] + before, "%s: rank %u group %u piece %u starts at %u, brute force %llu", S.name, me, g, p, pb_g[p], (unsigned long long)(pbase[p] + before));
            }
        }
        for (u32 p = 0; p < NP; ++p) {
            u64 all = 0;
            for (u32 v = 0; v < 256; ++v) all += pcnt[p * 256 + v];
            CHECK(rows[p] == all, "%s: the groups' tables hold %llu of the piece's %llu records", S.name, (unsigned long long)rows[p], (unsigned long long)all);
        }
    }
    // the pieces of a slice in the log: the own piece at `filled`, the other sources behind it in rank order, rows copied in rank order
    for (u32 me = 0; me < W; ++me) {
        std::vector<u64> recv((size_t)W * WIRE_HDR, 0);
        for (u32 r = 0; r < W; ++r)
            for (u32 v = 0; v < 256; ++v) { const u64 x = rnd() % 5 == 0 ? rnd() % 300 : 0; recv[(size_t)r * WIRE_HDR + 1 + v] = x; recv[(size_t)r * WIRE_HDR] += x; }
        std::vector<u32> pbase{7}, pcnt(256, 9u);  // (a piece of an earlier slice stays as it is)
        const u64 filled = 1000 + rnd() % 1000;
        push_pieces(recv.data(), W, me, filled, recv[(size_t)me * WIRE_HDR], pbase, pcnt);
        CHECK(pbase.size() == W + 1 && pcnt.size() == (size_t)(W + 1) * 256 && pbase[0] == 7 && pcnt[255] == 9, "%s: push_pieces does not append", S.name);
        u64 at = filled + recv[(size_t)me * WIRE_HDR];
        for (u32 r = 0; r < W && pbase.size() == W + 1; ++r) {
            CHECK(pbase[1 + r] == (r == me ? filled : at), "%s: piece of source %u at %u", S.name, r, pbase[1 + r]);
            if (r != me) at += recv[(size_t)r * WIRE_HDR];
            for (u32 v = 0; v < 256; ++v) CHECK(pcnt[(size_t)(1 + r) * 256 + v] == recv[(size_t)r * WIRE_HDR + 1 + v], "%s: piece row of source %u", S.name, r);
        }
    }
    // a total in a bin no prefix maps to, and a total that does not match the word count
    u32 hole = 256;
    for (u32 bin = 0; bin < 256; ++bin) if (!bin_mapped(M, bin)) hole = bin;
    CHECK(hole < 256, "%s: every bin is mapped", S.name);
    if (hole < 256) { std::vector<u32> t(256, 0u); t[hole] = 1; CHECK(raises(M, t.data(), W, 0, 1), "%s: a word in unmapped bin %u is accepted", S.name, hole); }
    CHECK(raises(M, tots[0].data(), W, 0, piece[0].size() + 1), "%s: a wrong word count is accepted", S.name);
}

int main() {
    std::mt19937_64 rnd(20240607);
    long nbin = 0, ncut = 0, nfine = 0, refused = 0;
    for (int trial = 0; trial < 240; ++trial) {
        static const u32 WS[4] = {1, 2, 3, 8}, PBS[5] = {9, 12, 24, 25, 28};
        const u32 W = WS[trial % 4], PB = PBS[(trial / 4) % 5], RB = PB - 8;
        // rank bounds: ascending, distinct, below 2^(PB-1) where the necklace prefixes lie, crowded towards small values
        std::vector<u32> bounds;
        while (bounds.size() + 1 < W) {
            const u32 b = 1 + (u32)((rnd() % ((1ull << (PB - 1)) - 1)) >> (rnd() % (PB - 4)));
            if (std::find(bounds.begin(), bounds.end(), b) == bounds.end()) bounds.push_back(b);
        }
        std::sort(bounds.begin(), bounds.end());
        // group cuts: multiples of 64 strictly inside the ranges
        std::vector<u32> gcuts;
        for (u32 d = 0; d < W; ++d) {
            const u64 lo = d ? bounds[d - 1] : 0, hi = d + 1 < W ? bounds[d] : 1ull << (PB - 1);
            for (int j = 0; j < 3; ++j) {
                const u64 v = ((lo + rnd() % (hi - lo)) + 63) & ~63ull;
                if (v > lo && v < hi && std::find(gcuts.begin(), gcuts.end(), (u32)v) == gcuts.end()) gcuts.push_back((u32)v);
            }
        }
        std::sort(gcuts.begin(), gcuts.end());
        auto dest = [bounds](u32 p) { u32 d = 0; for (u32 b : bounds) d += b <= p ? 1u : 0u; return d; };
        auto grp = [bounds, gcuts, dest](u32 p) { const u32 d = dest(p); const u32 lo = d ? bounds[d - 1] : 0u; u32 g = 0; for (u32 cv : gcuts) g += (cv > lo && cv <= p) ? 1u : 0u; return g; };
        {   // the bins of the plain receiver
            const BinMap M = make_bin_map(PB, bounds.data(), W);
            if (M.ok) {
                ++nbin;
                Scheme S{"bin map", PB, W, nullptr, [=](u32 p) { const u32 v = p >> RB, b = v + dest(p); return Word{v >= 255u ? 255u : std::min(b, 254u), dest(p), 0u, v}; }};
                check_scheme(S, M, rnd, M.v_of);
            } else ++refused;
        }
        {   // the cut plan of the grouped receiver
            const CutPlan M = make_cut_plan(PB, bounds.data(), W, gcuts);
            if (M.ok) {
                ++ncut;
                std::vector<u32> cuts = M.cuts;
                Scheme S{"cut plan", PB, W, &M, [=](u32 p) {
                    const u32 v = p >> RB;
                    u32 k = 0;
                    for (u32 cv : cuts) k += cv <= p ? 1u : 0u;
                    return Word{v >= 255u ? 255u : v + k, dest(p), grp(p), v};
                }};
                check_scheme(S, static_cast<const CutPlan&>(M), rnd, M.v_of);
            } else ++refused;
        }
        if (PB > 24) {  // FINE bins; one rank: the fixed cut of the one-GPU build, filled from the bottom
            const std::vector<u32> one{std::min<u32>(245u << FINE_LEVEL, (1u << (PB - 1)) - (1u << FINE_LEVEL))};
            const std::vector<u32>& gc = W == 1 ? one : gcuts;
            const u32 lmax = (trial & 8) ? 24u : std::min(24u, PB - 4);
            const FinePlan M = make_fine_plan(PB, lmax, bounds.data(), W, gc, W == 1);
            if (M.ok) {
                ++nfine;
                std::vector<u32> cuts = M.cuts, forced = bounds;
                forced.insert(forced.end(), gc.begin(), gc.end());
                auto grp1 = [=](u32 p) { const u32 d = dest(p); const u32 lo = d ? bounds[d - 1] : 0u; u32 g = 0; for (u32 cv : gc) g += (cv > lo && cv <= p) ? 1u : 0u; return g; };
                const u32 top = (u32)((1ull << PB) - 1);
                const FinePlan* MP = &M;
                Scheme S{"fine plan", PB, W, &M, [=](u32 p) {
                    if (p == top) return Word{255u, dest(p), grp1(p), 255u};
                    u32 start = 0, seg = 0;  // the group starts at the largest bound or group cut at or below p; its bins count from there
                    for (u32 f : forced) if (f <= p) start = std::max(start, f);
                    for (u32 cv : cuts) seg += (cv > start && cv <= p) ? 1u : 0u;
                    return Word{fine_bin(*MP, PB, p), dest(p), grp1(p), seg};
                }};
                check_scheme(S, static_cast<const CutPlan&>(M), rnd, M.seg_of);
            } else ++refused;
        }
    }
    printf("wire layout unit: %ld bin maps, %ld cut plans, %ld fine plans checked, %ld refused, %ld bad\n", nbin, ncut, nfine, refused, bad);
    return bad || nbin < 40 || ncut < 40 || nfine < 20 ? 1 : 0;
}
