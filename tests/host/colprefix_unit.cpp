// colprefix_unit.cpp — the two-level column prefixes of cbl_amd/csrc/colprefix.hpp on the host: the super-tile scan the producer
// kernels run (sup_scan_column) and the accessor the consumers read through (colpre_at), against a flat exclusive column prefix and
// the column totals of the same count matrix. Built with g++ -fsanitize=address,undefined by tests/test_colprefix_host.py.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../../cbl_amd/csrc/colprefix.hpp"

using namespace cblx;

static unsigned long long bad = 0, checked = 0;

// counts: [nt][256]. Builds local / sup the way the kernels do (one super-tile at a time, one column at a time), scans sup flat,
// and compares colpre_at for every (tile, digit), in both forms of the view, plus the totals.
static void check(const char* name, const std::vector<uint32_t>& counts, uint32_t nt) {
    const uint32_t nst = sup_count(nt);
    // exact sizes: a write or read past a ragged last super-tile is an ASan report
    std::vector<uint16_t> local((size_t)nt * 256);
    std::vector<uint32_t> sup((size_t)nst * 256), sup_pre((size_t)nst * 256), coltot(256), flat((size_t)nt * 256), want_tot(256, 0);
    for (uint32_t t = 0; t < nt; ++t)
        for (uint32_t d = 0; d < 256; ++d) { flat[(size_t)t * 256 + d] = want_tot[d]; want_tot[d] += counts[(size_t)t * 256 + d]; }
    uint32_t rows_seen = 0;
    for (uint32_t st = 0; st < nst; ++st) {
        const uint32_t rows = sup_rows(st, nt);
        rows_seen += rows;
        if (rows == 0 || rows > SUP_TILES) { ++bad; std::printf("%s: super-tile %u of %u tiles has %u rows\n", name, st, nt, rows); continue; }
        for (uint32_t d = 0; d < 256; ++d)
            sup[(size_t)st * 256 + d] = sup_scan_column(
                rows, [&](uint32_t r) { return counts[((size_t)st * SUP_TILES + r) * 256 + d]; },
                [&](uint32_t r, uint16_t p) { local[((size_t)st * SUP_TILES + r) * 256 + d] = p; });
    }
    if (rows_seen != nt || sup_rows(nst, nt) != 0) { ++bad; std::printf("%s: the super-tiles hold %u rows of %u\n", name, rows_seen, nt); }
    for (uint32_t d = 0; d < 256; ++d) {  // the flat column scan over sup (k_colscan_* on the device)
        uint32_t run = 0;
        for (uint32_t st = 0; st < nst; ++st) { sup_pre[(size_t)st * 256 + d] = run; run += sup[(size_t)st * 256 + d]; }
        coltot[d] = run;
    }
    const ColPre two(local.data(), sup_pre.data()), one(flat.data());
    for (uint32_t t = 0; t < nt; ++t)
        for (uint32_t d = 0; d < 256; ++d) {
            ++checked;
            const uint32_t w = flat[(size_t)t * 256 + d];
            if (colpre_at(two, t, d) != w || colpre_at(one, t, d) != w) {
                if (++bad < 10) std::printf("%s: tile %u digit %u: two-level %u, flat view %u, want %u\n", name, t, d, colpre_at(two, t, d), colpre_at(one, t, d), w);
            }
        }
    for (uint32_t d = 0; d < 256; ++d)
        if (coltot[d] != want_tot[d]) { if (++bad < 10) std::printf("%s: total of digit %u: %u, want %u\n", name, d, coltot[d], want_tot[d]); }
}

// n records into tiles of SUP_TILE_RECORDS (the last one ragged), digits drawn by `digit`
template <typename F> static std::vector<uint32_t> tiles_of(uint64_t n, uint32_t& nt, F digit) {
    nt = (uint32_t)((n + SUP_TILE_RECORDS - 1) / SUP_TILE_RECORDS);
    std::vector<uint32_t> c((size_t)nt * 256, 0);
    for (uint64_t i = 0; i < n; ++i) ++c[(size_t)(i / SUP_TILE_RECORDS) * 256 + digit(i)];
    return c;
}

int main() {
    std::mt19937_64 rng(12345);
    const uint32_t sizes[] = {0, 1, 15, 16, 17, 31, 32, 33, 1000};
    for (uint32_t nt : sizes) {
        char name[64];
        // random counts: full tiles with uniform digits, the last tile ragged
        std::snprintf(name, sizeof name, "random %u tiles", nt);
        uint32_t got;
        const uint64_t n = nt ? (uint64_t)(nt - 1) * SUP_TILE_RECORDS + 1 + rng() % SUP_TILE_RECORDS : 0;
        check(name, tiles_of(n, got, [&](uint64_t) { return (uint32_t)(rng() & 255u); }), nt);
        if (got != nt) { ++bad; std::printf("%s: %u tiles made\n", name, got); }
        // skewed: most records in few digits
        std::snprintf(name, sizeof name, "skewed %u tiles", nt);
        check(name, tiles_of(n, got, [&](uint64_t) { const uint32_t r = (uint32_t)rng(); return (r & 3u) ? (r >> 8) & 3u : (r >> 8) & 255u; }), nt);
        // every record in one column: the local prefix of the 16th tile of a super-tile is 15 * 4096 = 61 440
        std::snprintf(name, sizeof name, "one column %u tiles", nt);
        check(name, tiles_of((uint64_t)nt * SUP_TILE_RECORDS, got, [&](uint64_t) { return 255u; }), nt);
        // all-zero rows (tiles that hold nothing, as the unused rows of an upper-bound grid)
        std::snprintf(name, sizeof name, "zero rows %u tiles", nt);
        check(name, std::vector<uint32_t>((size_t)nt * 256, 0), nt);
        // zero rows among full ones
        std::snprintf(name, sizeof name, "sparse rows %u tiles", nt);
        std::vector<uint32_t> c = tiles_of((uint64_t)nt * SUP_TILE_RECORDS, got, [&](uint64_t) { return (uint32_t)(rng() & 255u); });
        for (uint32_t t = 0; t < nt; t += 3)
            for (uint32_t d = 0; d < 256; ++d) c[(size_t)t * 256 + d] = 0;
        check(name, c, nt);
    }
    {   // exactly 16 full tiles in one column, looked at directly: the largest value a local prefix takes
        uint32_t nt;
        const std::vector<uint32_t> c = tiles_of(16ull * SUP_TILE_RECORDS, nt, [](uint64_t) { return 7u; });
        uint16_t last = 0;
        const uint32_t tot = sup_scan_column(16, [&](uint32_t r) { return c[(size_t)r * 256 + 7]; }, [&](uint32_t r, uint16_t p) { if (r == 15) last = p; });
        if (nt != 16 || last != 61440 || tot != 65536) { ++bad; std::printf("16 full tiles in one column: last local %u, total %u\n", last, tot); }
    }
    std::printf("checked=%llu bad=%llu\n", checked, bad);
    return bad ? 1 : 0;
}
