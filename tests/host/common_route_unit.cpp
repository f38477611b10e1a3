// common_route_unit.cpp — cbl_amd/csrc/common_route.hpp against a table written out by hand: which of the four kernels of cblx_intersection_count takes a
// bucket both indexes hold, and which side is staged. Every edge of the rule is here: ca + cb = 255 / 256 / 257 split three ways, the shorter side at 1023 /
// 1024 / 1025 against a probe side as long and of 5000 words, all four pairs of kinds (0 = Vec, 1 = Trie), and sums that do not fit 32 bits.
// tests/similarity_shapes.py holds the same rows for the GPU tests. Built with g++ -fsanitize=address,undefined by tests/test_similarity_host.py.
#include <cstdio>

#include "../../cbl_amd/csrc/common_route.hpp"

using namespace cblx;

struct Row { uint32_t ca, cb; int a_trie, b_trie, route, stage_a; };
static const Row kRows[] = {
    {1u, 254u, 0, 0, COMMON_WAVE, 1},
    {1u, 254u, 0, 1, COMMON_WAVE, 1},
    {1u, 254u, 1, 0, COMMON_WAVE, 1},
    {1u, 254u, 1, 1, COMMON_WAVE, 1},
    {127u, 128u, 0, 0, COMMON_WAVE, 1},
    {127u, 128u, 0, 1, COMMON_WAVE, 1},
    {127u, 128u, 1, 0, COMMON_WAVE, 1},
    {127u, 128u, 1, 1, COMMON_WAVE, 1},
    {128u, 127u, 0, 0, COMMON_WAVE, 0},
    {128u, 127u, 0, 1, COMMON_WAVE, 0},
    {128u, 127u, 1, 0, COMMON_WAVE, 0},
    {128u, 127u, 1, 1, COMMON_WAVE, 0},
    {254u, 1u, 0, 0, COMMON_WAVE, 0},
    {254u, 1u, 0, 1, COMMON_WAVE, 0},
    {254u, 1u, 1, 0, COMMON_WAVE, 0},
    {254u, 1u, 1, 1, COMMON_WAVE, 0},
    {1u, 255u, 0, 0, COMMON_WAVE, 1},
    {1u, 255u, 0, 1, COMMON_WAVE, 1},
    {1u, 255u, 1, 0, COMMON_WAVE, 1},
    {1u, 255u, 1, 1, COMMON_WAVE, 1},
    {128u, 128u, 0, 0, COMMON_WAVE, 1},
    {128u, 128u, 0, 1, COMMON_WAVE, 1},
    {128u, 128u, 1, 0, COMMON_WAVE, 1},
    {128u, 128u, 1, 1, COMMON_WAVE, 1},
    {255u, 1u, 0, 0, COMMON_WAVE, 0},
    {255u, 1u, 0, 1, COMMON_WAVE, 0},
    {255u, 1u, 1, 0, COMMON_WAVE, 0},
    {255u, 1u, 1, 1, COMMON_WAVE, 0},
    {1u, 256u, 0, 0, COMMON_WG, 1},
    {1u, 256u, 0, 1, COMMON_WG, 1},
    {1u, 256u, 1, 0, COMMON_WG, 1},
    {1u, 256u, 1, 1, COMMON_WG, 1},
    {128u, 129u, 0, 0, COMMON_WG, 1},
    {128u, 129u, 0, 1, COMMON_WG, 1},
    {128u, 129u, 1, 0, COMMON_WG, 1},
    {128u, 129u, 1, 1, COMMON_WG, 1},
    {129u, 128u, 0, 0, COMMON_WG, 0},
    {129u, 128u, 0, 1, COMMON_WG, 0},
    {129u, 128u, 1, 0, COMMON_WG, 0},
    {129u, 128u, 1, 1, COMMON_WG, 0},
    {256u, 1u, 0, 0, COMMON_WG, 0},
    {256u, 1u, 0, 1, COMMON_WG, 0},
    {256u, 1u, 1, 0, COMMON_WG, 0},
    {256u, 1u, 1, 1, COMMON_WG, 0},
    {1023u, 1023u, 0, 0, COMMON_WG, 1},
    {1023u, 1023u, 0, 1, COMMON_WG, 1},
    {1023u, 1023u, 1, 0, COMMON_WG, 1},
    {1023u, 1023u, 1, 1, COMMON_WG, 1},
    {1023u, 5000u, 0, 0, COMMON_WG, 1},
    {1023u, 5000u, 0, 1, COMMON_WG, 1},
    {1023u, 5000u, 1, 0, COMMON_WG, 1},
    {1023u, 5000u, 1, 1, COMMON_WG, 1},
    {5000u, 1023u, 0, 0, COMMON_WG, 0},
    {5000u, 1023u, 0, 1, COMMON_WG, 0},
    {5000u, 1023u, 1, 0, COMMON_WG, 0},
    {5000u, 1023u, 1, 1, COMMON_WG, 0},
    {1024u, 1024u, 0, 0, COMMON_WG, 1},
    {1024u, 1024u, 0, 1, COMMON_WG, 1},
    {1024u, 1024u, 1, 0, COMMON_WG, 1},
    {1024u, 1024u, 1, 1, COMMON_WG, 1},
    {1024u, 5000u, 0, 0, COMMON_WG, 1},
    {1024u, 5000u, 0, 1, COMMON_WG, 1},
    {1024u, 5000u, 1, 0, COMMON_WG, 1},
    {1024u, 5000u, 1, 1, COMMON_WG, 1},
    {5000u, 1024u, 0, 0, COMMON_WG, 0},
    {5000u, 1024u, 0, 1, COMMON_WG, 0},
    {5000u, 1024u, 1, 0, COMMON_WG, 0},
    {5000u, 1024u, 1, 1, COMMON_WG, 0},
    {1025u, 1025u, 0, 0, COMMON_SLICED, 1},
    {1025u, 1025u, 0, 1, COMMON_SLICED, 1},
    {1025u, 1025u, 1, 0, COMMON_SLICED, 1},
    {1025u, 1025u, 1, 1, COMMON_MERGE, 1},
    {1025u, 5000u, 0, 0, COMMON_SLICED, 1},
    {1025u, 5000u, 0, 1, COMMON_SLICED, 1},
    {1025u, 5000u, 1, 0, COMMON_SLICED, 1},
    {1025u, 5000u, 1, 1, COMMON_MERGE, 1},
    {5000u, 1025u, 0, 0, COMMON_SLICED, 0},
    {5000u, 1025u, 0, 1, COMMON_SLICED, 0},
    {5000u, 1025u, 1, 0, COMMON_SLICED, 0},
    {5000u, 1025u, 1, 1, COMMON_MERGE, 0},
    {1u, 1u, 0, 0, COMMON_WAVE, 1},
    {4294967295u, 4294967295u, 1, 1, COMMON_MERGE, 1},
    {4294967295u, 1u, 0, 0, COMMON_WG, 0},
    {4294967295u, 4294967295u, 0, 1, COMMON_SLICED, 1},
};

int main() {
    static_assert(COMMON_SMALL == 256 && COMMON_LDS == 1024, "the rows below are written for these thresholds");
    static_assert(COMMON_WAVE == 0 && COMMON_WG == 1 && COMMON_MERGE == 2 && COMMON_SLICED == 3 && COMMON_ROUTES == 4, "the order of the stats");
    int bad = 0;
    for (const Row& r : kRows) {
        const int got = common_route(r.ca, r.cb, r.a_trie != 0, r.b_trie != 0);
        const int st = common_stage_a(r.ca, r.cb) ? 1 : 0;
        if (got != r.route || st != r.stage_a) {
            std::printf("ca=%u cb=%u kinds=%d%d: route %d (expected %d), stage_a %d (expected %d)\n", r.ca, r.cb, r.a_trie, r.b_trie, got, r.route, st, r.stage_a);
            ++bad;
        }
    }
    std::printf("%zu rows, %d wrong\n", sizeof(kRows) / sizeof(kRows[0]), bad);
    return bad ? 1 : 0;
}
