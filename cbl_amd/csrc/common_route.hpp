// common_route.hpp — which kernel counts the words two indexes share in a bucket both hold (cblx_intersection_count).
//
// ca, cb: the two counts; the STAGED side is the shorter one (a's on a tie) and goes into LDS with a hash table over it, the other side is the PROBE
// side and is streamed past it. The kinds decide between the last two routes only: two Tries are two ascending lists and can be merged at any length,
// anything else with a long staged side is cut into slices of COMMON_LDS words.
// No HIP in here: tests/host/common_route_unit.cpp builds it with g++ and holds it against a table written out by hand.
#pragma once
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cblx {

static const uint32_t COMMON_SMALL = 256;  // words of both sides one wave takes (k_common_wave: staged side <= 128)
static const uint32_t COMMON_LDS = 1024;   // staged words one workgroup's table takes (k_common_lds) = the reference's Vec threshold
enum { COMMON_WAVE = 0, COMMON_WG = 1, COMMON_MERGE = 2, COMMON_SLICED = 3, COMMON_ROUTES = 4 };  // the order of cblx_intersection_count's stats[1 .. 4]

// is a's side the staged one?
__host__ __device__ inline bool common_stage_a(uint32_t ca, uint32_t cb) { return ca <= cb; }

__host__ __device__ inline int common_route(uint32_t ca, uint32_t cb, bool a_trie, bool b_trie) {
    if ((uint64_t)ca + cb <= COMMON_SMALL) return COMMON_WAVE;
    const uint32_t s = ca < cb ? ca : cb;
    if (s <= COMMON_LDS) return COMMON_WG;
    return a_trie && b_trie ? COMMON_MERGE : COMMON_SLICED;
}

}  // namespace cblx
