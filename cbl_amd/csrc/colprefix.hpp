// colprefix.hpp — column prefixes of the partition's tile count matrix in two levels.
//
// A partition pass needs colpre[tile][d] = records with digit d in the tiles before `tile`. The FLAT form keeps that as a u32
// matrix [tile][256] made by a scan of the whole count matrix (k_colscan_*). The TWO-LEVEL form groups SUP_TILES consecutive
// tiles into a super-tile:
//     colpre[tile][d] = sup_pre[tile / SUP_TILES][d] + local[tile][d]
//   local[tile][256] u16: exclusive column prefix over the earlier tiles of the SAME super-tile (at most 15 full tiles)
//   sup[st][256]     u32: column sums of super-tile st; the flat column scan over this 16 x smaller matrix gives sup_pre and the totals
// The count matrix itself is never scanned (and, where the producer counts in LDS, never written).
// No HIP in here: tests/host/colprefix_unit.cpp builds it with g++ and checks it against a flat exclusive column prefix.
#pragma once
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cblx {

static const uint32_t SUP_TILES = 16;       // tiles per super-tile
static const uint32_t SUP_SHIFT = 4;
static const uint32_t SUP_TILE_RECORDS = 4096;  // records of a full tile (= RDX_TILE, asserted in kernels_radix.hpp)
static_assert((1u << SUP_SHIFT) == SUP_TILES, "SUP_SHIFT is log2(SUP_TILES)");
static_assert((SUP_TILES - 1) * SUP_TILE_RECORDS < 65536u, "a local prefix (up to SUP_TILES - 1 full tiles in one column) must fit 16 bits");

__host__ __device__ inline uint32_t sup_count(uint32_t ntiles) { return (ntiles + SUP_TILES - 1) / SUP_TILES; }
// rows of super-tile st that exist (the last one may be ragged; 0 past the end)
__host__ __device__ inline uint32_t sup_rows(uint32_t st, uint32_t ntiles) {
    const uint64_t first = (uint64_t)st * SUP_TILES;
    if (first >= ntiles) return 0;
    return ntiles - first < SUP_TILES ? (uint32_t)(ntiles - first) : SUP_TILES;
}

// One column of one super-tile: put(r, exclusive prefix of get(0..r)) for its `rows` rows; returns the column sum (the sup entry).
template <typename Get, typename Put> __host__ __device__ inline uint32_t sup_scan_column(uint32_t rows, Get get, Put put) {
    uint32_t run = 0;
    for (uint32_t r = 0; r < rows; ++r) {
        const uint32_t v = get(r);
        put(r, (uint16_t)run);
        run += v;
    }
    return run;
}

// What the consumers of a column prefix read through: either the flat matrix or the two levels. One layout for both, so that the
// u32 load is the same instruction in either form and only the u16 load depends on it: base[(tile >> shift)][d] (+ local[tile][d]).
struct ColPre {
    const uint32_t* base = nullptr;   // flat: colpre[tile][256]; two levels: sup_pre[tile / SUP_TILES][256]
    const uint16_t* local = nullptr;  // two levels: [tile][256]; flat: null
    uint32_t shift = 0;               // 0 or SUP_SHIFT
    ColPre() = default;
    __host__ __device__ ColPre(const uint32_t* flat) : base(flat) {}
    __host__ __device__ ColPre(const uint16_t* l, const uint32_t* sup_pre) : base(sup_pre), local(l), shift(SUP_SHIFT) {}
};
__host__ __device__ inline uint32_t colpre_at(const ColPre& v, uint32_t tile, uint32_t d) {
    uint32_t p = v.base[(uint64_t)(tile >> v.shift) * 256 + d];
    if (v.local) p += v.local[(uint64_t)tile * 256 + d];
    return p;
}

}  // namespace cblx
