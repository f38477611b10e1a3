// uniform_plan.hpp — the chunk plan of a batch of reads of ONE length without an invalid byte, as arithmetic.
//
// plan_chunks (pipeline.hpp) describes a batch by tables: chunk_start / chunk_len / kmer_off per chunk, tile_first per 4 KiB tile
// of the base stream (k_seq_chunk_count, k_chunk_fill, k_tile_first_chunk in kernels_encode.hpp). When every sequence has the same
// length L with K <= L and L - K + 1 <= CHUNK_KMERS (one chunk per sequence), sequences lie back to back and no byte is invalid,
// every entry is a closed formula of (s0, L, nk0, index):
//     nchunks = nseq      chunk_start[i] = s0 + i L      chunk_len[i] = L      kmer_off[i] = i nk0      (nk0 = L - K + 1)
//     tile_first[t] = first i with chunk_start[i] >= t * tile_bytes, at most nseq
// where s0 = offsets[0] - bias is the slice's first base relative to the 16-byte aligned position below it (0 .. 15).
// No HIP in here: tests/host/uniform_plan_unit.cpp builds it with g++ and holds it against a restatement of the table kernels.
#pragma once
#include <cstdint>

#if !defined(__HIPCC__) && !defined(__host__)
#define __host__
#define __device__
#endif

namespace cblx {

struct UniformPlan {
    uint32_t uniform = 0;  // 0: the tables describe the batch, nothing else in here is read
    uint32_t L = 0;        // length of every sequence = of its one chunk
    uint32_t nk0 = 0;      // k-mers of every chunk
    uint32_t s0 = 0;       // chunk_start[0]
    uint64_t n = 0;        // sequences = chunks
};

// the plan is arithmetic for nseq sequences of L bases each (equal lengths and clean bytes are the probe's to check)
__host__ __device__ inline bool uniform_plan_shape(uint64_t nseq, uint64_t L, uint32_t K, uint32_t chunk_kmers) {
    return nseq > 0 && nseq < 0xFFFFFFF0ull && L >= K && L - K + 1 <= chunk_kmers;
}
__host__ __device__ inline uint64_t uniform_chunk_start(const UniformPlan& u, uint64_t i) { return (uint64_t)u.s0 + i * u.L; }
__host__ __device__ inline uint64_t uniform_kmer_off(const UniformPlan& u, uint64_t i) { return i * u.nk0; }
__host__ __device__ inline uint32_t uniform_tile_first(const UniformPlan& u, uint64_t t, uint32_t tile_bytes) {
    const uint64_t key = t * tile_bytes;
    if (key <= u.s0) return 0;
    const uint64_t i = (key - u.s0 + u.L - 1) / u.L;
    return (uint32_t)(i < u.n ? i : u.n);
}

}  // namespace cblx
