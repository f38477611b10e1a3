// Host check of cbl_amd/csrc/uniform_plan.hpp: the closed formulas of the arithmetic chunk plan against a plain restatement of what the
// table kernels define (k_seq_chunk_count, k_chunk_fill, k_tile_first_chunk in kernels_encode.hpp, the two exclusive scans of
// plan_chunks in pipeline.hpp). Built with -fsanitize=address,undefined by tests/test_uniform_plan_host.py. Prints "bad=<n>".
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../cbl_amd/csrc/uniform_plan.hpp"

using namespace cblx;

static const uint32_t CHUNK_KMERS = 2048;      // common.hpp
static const uint32_t ENC_TILE_BYTES = 4096;   // kernels_encode.hpp

struct Tables {
    uint64_t nchunks = 0, n_kmers = 0, total_bases = 0;
    std::vector<uint64_t> chunk_start, kmer_off;
    std::vector<uint32_t> chunk_len, tile_first;
};

// the tables of nseq sequences with the given offsets (every length >= K)
static Tables tables(const std::vector<uint64_t>& off, uint32_t K) {
    Tables T;
    const uint64_t nseq = off.size() - 1, bias = off[0] & ~(uint64_t)15;
    T.total_bases = off[nseq] - bias;
    std::vector<uint64_t> chunk_base(nseq + 1, 0);
    for (uint64_t i = 0; i < nseq; ++i) {  // k_seq_chunk_count + the exclusive scan
        const uint64_t nk = off[i + 1] - off[i] - K + 1;
        chunk_base[i + 1] = chunk_base[i] + (nk + CHUNK_KMERS - 1) / CHUNK_KMERS;
    }
    T.nchunks = chunk_base[nseq];
    std::vector<uint32_t> chunk_nk(T.nchunks);
    T.chunk_start.resize(T.nchunks);
    T.chunk_len.resize(T.nchunks);
    for (uint64_t seq = 0; seq < nseq; ++seq)  // k_chunk_fill: chunk c belongs to the last seq with chunk_base[seq] <= c
        for (uint64_t c = chunk_base[seq]; c < chunk_base[seq + 1]; ++c) {
            const uint64_t j = c - chunk_base[seq], s0 = off[seq], len = off[seq + 1] - s0, start = j * CHUNK_KMERS;
            uint64_t end = start + CHUNK_KMERS + K - 1;
            if (end > len) end = len;
            T.chunk_start[c] = s0 + start - bias;
            T.chunk_len[c] = (uint32_t)(end - start);
            chunk_nk[c] = (uint32_t)(end - start - K + 1);
        }
    T.kmer_off.assign(T.nchunks + 1, 0);
    for (uint64_t c = 0; c < T.nchunks; ++c) T.kmer_off[c + 1] = T.kmer_off[c] + chunk_nk[c];
    T.n_kmers = T.kmer_off[T.nchunks];
    const uint64_t ntiles = (T.total_bases + ENC_TILE_BYTES - 1) / ENC_TILE_BYTES;
    T.tile_first.resize(ntiles + 1);
    for (uint64_t t = 0; t <= ntiles; ++t) {  // k_tile_first_chunk: first c with chunk_start[c] >= t * ENC_TILE_BYTES
        const uint64_t key = t * ENC_TILE_BYTES;
        uint64_t lo = 0, hi = T.nchunks;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if (T.chunk_start[mid] < key) lo = mid + 1; else hi = mid;
        }
        T.tile_first[t] = (uint32_t)lo;
    }
    return T;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {  // splitmix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

static int bad = 0, cases = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++bad <= 20) { printf("FAIL %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } } } while (0)

// returns whether the last tile holds no chunk start
static bool one_case(uint64_t first, uint32_t L, uint32_t K, uint64_t nseq) {
    ++cases;
    std::vector<uint64_t> off(nseq + 1);
    for (uint64_t i = 0; i <= nseq; ++i) off[i] = first + i * L;
    const Tables T = tables(off, K);
    const bool shape = uniform_plan_shape(nseq, L, K, CHUNK_KMERS);
    CHECK(shape == (T.nchunks == nseq), "first=%llu L=%u K=%u nseq=%llu: shape=%d, table nchunks=%llu", (unsigned long long)first, L, K, (unsigned long long)nseq, (int)shape,
          (unsigned long long)T.nchunks);
    if (!shape) return false;
    UniformPlan u;
    u.uniform = 1; u.L = L; u.nk0 = L - K + 1; u.s0 = (uint32_t)(first & 15); u.n = nseq;
    CHECK(T.n_kmers == nseq * u.nk0, "n_kmers %llu", (unsigned long long)T.n_kmers);
    for (uint64_t i = 0; i < nseq; ++i) {
        CHECK(uniform_chunk_start(u, i) == T.chunk_start[i], "chunk_start[%llu] L=%u s0=%u", (unsigned long long)i, L, u.s0);
        CHECK(T.chunk_len[i] == L, "chunk_len[%llu] = %u, L=%u", (unsigned long long)i, T.chunk_len[i], L);
        CHECK(uniform_kmer_off(u, i) == T.kmer_off[i], "kmer_off[%llu] L=%u K=%u", (unsigned long long)i, L, K);
    }
    CHECK(uniform_kmer_off(u, nseq) == T.kmer_off[nseq], "kmer_off[nseq]");
    CHECK(uniform_chunk_start(u, nseq) == T.chunk_start[nseq - 1] + T.chunk_len[nseq - 1], "end of the last chunk");
    for (uint64_t t = 0; t < T.tile_first.size(); ++t)
        CHECK(uniform_tile_first(u, t, ENC_TILE_BYTES) == T.tile_first[t], "tile_first[%llu] = %u, table %u (first=%llu L=%u nseq=%llu)", (unsigned long long)t,
              uniform_tile_first(u, t, ENC_TILE_BYTES), T.tile_first[t], (unsigned long long)first, L, (unsigned long long)nseq);
    const size_t nt = T.tile_first.size() - 1;
    return nt >= 1 && T.tile_first[nt - 1] == T.tile_first[nt];
}

int main() {
    const uint32_t Ks[] = {5, 21, 31, 59};
    for (uint32_t K : Ks)
        for (uint64_t r = 0; r < 16; ++r) {
            const uint64_t first = 4096 * 3 + r;
            for (uint64_t nseq : {1ull, 2ull, 27ull, 28ull, 29ull, 1000ull}) {
                one_case(first, K, K, nseq);                 // L = K: one k-mer per sequence
                one_case(first, K + 1, K, nseq);
                one_case(first, 64, K, nseq);                // L divides the tile (K <= 59 < 64)
                one_case(first, 150, K, nseq);
                one_case(first, K + 2047, K, nseq);          // L - K + 1 = 2048: the largest single chunk
                one_case(first, K + 2048, K, nseq);          // 2049: two chunks per sequence, not arithmetic
                one_case(first, 4096, K, nseq);
            }
        }
    // a last tile that holds no chunk start: 28 reads of 150 bases end at byte 4200, the last one starts at 4050
    CHECK(one_case(0, 150, 31, 28), "28 x 150: the last tile should hold no chunk start");
    CHECK(one_case(7, 150, 31, 28), "28 x 150 from byte 7: the last tile should hold no chunk start");
    CHECK(!one_case(0, 64, 31, 128), "128 x 64: the last tile holds 64 chunk starts");
    int empty_last = 0;
    for (int it = 0; it < 3000; ++it) {
        const uint32_t K = 5 + 2 * (uint32_t)(rnd() % 28);  // odd, 5 .. 59
        const uint32_t span = (it % 3 == 0) ? 2049u : ((it % 3 == 1) ? 200u : 16u);
        const uint32_t L = K + (uint32_t)(rnd() % span);
        const uint64_t first = (rnd() % 100000) * ((it & 1) ? 1 : 16) + (rnd() % 16);
        const uint64_t nseq = 1 + rnd() % ((L > 512) ? 40 : 3000);
        empty_last += one_case(first, L, K, nseq) ? 1 : 0;
    }
    CHECK(empty_last > 0, "no random case had an empty last tile");
    CHECK(!uniform_plan_shape(0, 150, 31, CHUNK_KMERS), "no sequence");
    CHECK(!uniform_plan_shape(10, 30, 31, CHUNK_KMERS), "shorter than K");
    CHECK(!uniform_plan_shape(0xFFFFFFF0ull, 150, 31, CHUNK_KMERS), "too many chunks");
    CHECK(uniform_plan_shape(0xFFFFFFEFull, 150, 31, CHUNK_KMERS), "the largest batch");
    printf("cases=%d empty_last=%d bad=%d\n", cases, empty_last, bad);
    return bad ? 1 : 0;
}
