/* cblx.h — C ABI of the MI355X-native bulk k-mer insertion path for CBL indexes.
 *
 * One `cblx_ctx` stands for one `CBL<K, T, PREFIX_BITS>` value of the reference
 * (/root/reference/src/cbl.rs:40-54). The reference has no plugin registry; its only FFI is
 * autocxx -> C++ for RankBV / TieredVec32 (/root/reference/src/ffi.rs:7-20). This header is the
 * `extern "C"` layer a Rust `CBL<K,T,PREFIX_BITS>` facade binds instead:
 * const generics become the runtime fields of `cblx_params`; `panic!` becomes a non-zero status +
 * `cblx_last_error` (the shim re-panics with the same message).
 *
 * Conventions
 *   - every function returns 0 on success, a CBLX_E* code otherwise; nothing throws across the ABI;
 *   - plain pointers + sizes only; input pointers are borrowed for the duration of the call;
 *   - `*_device` entry points take DEVICE pointers valid on the ctx's GPU, all others HOST pointers;
 *   - a ctx is single-owner / not re-entrant (the reference API is `&mut self` throughout);
 *   - `cblx_insert_seq*` may only enqueue; every observer flushes first.
 *   - the HIP library is the only implementation: there is no CPU fallback behind this ABI.
 */
#ifndef CBLX_H
#define CBLX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: cblx_merge_from, cblx_stage_units, cblx_fine_builds, cblx_comm_groups_fine, cblx_comm_protocol_used, CBLX_PROTO_AUTO (the default of a new
 * communicator: an unchanged 2 - 4 rank caller no longer runs BINS), CBLX_PROTO_REPLICATE; empty PREFIX_BITS > 24 builds take the FINE route. A binding
 * built against this header must refuse a library that reports less.
 * Added under 3 (a new symbol is compatible): cblx_set_op with CBLX_SETOP_OR / AND / SUB / XOR, cblx_get_device, cblx_set_op_assign, and cblx_set_op_many with
 * CBLX_SETOP_MAX_OPERANDS; cblx_remove_words_device, cblx_remove_seq, cblx_remove_seqs, cblx_remove_seqs_device, cblx_remove_fastx_file and cblx_remove_kmers;
 * cblx_export_kmers_range, cblx_export_kmers_range_device, cblx_list_range, cblx_list_range_device, cblx_list_to_fd, cblx_list_to_file and cblx_bucket_nodes;
 * cblx_contains_seqs_counts, cblx_contains_seqs_counts_device, cblx_contains_seqs_flags_counts_device and cblx_query_fastx_file_counts;
 * cblx_intersection_count with CBLX_COMMON_STATS, and cblx_intersection_counts; cblx_set_at_least and cblx_occupancy_counts;
 * cblx_contains_seqs_counts_many and cblx_contains_seqs_counts_many_device;
 * cblx_neighbors_kmers, cblx_neighbors_kmers_device, cblx_neighbors_range, cblx_neighbors_range_device and cblx_degree_table;
 * cblx_rank_kmers, cblx_rank_kmers_device, cblx_unitig_table, cblx_unitig_table_device, cblx_unitigs_text_device, cblx_unitigs_to_fd and cblx_unitigs_to_file;
 * cblx_biunitig_table, cblx_biunitig_table_device, cblx_biunitigs_text_device, cblx_biunitigs_to_fd and cblx_biunitigs_to_file;
 * cblx_gfa_links, cblx_gfa_links_device, cblx_gfa_text_device, cblx_gfa_to_fd and cblx_gfa_to_file;
 * cblx_unitig_ends, cblx_unitig_ends_device, cblx_tips_mark, cblx_tips_mark_device and cblx_clip_tips with cblx_clip_stats and CBLX_CLIP_ISOLATED;
 * cblx_components, cblx_components_device and cblx_components_filter with cblx_component_stats and CBLX_COMPONENTS_LARGEST;
 * cblx_abundance_seqs, cblx_abundance_seqs_device, cblx_abundance_histogram, cblx_unitig_coverage, cblx_unitig_coverage_device, cblx_gfa_tagged_text_device,
 * cblx_gfa_tagged_to_fd, cblx_gfa_tagged_to_file and cblx_abundance_filter with cblx_abundance_stats and CBLX_ABUNDANCE_UNITIGS;
 * cblx_bubbles_mark, cblx_bubbles_mark_device and cblx_pop_bubbles with cblx_bubble_stats. */
#define CBLX_ABI_VERSION 3

enum {
    CBLX_OK = 0,
    CBLX_EINVAL = 1,   /* bad parameter (K, PREFIX_BITS, null pointer, params mismatch) */
    CBLX_ESHORT = 2,   /* "Sequence size (n) is smaller than K (k)"   src/cbl.rs:329-334 */
    CBLX_EFORMAT = 3,  /* index bytes do not parse / trailing bytes    src/cbl.rs:146-158 */
    CBLX_EDEVICE = 4,  /* HIP runtime error or no usable GPU */
    CBLX_ENOMEM = 5,
    CBLX_ERANGE = 6    /* output buffer too small */
};

typedef struct cblx_ctx cblx_ctx;

typedef struct cblx_params {
    uint32_t k;           /* const K: odd, 5..59 (build.rs:18-24; 2K + POS_BITS <= 128, src/cbl.rs:87-91) */
    uint32_t prefix_bits; /* const PREFIX_BITS: 1..32 and < 2K + POS_BITS (src/wordset/mod.rs:37-41); default 24 */
    uint32_t canonical;   /* CBL::new() = 0, CBL::new_canonical() = 1 (src/cbl.rs:71-79) */
    int32_t device;       /* HIP device ordinal; -1 = current device */
    uint32_t flags;       /* CBLX_FLAG_* */
    uint32_t reserved;
} cblx_params;

#define CBLX_FLAG_PROFILE 1u /* record per-stage HIP-event timings of each flush (cblx_stage_times) */

uint32_t cblx_abi_version(void);
/* Error text of the last failed call on this thread that had no ctx (cblx_create). */
const char* cblx_last_global_error(void);

/* CBL::new / new_canonical (src/cbl.rs:71-79, asserts :87-91 and src/wordset/mod.rs:37-41). */
int cblx_create(const cblx_params* params, cblx_ctx** out);
/* Drop (frees device memory owned by the ctx). */
void cblx_destroy(cblx_ctx* ctx);
const char* cblx_last_error(const cblx_ctx* ctx);

/* CBL::insert_seq (src/cbl.rs:328-339): enqueue ONE sequence of ASCII nucleotides (copied). */
int cblx_insert_seq(cblx_ctx* ctx, const uint8_t* seq, uint64_t len);
/* The caller loop `for record in reader { cbl.insert_seq(record.seq()) }` (examples/cbl.rs:160-163,242-245)
 * in one call: sequence i is bases[offsets[i] .. offsets[i+1]), i < n. Stream order = i ascending. */
int cblx_insert_seqs(cblx_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n);
/* Same, inputs already resident in HBM (device pointers; d_bases 16-byte aligned). offsets[0] need not be 0: a slice
 * offsets[a..b] of a larger batch addresses the same d_bases. Runs the insert before returning. */
int cblx_insert_seqs_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n);
/* The reader loop of examples/cbl.rs:154-163 (needletail stand-in): every record of a plain-text FASTA (multi-line ok)
 * or 4-line FASTQ file, plain or gzip (zlib is looked up at run time), goes through insert_seq, in file order. */
int cblx_insert_fastx_file(cblx_ctx* ctx, const char* path, uint64_t* n_records);
/* Materialise everything enqueued so far into the resident index (idempotent). */
int cblx_flush(cblx_ctx* ctx);

/* The reader loop of examples/cbl.rs:154-163 for a multi-GPU build from ONE file with file-order parity: parses the file like
 * cblx_insert_fastx_file but INSERTS NOTHING; the records that block-cyclic dealing gives this rank — record i (file order,
 * 0-based) belongs to rank (i / block) % world — are staged in HBM, in file order, and lent to the caller as device arrays
 * (bases, n_staged + 1 offsets, d_offsets[0] = 0; d_bases 16-byte aligned) until cblx_stage_release. Local block c (records
 * [c * block, (c + 1) * block) of the staged list) is block c * world + rank of the file, so a sharded build that feeds local
 * block c as slice c has the stream order of the file. *n_in_file = records in the whole file. block = 0: count only.
 * While records are staged the ctx takes no cblx_insert_seq* calls; its index can be read and inserted into by the
 * *_device entry points. A record shorter than K is CBLX_ESHORT on the rank that owns it. */
int cblx_stage_fastx_blocks(cblx_ctx* ctx, const char* path, uint64_t block, uint32_t rank, uint32_t world, const uint8_t** d_bases,
                            const uint64_t** d_offsets, uint64_t* n_staged, uint64_t* n_in_file);
int cblx_stage_release(cblx_ctx* ctx);
/* The same staging for the ranks of a communicator (rank / world are the communicator's), with the parse SHARED between them:
 * rank r counts the records of bytes [r, r + 1) * size / world of the file, the counts and the byte offsets of the block starts
 * are summed over the ranks, and every rank then reads only the bytes of ITS blocks — host time per rank ~ 1 / world instead of
 * one whole-file parse per rank. *block: records per block; 0 = chosen here so that every rank gets about `slices` blocks
 * (written back). A file the parallel readers do not take (gzip, a record shorter than K, a malformed FASTQ record) falls back
 * to cblx_stage_fastx_blocks on every rank. Collective: every rank of the communicator calls it with the same path. */
struct cblx_comm;
int cblx_stage_fastx_blocks_comm(cblx_ctx* ctx, struct cblx_comm* comm, const char* path, uint64_t* block, uint32_t slices,
                                 const uint8_t** d_bases, const uint64_t** d_offsets, uint64_t* n_staged, uint64_t* n_in_file);

/* Device word arrays (all *_words_device entry points): word i = (hi[i] << 64) | lo[i]. `lo` is uint64_t[]; the element
 * type of `hi` follows from K like the reference's T (build.rs:34-41) and is reported by cblx_consts.hi_bytes:
 *   0 -> no hi array (2K + POS_BITS <= 64; pass NULL), 1 -> uint8_t[] (K = 31: 68-bit words), 8 -> uint64_t[] (K >= 33). */

/* WordSet::insert_batch (src/wordset/mod.rs:187-216) on already transformed words, stream order = index order.
 * On an empty index the first partition pass reads the caller's arrays in place (no copy). */
int cblx_insert_words_device(cblx_ctx* ctx, const uint64_t* d_lo, const void* d_hi, uint64_t n);
/* CBL::get_seq_words over every chunk of every sequence (src/cbl.rs:239-289), no insertion: writes the
 * words in stream order to d_lo/d_hi (device, capacity `cap` words) and their number to *n_words. */
int cblx_seq_words_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n,
                          uint64_t* d_lo, void* d_hi, uint64_t cap, uint64_t* n_words);

/* Multi-GPU exchange step (no reference counterpart; the reference is single-process): STABLE partition of n words
 * by destination = #{i : bounds[i] <= prefix(word)}, nd destinations (<= 16), bounds[nd-1] ascending prefix values
 * (host). Destination d's words land contiguously, in input order, at d_out[sum(counts[0..d])..]; counts[nd] (host)
 * receives the run lengths. Device word arrays as above. */
int cblx_partition_words_device(cblx_ctx* ctx, const uint64_t* d_lo, const void* d_hi, uint64_t n, const uint32_t* bounds,
                                uint32_t nd, uint64_t* d_out_lo, void* d_out_hi, uint64_t* counts);

/* cblx_seq_words_device + cblx_partition_words_device in one call (the per-slice step of the multi-GPU build): the
 * words of the sequences, grouped by destination, written to d_out_lo/d_out_hi (capacity `cap` words). */
int cblx_seq_words_partitioned_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n,
                                      const uint32_t* bounds, uint32_t nd, uint64_t* d_out_lo, void* d_out_hi, uint64_t cap,
                                      uint64_t* counts, uint64_t* n_words);

/* Multi-GPU build, "sorted batch" protocol (no reference counterpart). A rank partitions ITS words completely before the
 * exchange; per destination it ships a slice of the prefix-sorted batch — the non-empty prefixes, their word counts and
 * the suffixes alone, packed to suffix_bytes (= cblx_consts.bytes) little-endian bytes each: 6 B per word at K=31 /
 * PREFIX_BITS=24 instead of the 9 B of a full word — and the receiver merges the batches of all ranks bucket by bucket
 * without partitioning anything again. */
typedef struct cblx_batch_view {
    uint64_t n_buckets;       /* non-empty prefixes of the batch */
    uint64_t n_words;
    const uint32_t* d_prefix; /* device [n_buckets], strictly ascending */
    const uint32_t* d_count;  /* device [n_buckets], words per prefix */
    const uint8_t* d_suffix;  /* device [n_words * suffix_bytes], bucket-major, stream order inside a bucket */
} cblx_batch_view;
/* Sender: KRN-1 + the full stable partition of the words of n device-resident sequences. The batch stays in the ctx until
 * it is exported (or replaced by the next begin). Destination d = #{i : bounds[i] <= prefix} (nd destinations, nd-1
 * ascending host bounds) owns buckets [bucket_split[d], bucket_split[d+1]) and words [word_split[d], word_split[d+1])
 * of it (host arrays of nd + 1 entries). */
int cblx_sorted_batch_begin(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n, const uint32_t* bounds,
                            uint32_t nd, uint64_t* bucket_split, uint64_t* word_split);
/* Writes the pending batch — all destinations, in order — to caller-owned device arrays of bucket_split[nd],
 * bucket_split[nd] and word_split[nd] * suffix_bytes elements, and drops it. */
int cblx_sorted_batch_export(cblx_ctx* ctx, uint32_t* d_prefix, uint32_t* d_count, uint8_t* d_suffix);
/* Receiver: WordSet::insert_batch (src/wordset/mod.rs:187-216) over n_batches sorted batches; stream order = batch
 * order (then bucket order is irrelevant, and stream order inside a bucket of a batch is kept). */
int cblx_insert_sorted_batches_device(cblx_ctx* ctx, const cblx_batch_view* batches, uint32_t n_batches);

/* ---- prefix-range sharded indexes (BASELINE.json cfg 5 on N GPUs; no reference counterpart: the reference is one process) ----
 * `cbl merge a b -o out` (examples/cbl.rs:270-279) per prefix range: every rank loads ITS range of both files
 * (read_index, examples/cbl.rs:117-130), merges (src/wordset/set_ops.rs:123-157: buckets are independent by prefix) and
 * writes its entries at its own offset of the output (write_index, examples/cbl.rs:132-142). Two operands cut at
 * different bounds are brought to common bounds by moving bucket batches between ranks (export -> exchange -> install). */
typedef struct cblx_shard_info {
    uint64_t header_entries;   /* entry count in the file header (the whole index) */
    uint64_t local_entries;    /* entries this rank loaded */
    uint64_t begin_off, end_off; /* byte range of the file this rank parsed */
    uint32_t first_prefix, last_prefix; /* of the loaded entries (when local_entries != 0) */
    uint32_t exact;            /* 1: the walk over [begin_off, end_off) ended exactly at end_off and nothing looked wrong */
    uint32_t canonical;        /* the file's canonical flag */
} cblx_shard_info;
/* Replaces the ctx's contents by rank `rank`'s share of an index file cut into `world` prefix ranges.
 *   bounds == NULL: the entries are cut into `world` runs of about equal BYTE length; bounds_out[world-1] receives the first
 *                   prefix of runs 1..world-1 (2^PREFIX_BITS for an empty tail run): the job's shard bounds.
 *   bounds != NULL: world-1 ascending prefix values; rank r takes the entries with bounds[r-1] <= prefix < bounds[r].
 * The format has no lengths to skip by, so entry starts are RECOGNISED speculatively (a bisection over byte offsets);
 * sequential != 0 walks every entry from the first one instead (always right, reads the file up to the end of the range).
 * The caller must check over ALL ranks that every info.exact is 1 and that the local_entries add up to header_entries,
 * and otherwise repeat the call with sequential = 1 on every rank. K / PREFIX_BITS as for cblx_load. */
int cblx_load_shard_from_file(cblx_ctx* ctx, const char* path, uint32_t rank, uint32_t world, const uint32_t* bounds, int sequential,
                              uint32_t* bounds_out, cblx_shard_info* info);
/* Host-only part of the above (no ctx, no GPU): where `world` prefix ranges cut the entries of an index file. offs[world + 1]
 * = byte offset of every range's first entry ([world] = file size), first[world + 1] = that entry's prefix (2^PREFIX_BITS when
 * nothing follows), *ok = 0 when the speculative search gave up (use sequential = 1). Only k / prefix_bits of params are read. */
int cblx_index_shard_cuts(const cblx_params* params, const char* path, uint32_t world, const uint32_t* bounds, int sequential,
                          uint64_t* offs, uint32_t* first, int* ok);
/* The resident index as a bucket batch: ascending non-empty prefixes, words per prefix, kind (0 = Vec, 1 = Trie) and the
 * suffixes packed to cblx_consts.bytes little-endian bytes each, bucket-major, STORED order inside a bucket. */
typedef struct cblx_bucket_view {
    uint64_t n_buckets, n_words;
    const uint32_t* d_prefix; /* device [n_buckets] */
    const uint32_t* d_count;  /* device [n_buckets] */
    const uint8_t* d_kind;    /* device [n_buckets] */
    const uint8_t* d_suffix;  /* device [n_words * suffix_bytes] */
} cblx_bucket_view;
/* Where nd-1 ascending prefix bounds (host) cut the resident index: destination d = #{i : bounds[i] <= prefix} owns buckets
 * [bucket_split[d], bucket_split[d+1]) and words [word_split[d], word_split[d+1]) of the export (host arrays, nd + 1). */
int cblx_resident_split(cblx_ctx* ctx, const uint32_t* bounds, uint32_t nd, uint64_t* bucket_split, uint64_t* word_split);
/* Writes the whole resident index to caller-owned device arrays of cblx_num_buckets / cblx_count elements (the index stays). */
int cblx_resident_export(cblx_ctx* ctx, uint32_t* d_prefix, uint32_t* d_count, uint8_t* d_kind, uint8_t* d_suffix);
/* Replaces the ctx's contents by the concatenation of n_parts bucket batches (prefixes strictly ascending over the whole
 * concatenation: the pieces of one prefix range received from ranks 0..W-1 in rank order). Kinds and stored order are kept,
 * as WordSet's Deserialize keeps them (src/wordset/mod.rs:398-437). */
int cblx_install_buckets_device(cblx_ctx* ctx, const cblx_bucket_view* parts, uint32_t n_parts);
/* The entries of the serialized index alone — what follows `canonical u8 | varint(n_entries)` in cblx_serialize's bytes — so
 * that several ranks can write one file: size first, then the bytes at `file_off` of an existing file (opened write-only). */
int cblx_serialized_body_size(cblx_ctx* ctx, uint64_t* n_entries, uint64_t* nbytes);
int cblx_write_body_at(cblx_ctx* ctx, const char* path, uint64_t file_off);

/* ---- the multi-GPU build behind this ABI (no reference counterpart; BASELINE.json north_star: prefix space partitioned over the
 * GPUs of a node, one exchange over xGMI after the radix step) -------------------------------------------------------------
 * One process (or thread) per GPU, each with its own cblx_ctx and one cblx_comm. The communicator is RCCL (librccl.so.1 is
 * looked up at run time; rank 0 makes the id with cblx_comm_unique_id and the host program hands it to the other ranks by
 * whatever means it has), or a set of host callbacks that move the bytes (tests; fabrics RCCL does not drive). */
typedef struct cblx_comm cblx_comm;
#define CBLX_COMM_ID_BYTES 128
typedef struct cblx_transport {
    void* user;
    /* in place: vals[i] = sum over ranks of vals[i] (host memory), on every rank */
    int (*all_reduce_sum_u64)(void* user, uint64_t* vals, uint64_t n);
    /* send[d * per_rank ..] goes to rank d, recv[s * per_rank ..] comes from rank s (host memory) */
    int (*all_to_all_u64)(void* user, const uint64_t* send, uint64_t* recv, uint64_t per_rank);
    /* personalised exchange of byte runs in DEVICE memory: bytes [send_off[d], send_off[d+1]) of d_src go to rank d, the bytes
     * from rank s land at [recv_off[s], recv_off[s+1]) of d_dst (world + 1 host offsets each; the rank's own run included).
     * Complete on return. */
    int (*exchange)(void* user, const uint8_t* d_src, const uint64_t* send_off, uint8_t* d_dst, const uint64_t* recv_off);
} cblx_transport;
int cblx_comm_unique_id(uint8_t id[CBLX_COMM_ID_BYTES]);
int cblx_comm_init_rccl(cblx_comm** out, const uint8_t* id, uint32_t rank, uint32_t world, int32_t device);
int cblx_comm_init_transport(cblx_comm** out, const cblx_transport* t, uint32_t rank, uint32_t world, int32_t device);
void cblx_comm_destroy(cblx_comm* comm);
const char* cblx_comm_last_error(const cblx_comm* comm);
typedef struct cblx_exchange_stats { uint64_t sent_bytes, recv_bytes, messages; } cblx_exchange_stats; /* own runs excluded */
int cblx_comm_stats(cblx_comm* comm, cblx_exchange_stats* out, int reset);
/* What crosses the links in cblx_sharded_insert_seqs_device (every rank of a job sets the same):
 *   CBLX_PROTO_BINS: the exchange sits between the first and the second partition pass. The sender runs KRN-1 and
 *     the first pass on bins that refine that pass's digit by the destination rank; 8-byte records (16 for words that keep
 *     a 64-bit hi part) + 1 digit byte per word cross the links, the receiver runs the remaining passes and the bucket
 *     kernels on what arrived. No pass is added to the one-GPU pipeline and nothing is copied: the choice when the kernels
 *     are the bound (8 GPUs). Needs PREFIX_BITS >= 9, else SORTED is used.
 *   CBLX_PROTO_SORTED: the sender partitions completely; non-empty prefixes, counts and the suffixes packed to
 *     cblx_consts.bytes cross the links (6.1 B per word at K = 31 / PREFIX_BITS = 24), the receiver merges the batches run
 *     by run (one more pass over the words): the choice when the links are the bound (2-4 GPUs).
 *   CBLX_PROTO_AUTO (what a new communicator is set to): SORTED on 2 - 4 ranks, BINS otherwise. Between 2 - 4 GPUs every pair shares ONE link
 *     and the bytes on it bound the job; rehearsed against a paced wire (profiles/r05_wire_emulated.md, cfg 3, 55 GB/s per link): 2 ranks
 *     101 ms SORTED / 127 ms BINS, 4 ranks 69 / 71 ms (the two meet near 60 GB/s per link), 8 ranks BINS 47 ms. cblx_comm_protocol_used: what the last sharded insert ran on. */
#define CBLX_PROTO_SORTED 0u
#define CBLX_PROTO_BINS 1u
#define CBLX_PROTO_AUTO 2u
/*   CBLX_PROTO_REPLICATE (round 6): READS cross the links, not words — every rank packs its reads into bit planes on the device (3 bits per
 *     base = 0.3 bytes per k-mer), planes and offsets are all-gathered, and every rank runs KRN-1 and the first partition pass over ALL ranks'
 *     reads, keeping the words of its own prefix range; the receiver steps are those of BINS (groups, FINE bins). W encodes per rank instead
 *     of one and next to nothing on the wire: the choice where one link per pair of GPUs bounds the other protocols (2 - 3 GPUs). Falls back to
 *     BINS together with every other rank on a non-empty index or bounds the bins refuse. */
#define CBLX_PROTO_REPLICATE 3u
int cblx_comm_set_protocol(cblx_comm* comm, uint32_t protocol);
int cblx_comm_protocol_used(const cblx_comm* comm, uint32_t* out);
/* The receiver of CBLX_PROTO_BINS in GROUPS (no reference counterpart; same result, another schedule): every rank's prefix range is
 * cut into `groups` parts of about equal sampled mass, the senders' first pass also separates the groups, the data crosses the links
 * group-major, and the receiver runs the remaining passes + bucket kernels of group g while groups g+1.. are still on the wire.
 * 0 = default (CBLX_RECV_GROUPS in the environment, else 4), 1 = off (everything waits for the last record), at most 14. Every rank
 * of a job sets the same. cblx_comm_groups_used: groups the last cblx_sharded_insert_seqs_device of this rank worked through
 * (0: it took the ungrouped path — index not empty, ranges too narrow for the cuts, one rank). */
/* Rehearsal of ONE rank of a `world`-GPU job on one GPU (dev / bench tooling, no reference counterpart: tools/emulate_wire.py). Ranks
 * 1 .. world-1 are run one after the other on communicators that RECORD, in the process-wide store `store_id`, what each would send
 * to rank 0; a rank-0 communicator then REPLAYS them: its collectives are answered from the records and the bytes of every exchange
 * are copied into its receive arena on a side stream held back until a wire of `link_gbps` GB/s per source rank would have delivered
 * them (0 = as fast as the copies go). All ranks of a rehearsal hold equally many reads and make the same calls with the same bounds
 * and group setting. */
int cblx_comm_init_sim(cblx_comm** out, uint32_t rank, uint32_t world, int32_t device, uint64_t store_id, double link_gbps);
int cblx_sim_store_free(uint64_t store_id);
int cblx_comm_set_recv_groups(cblx_comm* comm, uint32_t groups);
int cblx_comm_groups_used(const cblx_comm* comm, uint32_t* out);
/* ... and how many of those groups sorted 16 prefix bits behind the senders' first pass instead of PREFIX_BITS - 8 (PREFIX_BITS > 24: the first
 * pass runs on FINE bins that cut a narrow group's prefix range into aligned blocks of 2^16 prefixes, so its receiver needs two partition
 * passes instead of three; CBLX_FINE_BINS=0 in the environment switches that off). Same result either way. */
int cblx_comm_groups_fine(const cblx_comm* comm, uint32_t* out);
/* CBL::insert_seq for every sequence of THIS rank's shard, into an index sharded by prefix range over the ranks of `comm`
 * (every rank makes the same call with its own shard). The shard is consumed in n_slices slices, reads
 * [slice_cuts[s], slice_cuts[s+1]) (n_slices + 1 ascending values, the same NUMBER of slices on every rank): the exchange of
 * a slice overlaps the kernels of the next one, and the job's stream order is slice-major, rank-minor — the order of the file
 * when its blocks were dealt to the ranks cyclically (cblx_stage_fastx_blocks). bounds[world - 1]: the shard bounds (rank r
 * owns bounds[r-1] <= prefix < bounds[r]); *bounds_valid = 0 on the first call lets the ranks choose them together (quantiles
 * of a sampled prefix histogram: necklace prefixes are heavily skewed) and sets it to 1. Afterwards the ctx of rank r holds
 * range r of the index: count / serialize / cblx_write_body_at work per range. */
int cblx_sharded_insert_seqs_device(cblx_ctx* ctx, cblx_comm* comm, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n,
                                    const uint64_t* slice_cuts, uint32_t n_slices, uint32_t* bounds, int* bounds_valid);

/* CBL::count / is_empty / is_canonical (src/cbl.rs:164-177). */
int cblx_count(cblx_ctx* ctx, uint64_t* out);
int cblx_num_buckets(cblx_ctx* ctx, uint64_t* out); /* tiered.len() = number of non-empty prefixes */
int cblx_is_empty(cblx_ctx* ctx, int* out);
int cblx_is_canonical(const cblx_ctx* ctx, int* out);

/* Serialize (derive on CBL src/cbl.rs:40-54 + WordSet::serialize src/wordset/mod.rs:382-396) with
 * bincode DefaultOptions + varint (src/cbl.rs:132-135): the exact bytes of CBL::save_to_file. */
int cblx_serialized_size(cblx_ctx* ctx, uint64_t* nbytes);
int cblx_serialize(cblx_ctx* ctx, uint8_t* buf, uint64_t cap, uint64_t* written);
int cblx_save_to_file(cblx_ctx* ctx, const char* path);
/* Deserialize (src/wordset/mod.rs:398-437; reject_trailing_bytes): replaces the ctx's contents.
 * K / PREFIX_BITS are not stored in the file (compile-time on both sides in the reference). */
int cblx_load(cblx_ctx* ctx, const uint8_t* data, uint64_t len);
int cblx_load_from_file(cblx_ctx* ctx, const char* path);

/* `self |= other` (src/cbl.rs:433-449 -> src/wordset/set_ops.rs:123-157). */
int cblx_merge_assign(cblx_ctx* self, cblx_ctx* other);
/* dst = what `self |= other` would leave in self, with self itself untouched (and other exactly as `|=` leaves it: its Vec buckets that
 * meet a bucket of self sorted). No reference counterpart as a call — it is `dst = self.clone(); dst |= other`
 * (/root/reference/src/cbl.rs:433-449) without the copy: the device merge writes a new arena anyway. dst's previous content is dropped;
 * dst, self and other are three different contexts of equal K / PREFIX_BITS / canonical, dst and self on the same device. */
int cblx_merge_from(cblx_ctx* dst, cblx_ctx* self, cblx_ctx* other);

/* dst = what `&mut a OP &mut b` returns (/root/reference/src/cbl.rs:411-431, 451-471, 491-511, 531-551 -> src/wordset/set_ops.rs:78-121, 159-190,
 * 241-279, 319-364 -> src/trievec/set_ops.rs): a bucket only one operand holds is cloned as stored (kind and order kept; AND keeps none, SUB only
 * a's), a bucket both hold becomes a Vec of the result in ascending order whatever its length, and is dropped when empty. a and b keep their sets and
 * are left as the reference leaves them: on every prefix both hold, a Vec bucket of either is sorted ascending (also where the result is empty).
 * Pending inserts of a and b are applied first. dst's previous content and pending work are dropped as cblx_merge_from drops them; dst takes a's
 * canonical flag. CBLX_EINVAL, with the three contexts unchanged: dst, a and b not three different contexts, K / PREFIX_BITS differ, a and b differ in
 * `canonical`, op > 3, or the contexts live on different devices. On any other error (a flush of a or b that fails, CBLX_ENOMEM) dst's previous
 * content is lost, as with cblx_merge_from. The assigning forms (`&=`, `-=`, `^=`) have another bucket layout: cblx_set_op_assign. */
#define CBLX_SETOP_OR 0
#define CBLX_SETOP_AND 1
#define CBLX_SETOP_SUB 2
#define CBLX_SETOP_XOR 3
int cblx_set_op(cblx_ctx* dst, cblx_ctx* a, cblx_ctx* b, uint32_t op);
/* a OP= &mut b: a holds what the reference's `a &= &mut b` (CBLX_SETOP_AND), `a -= &mut b` (SUB) or `a ^= &mut b` (XOR) leaves in a, b what it leaves in b
 * (src/cbl.rs:473-489, 513-529, 553-569 -> src/wordset/set_ops.rs:192-239, 281-317, 366-410 -> src/trievec/set_ops.rs:101-129, 163-187, 226-257).
 * A bucket only a holds is dropped (AND) or kept as stored (SUB, XOR); a bucket only b holds is cloned as stored (XOR). A bucket both hold keeps a's kind:
 * a Trie holds the result in ascending order whatever its length, a Vec is sorted, takes the words only b holds in ascending order at its end (XOR) and loses
 * its deletions by swap_remove on ascending indices in reverse (src/trievec/mod.rs:146-168), so it stays a Vec above 1024 words; a bucket that comes out
 * empty leaves the index. On every prefix both hold, a Vec bucket of b ends up sorted ascending; b's other buckets and a's untouched buckets keep their order.
 * CBLX_SETOP_OR is cblx_merge_assign(a, b). Pending inserts of a and b are applied first. CBLX_EINVAL, with both contexts unchanged: a == b, K /
 * PREFIX_BITS differ, a and b differ in `canonical`, op > 3, or the contexts live on different devices. */
int cblx_set_op_assign(cblx_ctx* a, cblx_ctx* b, uint32_t op);
/* dst = CBL::merge (op = CBLX_SETOP_OR) or CBL::intersect (CBLX_SETOP_AND) of the n operands srcs[0 .. n) (/root/reference/src/cbl.rs:106-124 ->
 * src/wordset/set_ops.rs:11-42, 49-75). merge: a bucket exactly one operand holds is cloned as stored (kind and order kept); a bucket two or more hold becomes
 * a Vec of the ascending union whatever its length, and every holder's Vec bucket on that prefix is sorted ascending; operands that lack the prefix are
 * untouched. intersect: only prefixes ALL operands hold are visited; there every operand's Vec bucket is sorted ascending and the result is a Vec of the
 * ascending intersection, dropped when empty — so intersect of one index turns each of its buckets into an ascending Vec, and an empty operand makes the result
 * empty and leaves every operand as it is. For n = 2 both equal cblx_set_op byte for byte, operands included; a fold of cblx_set_op over more operands gives
 * the same SET but other operand and result bytes. dst's content is replaced; pending inserts of every operand are applied first.
 * CBLX_EINVAL, with every context unchanged: n == 0, n > CBLX_SETOP_MAX_OPERANDS, a null entry, dst among srcs, the same context twice, K / PREFIX_BITS /
 * `canonical` / device differ, or op is CBLX_SETOP_SUB / XOR (the reference has no n-ary form of them). */
#define CBLX_SETOP_MAX_OPERANDS 64
int cblx_set_op_many(cblx_ctx* dst, cblx_ctx* const* srcs, uint32_t n, uint32_t op);
/* dst = the k-mers at least t of the n operands srcs[0 .. n) hold, 1 <= t <= n (the reference has no such operation, the rules are
 * fixed here). t = 1 is cblx_set_op_many with CBLX_SETOP_OR byte for byte, result and operands. t >= 2: a prefix fewer than t operands hold is not visited —
 * no result bucket, no operand changes there; on a prefix t or more hold every holder's Vec bucket is sorted ascending (Tries are untouched) and the result
 * bucket is a Vec of the ascending values t holders or more hold, whatever its length, dropped when empty. So for n >= 2, t = n is cblx_set_op_many with
 * CBLX_SETOP_AND byte for byte. An empty operand counts towards n and holds nothing; with fewer than t non-empty operands the result is empty and nothing is
 * sorted. dst's content is replaced; pending inserts of every operand are applied first. CBLX_EINVAL, with every context unchanged: as cblx_set_op_many —
 * n == 0, n > CBLX_SETOP_MAX_OPERANDS, a null entry, dst among srcs, the same context twice, K / PREFIX_BITS / `canonical` / device differ — or t == 0 or
 * t > n. */
int cblx_set_at_least(cblx_ctx* dst, cblx_ctx* const* srcs, uint32_t n, uint32_t t);
/* hist[j] = the number of distinct k-mers exactly j of the n operands hold, j = 0 .. n (hist has n + 1 entries, hist[0] = 0): sum of j * hist[j] = the sum of
 * the counts, sum of hist[j] = the size of the merge, hist[n] = the size of the intersection. No index is built, but this is NOT cblx_intersection_count's
 * untouched-operands guarantee: it visits what a merge visits and leaves the operands as a merge does — on every prefix two or more operands hold, their Vec
 * buckets end up sorted ascending; the sets are unchanged. Buckets one operand holds add their length from the directory alone. Pending inserts of every
 * operand are applied first. CBLX_EINVAL, with every context unchanged: n == 0, n > CBLX_SETOP_MAX_OPERANDS, a null argument or entry, the same context
 * twice, or K / PREFIX_BITS / `canonical` / device differ. */
int cblx_occupancy_counts(cblx_ctx* const* srcs, uint32_t n, uint64_t* hist);
/* *common = |a AND b|, the number of k-mers both indexes hold, without building an index and without touching the operands: unlike
 * cblx_set_op with CBLX_SETOP_AND nothing is sorted — cblx_serialize of a and of b gives the same bytes before and after the call, kinds and stored order of the
 * Vec buckets included. With |a| and |b| (cblx_count) this one number gives the sizes of union, difference and symmetric difference, Jaccard and containment.
 * Pending inserts of both operands are applied first (an observer, as cblx_set_op is). a == b is allowed and gives cblx_count(a); an empty operand gives 0;
 * neither launches a kernel. stats (CBLX_COMMON_STATS entries, or NULL) receives [0] the prefixes both hold and [1] .. [4] how many of those buckets each route
 * took: one wave, one workgroup, merge path, sliced (all zero where no kernel ran). CBLX_EINVAL, with both contexts unchanged: a null argument, K / PREFIX_BITS
 * differ, a and b differ in `canonical`, or the contexts live on different devices. */
#define CBLX_COMMON_STATS 5
int cblx_intersection_count(cblx_ctx* a, cblx_ctx* b, uint64_t* common, uint64_t* stats);
/* The same for every pair of the n operands srcs[0 .. n): out[i * n + j] = out[j * n + i] = |S_i AND S_j| (every unordered pair computed once),
 * out[i * n + i] = cblx_count(S_i); out holds n * n entries, row-major. Every operand's pending inserts are applied once, up front. CBLX_EINVAL, with every
 * context unchanged: n == 0, n > CBLX_SETOP_MAX_OPERANDS, a null entry, the same context twice, or K / PREFIX_BITS / `canonical` / device differ. */
int cblx_intersection_counts(cblx_ctx* const* srcs, uint32_t n, uint64_t* out);
/* The HIP device ordinal the context lives on (cblx_params.device = -1 resolved at creation). */
int cblx_get_device(const cblx_ctx* ctx, int32_t* out);

/* Walk the resident buckets in ascending prefix order (lets a Rust shim rebuild a WordSet, and tests
 * compare bucket contents): kind 0 = Vec (stored = first-occurrence order), 1 = Trie (ascending).
 * Suffix i of the bucket is (hi[i] << 64) | lo[i]; hi is NULL when SUFFIX_BITS <= 64. Return non-zero
 * from the callback to stop. */
typedef int (*cblx_bucket_cb)(void* user, uint32_t prefix, int kind, uint64_t len, const uint64_t* lo,
                              const uint64_t* hi);
int cblx_export_buckets(cblx_ctx* ctx, cblx_bucket_cb cb, void* user);

/* CBL::contains_seq (src/cbl.rs:311-324): one byte (0/1) per k-mer of one sequence, into `out[cap]`. */
int cblx_contains_seq(cblx_ctx* ctx, const uint8_t* seq, uint64_t len, uint8_t* out, uint64_t cap, uint64_t* n);
/* The same for a batch of sequences in one pass (the loop of `cbl query`, examples/cbl.rs:205-228): flags of sequence 0,
 * then sequence 1, ... (`out` may be NULL when only the tallies are wanted); *n_out = k-mers queried, *positive = flags
 * set. Every sequence must hold at least K bytes (CBLX_ESHORT otherwise, nothing is queried).
 * _device: d_bases (16-byte aligned, 16 readable bytes past the end) / d_offsets / d_out are device pointers. */
int cblx_contains_seqs(cblx_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n, uint8_t* out, uint64_t cap,
                       uint64_t* n_out, uint64_t* positive);
int cblx_contains_seqs_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n, uint8_t* d_out,
                              uint64_t cap, uint64_t* n_out, uint64_t* positive);
/* `cbl query <index> <fastx>` (examples/cbl.rs:205-228): contains_seq for every record of a FASTA/FASTQ(.gz) file, read like
 * cblx_insert_fastx_file; *total = k-mers queried, *positive = those found. The index is not modified. */
int cblx_query_fastx_file(cblx_ctx* ctx, const char* path, uint64_t* n_records, uint64_t* total, uint64_t* positive);
/* ---- per-sequence tallies: which of my reads match the index? CBL::contains_seq (src/cbl.rs:311-324) for every sequence of a batch, reduced where the
 * flags are made to the pair the loop of `cbl query` (examples/cbl.rs:205-228) keeps per file: seq_total[i] = k-mers of sequence i queried (the length of its
 * contains_seq result: what get_seq_words yields, bytes that are not ACGT skipped), seq_positive[i] = those found. n entries each, either array may be NULL,
 * every entry is written. The flags are produced and summed on the device and never cross to the host: 8 bytes per sequence come back instead of a byte per
 * k-mer. *n_out / *positive are the tallies of the whole batch as cblx_contains_seqs returns them: the sums of the two arrays. Contract of the batch query:
 * a sequence shorter than K is CBLX_ESHORT and nothing is queried or written, n == 0 is a no-op, the index is not modified, one call takes fewer than
 * 2^32 - 16 k-mers. _device: device pointers for bases, offsets (as for cblx_contains_seqs_device) and the two arrays.
 * _flags_counts_device: the same call that also leaves the flags in d_out[cap] (device), as cblx_contains_seqs_device does. */
int cblx_contains_seqs_counts(cblx_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n, uint32_t* seq_total, uint32_t* seq_positive,
                              uint64_t* n_out, uint64_t* positive);
int cblx_contains_seqs_counts_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n, uint32_t* d_seq_total,
                                     uint32_t* d_seq_positive, uint64_t* n_out, uint64_t* positive);
int cblx_contains_seqs_flags_counts_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n, uint8_t* d_out, uint64_t cap,
                                           uint32_t* d_seq_total, uint32_t* d_seq_positive, uint64_t* n_out, uint64_t* positive);
/* cblx_query_fastx_file (`cbl query`, examples/cbl.rs:205-228) that keeps the pair of every record: rec_total[i] / rec_positive[i] (host, cap entries each,
 * either may be NULL) for record i of the file, 0-based, in file order. A file of more than cap records is CBLX_ERANGE with *n_records = its record count
 * (cblx_stage_fastx_blocks with block = 0 counts in advance); the arrays then hold only the records of the flushes that fitted. With both arrays NULL it is
 * cblx_query_fastx_file. */
int cblx_query_fastx_file_counts(cblx_ctx* ctx, const char* path, uint32_t* rec_total, uint32_t* rec_positive, uint64_t cap, uint64_t* n_records,
                                 uint64_t* total, uint64_t* positive);
/* ---- a batch against a PANEL of up to CBLX_SETOP_MAX_OPERANDS indexes in one pass (ours): for every sequence, how many of its k-mers
 * each of srcs[0 .. n) holds — screening against several references, classification. The k-mers, their order and seq_total[nseq] are exactly those of
 * cblx_contains_seqs_counts; row j of seq_positive (n * nseq entries, [j * nseq + s]) is what cblx_contains_seqs_counts(srcs[j], ...) returns; bit j of
 * kmer_mask[i] (mask_cap words, one per k-mer) is flag i of cblx_contains_seqs(srcs[j], ...), bits n and above are 0; positive[j] (n entries) is the sum of
 * row j and *n_out the number of k-mers. Any of the arrays may be NULL; every entry of every given array is written. The operands are observers: pending
 * inserts are applied first, nothing is modified or sorted (cblx_serialize of every operand gives the same bytes before and after). An empty operand counts
 * towards n: its row and its bit are 0. CBLX_EINVAL: n == 0, n > CBLX_SETOP_MAX_OPERANDS, a null argument or entry, the same context twice, or K /
 * PREFIX_BITS / `canonical` / device differ. A sequence shorter than K is CBLX_ESHORT and mask_cap smaller than the number of k-mers CBLX_ERANGE: nothing is
 * written then. nseq == 0 writes *n_out = 0 and positive[j] = 0. One call takes fewer than 2^32 - 16 k-mers. The work runs on the stream of the first
 * non-empty operand. _device: device pointers for bases, offsets (as for cblx_contains_seqs_device) and the three arrays; n_out and positive stay host. */
int cblx_contains_seqs_counts_many(cblx_ctx* const* srcs, uint32_t n, const uint8_t* bases, const uint64_t* offsets, uint64_t nseq, uint32_t* seq_total,
                                   uint32_t* seq_positive, uint64_t* kmer_mask, uint64_t mask_cap, uint64_t* n_out, uint64_t* positive);
int cblx_contains_seqs_counts_many_device(cblx_ctx* const* srcs, uint32_t n, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t nseq,
                                          uint32_t* d_seq_total, uint32_t* d_seq_positive, uint64_t* d_kmer_mask, uint64_t mask_cap, uint64_t* n_out,
                                          uint64_t* positive);
/* CBL::contains_all (src/cbl.rs:293-307): *out = 1 iff every k-mer of the sequence is in the set. */
int cblx_contains_all(cblx_ctx* ctx, const uint8_t* seq, uint64_t len, int* out);

/* Packed k-mers: k-mer i is IntKmer::to_int() (2K bits, first base most significant, src/kmer.rs:200-202) given as
 * lo[i] (low 64 bits) and hi[i] (the rest; `hi` may be NULL when K <= 31, must not be when K >= 33).
 *   cblx_insert_kmers   = n successive CBL::insert calls (src/cbl.rs:226-228 -> get_word :199-206 -> WordSet::insert
 *                         src/wordset/mod.rs:97-120); was_absent[i] (may be NULL) is the i-th call's return value:
 *                         1 iff the k-mer was neither in the set nor earlier in this batch.
 *   cblx_contains_kmers = CBL::contains (src/cbl.rs:219-221) for each k-mer, one byte (0/1) each.
 * In a canonical index the k-mer is replaced by its canonical form first, as in the reference. A k-mer with bits set
 * above 2K is refused (CBLX_EINVAL) and nothing is inserted. */
int cblx_insert_kmers(cblx_ctx* ctx, const uint64_t* lo, const uint64_t* hi, uint64_t n, uint8_t* was_absent);
int cblx_contains_kmers(cblx_ctx* ctx, const uint64_t* lo, const uint64_t* hi, uint64_t n, uint8_t* out);
/* ---- removal: CBL::remove_seq (src/cbl.rs:343-354), CBL::remove (:233-235) and `cbl remove` (examples/cbl.rs:250-269). The index after the call holds the
 * bytes the reference's sequential replay leaves: a Vec bucket loses its words by swap_remove in stream order, a Trie bucket by deletion,
 * and a Trie of at most 1024 words at the end of a GROUP — a maximal run of consecutive words of one remove_batch call with equal prefix — becomes an ascending Vec
 * there (adapt_container_shrink runs after every group whose prefix is present, hit or no hit). A bucket that comes out empty leaves the index.
 * Rules: pending inserts are applied first; a removal runs before the call returns, it is not enqueued; a sequence shorter than K is CBLX_ESHORT with the
 * behaviour of the matching insert entry point (a batch, host or device, whatever its size: nothing is removed — all lengths are checked before the first
 * sub-batch; a file: the records in front of it are removed); removal from an empty index or with
 * n == 0 is a no-op that returns 0; bytes that are not ACGT are skipped exactly as insertion skips them; a batch has the insert path's size limit (the sequence forms
 * are cut into sub-batches at sequence boundaries, one call of cblx_remove_words_device / cblx_remove_kmers takes fewer than 2^32-16 words). cblx_remove_seq called once per
 * read costs a device round trip and a pass over the index per call: cblx_remove_fastx_file and the batch forms batch for it; there is no per-record queue for removals. */
/* WordSet::remove_batch (src/wordset/mod.rs:218-237) on already transformed words: ONE call = ONE batch, its groups are the maximal runs of
 * consecutive words with equal prefix. Device word arrays as for cblx_insert_words_device. */
int cblx_remove_words_device(cblx_ctx* ctx, const uint64_t* d_lo, const void* d_hi, uint64_t n);
/* CBL::remove_seq (src/cbl.rs:343-354) for sequence 0, then 1, ...: one remove_batch per chunk of get_seq_words. */
int cblx_remove_seq(cblx_ctx* ctx, const uint8_t* seq, uint64_t len);
int cblx_remove_seqs(cblx_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n);
int cblx_remove_seqs_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n);
/* the reader loop of `cbl remove` (examples/cbl.rs:250-265), read like cblx_insert_fastx_file */
int cblx_remove_fastx_file(cblx_ctx* ctx, const char* path, uint64_t* n_records);
/* n successive CBL::remove calls (src/cbl.rs:233-235 -> src/wordset/mod.rs:122-137; every call a group of its own); was_present[i] (may be
 * NULL) is the i-th call's return value: 1 iff the k-mer was in the set and not removed earlier in this batch. Packed k-mers, canonical
 * handling and the refusal of bits above 2K as for cblx_insert_kmers. */
int cblx_remove_kmers(cblx_ctx* ctx, const uint64_t* lo, const uint64_t* hi, uint64_t n, uint8_t* was_present);
/* CBL::iter (src/cbl.rs:358-361): every k-mer of the set, packed as above, in the reference's iteration order
 * (prefixes ascending; a Vec bucket in stored order, a Trie bucket ascending), recovered from its word by
 * revert_necklace_pos (src/necklace/mod.rs:29-31). *n = count(); `hi` may be NULL when K <= 31. */
int cblx_export_kmers(cblx_ctx* ctx, uint64_t* lo, uint64_t* hi, uint64_t cap, uint64_t* n);
/* ---- reading the index out in pieces. Element e of the ITERATION ORDER is the e-th k-mer CBL::iter yields (order as for cblx_export_kmers). The range
 * calls take elements [first, first + n): first > count() is CBLX_EINVAL, a range that runs past the end is clamped, first == count() or n == 0 writes
 * nothing and returns 0. Device workspace is O(n) plus one uint64_t per bucket, not O(count()). Pending inserts are applied first. The index must not
 * change between the calls that walk it: positions are positions in the order of the moment. */
/* CBL::iter, elements [first, first + n) of the iteration order; *written = min(n, count - first). Host / device outputs. `hi` may be NULL when
 * K <= 31, is CBLX_EINVAL when K >= 33. */
int cblx_export_kmers_range(cblx_ctx* ctx, uint64_t first, uint64_t n, uint64_t* lo, uint64_t* hi, uint64_t* written);
int cblx_export_kmers_range_device(cblx_ctx* ctx, uint64_t first, uint64_t n, uint64_t* d_lo, uint64_t* d_hi, uint64_t* written);
/* ---- the index as the node set of a de Bruijn graph: Kmer::successors / Kmer::predecessors (src/kmer.rs:82-90), each looked up with
 * CBL::contains (src/cbl.rs:219-221). With MASK = 2^(2K) - 1, append(x, c) = ((x << 2) | c) & MASK and prepend(x, c) = (x >> 2) | (c << 2(K - 1)) for a base
 * code c = 0 .. 3 (A 0, C 1, T 2, G 3), the NEIGHBOUR MASK of a packed k-mer x is one byte: bit c = contains(append(x, c)), bit 4 + c = contains(prepend(x, c)).
 * A canonical index canonicalises the neighbour, as cblx_contains_kmers does; x itself is taken as given and need not be in the set. A self-loop sets its
 * bits like any other neighbour, and in a canonical index two bits may name the same stored k-mer: both are set. All five calls are observers: pending inserts
 * are applied first, nothing is modified or sorted (cblx_serialize gives the same bytes before and after). An empty index gives zero masks and a zero table.
 * The work runs in passes of CBLX_NEIGHBOR_PASS k-mers (environment, read per call; default 2^22, at most 2^28): 8 words and 8 flag bytes of device scratch per
 * k-mer of a pass. The 8 m words of a pass are answered as a flags query is: by the join where the word has at most 96 bits and a suffix of at most 64, and
 * 8 m >= CBLX_QUERY_JOIN_MIN (default 2^22); one bucket read per word otherwise. */
/* masks[i] = the neighbour mask of packed k-mer i (lo / hi as for cblx_contains_kmers: hi may be NULL when K <= 31). A refusal writes nothing: a null
 * argument with n > 0 or a k-mer with bits set above 2K is CBLX_EINVAL, wherever in the batch it stands. n == 0 succeeds and writes nothing.
 * _device: device pointers for the three arrays. */
int cblx_neighbors_kmers(cblx_ctx* ctx, const uint64_t* lo, const uint64_t* hi, uint64_t n, uint8_t* masks);
int cblx_neighbors_kmers_device(cblx_ctx* ctx, const uint64_t* d_lo, const uint64_t* d_hi, uint64_t n, uint8_t* d_masks);
/* The masks of elements [first, first + n) of the iteration order: masks[i] belongs to the k-mer cblx_export_kmers_range writes at index i. Argument rules
 * and status codes of the range calls above; *written = min(n, count - first). Device workspace is O(CBLX_NEIGHBOR_PASS), not O(n). */
int cblx_neighbors_range(cblx_ctx* ctx, uint64_t first, uint64_t n, uint8_t* masks, uint64_t* written);
int cblx_neighbors_range_device(cblx_ctx* ctx, uint64_t first, uint64_t n, uint8_t* d_masks, uint64_t* written);
/* The degree table of the graph: table[5 * out + in] = the k-mers of the index with out = popcount(mask & 15) successors and in = popcount(mask >> 4)
 * predecessors in the set; the 25 entries add up to cblx_count. The masks stay on the device: 200 bytes come back. */
int cblx_degree_table(cblx_ctx* ctx, uint64_t table[25]);
/* The same elements as text: K bytes of IntKmer::to_nucs (b"ACTG"[code], first base first: src/kmer.rs:26-27) + '\n' each (examples/cbl.rs:190-193). cap in
 * bytes; *written_bytes = (K + 1) * min(n, count - first). When cap is smaller than that the call returns CBLX_ERANGE, *written_bytes is the need and
 * nothing is written. */
int cblx_list_range(cblx_ctx* ctx, uint64_t first, uint64_t n, uint8_t* buf, uint64_t cap, uint64_t* written_bytes);
int cblx_list_range_device(cblx_ctx* ctx, uint64_t first, uint64_t n, uint8_t* d_buf /* 16-byte aligned */, uint64_t cap, uint64_t* written_bytes);
/* `cbl list` (examples/cbl.rs:177-201): every k-mer as a line, streamed to a file descriptor in order. chunk_kmers = k-mers per device chunk (0 = default:
 * 2^21, 64 MiB of text at K = 31). While the device emits chunk i, chunk i - 1 crosses to pinned memory and chunk i - 2 is handed to write(): two device and
 * two pinned buffers of one chunk each, whatever the size of the index. A short or failed write is CBLX_EINVAL with the errno text; what was written
 * before it stays written. *n_kmers = count(). */
int cblx_list_to_fd(cblx_ctx* ctx, int fd, uint64_t chunk_kmers, uint64_t* n_kmers);
int cblx_list_to_file(cblx_ctx* ctx, const char* path, uint64_t chunk_kmers, uint64_t* n_kmers);   /* create / truncate, then the above */
/* ---- unitigs. The ORDINAL of a k-mer is its index in the iteration order: the index at which cblx_export_kmers_range writes it.
 * rank[i] = the ordinal of packed k-mer i, UINT64_MAX when the set does not hold it: the inverse of the iteration order. Argument rules of
 * cblx_neighbors_kmers: hi may be NULL when K <= 31; a null argument with n > 0 or a k-mer with bits set above 2K, wherever in the batch, is CBLX_EINVAL
 * and nothing is written; n == 0 succeeds. A canonical index canonicalises the query, as cblx_contains_kmers does. An observer: pending inserts are
 * applied first, nothing is modified or sorted. _device: device pointers for the three arrays. */
int cblx_rank_kmers(cblx_ctx* ctx, const uint64_t* lo, const uint64_t* hi, uint64_t n, uint64_t* rank);
int cblx_rank_kmers_device(cblx_ctx* ctx, const uint64_t* d_lo, const uint64_t* d_hi, uint64_t n, uint64_t* d_rank);
/* The compaction table of a NON-CANONICAL index. An edge x -> y (y = append(x, c), both in the set) is SIMPLE when x has one successor and y one
 * predecessor in the set (the degrees of the neighbour masks; a self-loop counts on both sides). The simple edges cut the set into disjoint paths and
 * cycles: the UNITIGS. The head of a path is its k-mer without a simple in-edge; a cycle of simple edges only has none: its head is its member with the
 * smallest ordinal, and the unitig is CIRCULAR. Unitigs are numbered 0 .. U - 1 by ascending ordinal of their heads.
 *   per k-mer:   unitig[ordinal], offset[ordinal] = the simple edges from the head to it                          (cap_kmers elements each)
 *   per unitig:  head[u] = the head's ordinal, length[u] = its k-mers, flags[u] bit 0 = circular                   (cap_unitigs elements each)
 * Any array may be NULL and is then not written; with all five NULL the call only counts. *n_kmers = count(), *n_unitigs = U, *n_circular are always
 * set (any may be NULL). A capacity below the need of an array that is given is CBLX_ERANGE: the counts are set and nothing is written. A canonical
 * index is CBLX_EINVAL (its unitigs are the bidirected ones: cblx_biunitig_table); 2^32 - 16 k-mers or more are CBLX_ERANGE (ordinals are 32-bit inside). An empty index
 * gives U = 0. Numbering and the rotation of a circular unitig follow the iteration order, so they follow the Vec buckets' first-occurrence order.
 * An observer; every call recomputes. Device workspace: about 25 bytes per k-mer. _device: device pointers for the five arrays. */
int cblx_unitig_table(cblx_ctx* ctx, uint32_t* unitig, uint32_t* offset, uint64_t cap_kmers, uint32_t* head, uint32_t* length, uint8_t* flags,
                      uint64_t cap_unitigs, uint64_t* n_kmers, uint64_t* n_unitigs, uint64_t* n_circular);
int cblx_unitig_table_device(cblx_ctx* ctx, uint32_t* d_unitig, uint32_t* d_offset, uint64_t cap_kmers, uint32_t* d_head, uint32_t* d_length, uint8_t* d_flags,
                             uint64_t cap_unitigs, uint64_t* n_kmers, uint64_t* n_unitigs, uint64_t* n_circular);
/* The text of the unitigs, lines in unitig order: the K letters of the head (b"ACTG"[code], first base first, as cblx_list_range writes them), then the
 * last letter of every following k-mer in offset order, then '\n': K + length bytes a line, count() + U * K bytes in all. A circular unitig is written
 * open, from its head. *bytes = the need, *n_unitigs = U. d_buf == NULL gives the sizes only; cap < need is CBLX_ERANGE with the need reported and
 * nothing written. */
int cblx_unitigs_text_device(cblx_ctx* ctx, uint8_t* d_buf, uint64_t cap, uint64_t* bytes, uint64_t* n_unitigs);
/* The same text streamed to a file descriptor: it is built once on the device and leaves in chunks of chunk_bytes (0 = default: the bytes of a
 * cblx_list_to_fd chunk) through two pinned buffers, as the list does; the error rules are cblx_list_to_fd's. */
int cblx_unitigs_to_fd(cblx_ctx* ctx, int fd, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* bytes);
int cblx_unitigs_to_file(cblx_ctx* ctx, const char* path, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* bytes);   /* create / truncate, then the above */
/* ---- bidirected unitigs: the compaction of a CANONICAL index with odd K. Stored k-mer i (ordinal i, x_i its stored form) has two
 * ORIENTED copies: (i, 0) spells x_i and (i, 1) spells rc(x_i); the mirror of (i, s) is (i, 1 - s). There is an edge (i, s) -> (j, t) when
 * sigma(j, t) = append(sigma(i, s), c) and x_j is in the set; edges come in mirror pairs, (j, 1 - t) -> (i, 1 - s). Degrees are those of the neighbour
 * mask m of i: out(i, 0) = popcount(m & 15), in(i, 0) = popcount(m >> 4), out(i, 1) = in(i, 0), in(i, 1) = out(i, 0). An edge is SIMPLE when
 * out(i, s) = 1, in(j, t) = 1 and j != i. An edge between a stored k-mer and itself — the hairpin (i, s) -> (i, 1 - s), the homopolymer loop — is never
 * simple, though it counts in the degrees: THIS DIFFERS FROM cblx_unitig_table, where poly-A alone is a circular unitig; here it is a unitig of
 * length 1 that is not circular. The simple edges cut the oriented k-mers into paths and cycles that come in distinct mirror pairs; a UNITIG is one
 * image of each pair. Of a path with head (h, s) and tail (t, u) the image with h < t is kept, or with h = t and s = 0 (length 1). Of a cycle of simple
 * edges only the head is the member with the smallest ordinal, the image kept is the one where that head has s = 0, and the unitig is CIRCULAR.
 * Unitigs are numbered by ascending ordinal of their heads; every stored k-mer lies on exactly one.
 *   per k-mer:   unitig[ordinal], offset[ordinal] = the simple edges from the head, reversed[ordinal] = the s of its copy on the kept image (uint8)
 *   per unitig:  head[u] = the head's ordinal, length[u], flags[u] bit 0 = circular
 * The conventions of cblx_unitig_table: any array may be NULL, with all six NULL the call only counts; the counts are always set; a short capacity is
 * CBLX_ERANGE with the need reported and nothing written; an observer; an empty index gives U = 0. A non-canonical index is CBLX_EINVAL (it has
 * cblx_unitig_table), an even K is CBLX_EINVAL, 2^31 - 8 k-mers or more are CBLX_ERANGE (the ids 2 i + s are 32-bit). Device workspace: about 50 bytes
 * per k-mer. _device: device pointers for the six arrays. */
int cblx_biunitig_table(cblx_ctx* ctx, uint32_t* unitig, uint32_t* offset, uint8_t* reversed, uint64_t cap_kmers, uint32_t* head, uint32_t* length, uint8_t* flags,
                        uint64_t cap_unitigs, uint64_t* n_kmers, uint64_t* n_unitigs, uint64_t* n_circular);
int cblx_biunitig_table_device(cblx_ctx* ctx, uint32_t* d_unitig, uint32_t* d_offset, uint8_t* d_reversed, uint64_t cap_kmers, uint32_t* d_head, uint32_t* d_length,
                               uint8_t* d_flags, uint64_t cap_unitigs, uint64_t* n_kmers, uint64_t* n_unitigs, uint64_t* n_circular);
/* The text, lines in unitig order: the K letters of sigma(head), then the last letter of sigma of every following member in offset order (for a reversed
 * member the complement of its stored form's first base), then '\n': count() + U * K bytes in all. A circular unitig is written open, from its head. The
 * rules of cblx_unitigs_text_device / cblx_unitigs_to_fd / cblx_unitigs_to_file; a refused cblx_biunitigs_to_file does not create the file. */
int cblx_biunitigs_text_device(cblx_ctx* ctx, uint8_t* d_buf, uint64_t cap, uint64_t* bytes, uint64_t* n_unitigs);
int cblx_biunitigs_to_fd(cblx_ctx* ctx, int fd, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* bytes);
int cblx_biunitigs_to_file(cblx_ctx* ctx, const char* path, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* bytes);
/* ---- the links between the unitigs and the GFA text of the compacted graph. The form follows the index: a non-canonical index
 * gives the links between the unitigs of cblx_unitig_table, a canonical one those between the bidirected unitigs of cblx_biunitig_table; unitig numbers,
 * offsets and `reversed` are exactly those tables', and so are the refusals (an even K of a canonical index is CBLX_EINVAL, too many k-mers CBLX_ERANGE).
 * Unitig u has a kept image, side 0 ('+'), and in the bidirected form a mirror image, side 1 ('-'): its oriented k-mers (i, 1 - s) in reverse offset order.
 * SLOT 2 u + side; in the plain form only even slots hold anything. A LINK is every edge of the graph — self-edges and hairpins included — that does not
 * join two consecutive offsets of one image (so the cut edge of a circular unitig is a link u+ -> u+). Every link leaves the last oriented k-mer of an image
 * and enters the first one of an image.
 *   link_start[slot]   uint64, 2 U + 1 entries: the links that leave `slot` are [link_start[slot], link_start[slot + 1]); link_start[2 U] = L
 *   link_to[l]         uint32, L entries: the unitig the link enters
 *   link_rev[l]        uint8, L entries: 0 when it enters the head of that unitig's kept image ('+'), 1 when the head of its mirror ('-'); plain form: 0
 * Within a slot the links are in ascending code of the base appended. Bidirected links come in mirror pairs: (a -> b) with (b ^ 1 -> a ^ 1) in slot ids; a
 * link with b = a ^ 1 is its own mirror and occurs once. Any array may be NULL and is then not written; with all three NULL the call only counts.
 * *n_unitigs = U and *n_links = L are always set. cap_starts < 2 U + 1 (with link_start) or cap_links < L (with link_to or link_rev) is CBLX_ERANGE: the
 * needs are reported and nothing is written. An empty index gives U = L = 0 and link_start[0] = 0. */
int cblx_gfa_links(cblx_ctx* ctx, uint64_t* link_start, uint64_t cap_starts, uint32_t* link_to, uint8_t* link_rev, uint64_t cap_links, uint64_t* n_unitigs,
                   uint64_t* n_links);
int cblx_gfa_links_device(cblx_ctx* ctx, uint64_t* d_link_start, uint64_t cap_starts, uint32_t* d_link_to, uint8_t* d_link_rev, uint64_t cap_links,
                          uint64_t* n_unitigs, uint64_t* n_links);
/* GFA 1.0: "H\tVN:Z:1.0\n", then "S\t<u>\t<line u of the unitig text>\n" for u = 0 .. U - 1, then "L\t<u>\t<+|->\t<v>\t<+|->\t<K - 1>M\n" for the links in table
 * order; numbers are decimal without padding. Of a mirror pair of links one L line is written — the link whose (from slot, to slot) is lexicographically
 * <= its mirror's (to slot ^ 1, from slot ^ 1) — and a link that is its own mirror once; the plain form writes every link. *n_links = the L lines written.
 * An empty index gives the 11 header bytes. d_buf, cap and *bytes as in cblx_unitigs_text_device; fd, path and chunk_bytes (0 = that text's default) as
 * in cblx_unitigs_to_fd / cblx_unitigs_to_file; a refused cblx_gfa_to_file does not create the file. */
int cblx_gfa_text_device(cblx_ctx* ctx, uint8_t* d_buf, uint64_t cap, uint64_t* bytes, uint64_t* n_unitigs, uint64_t* n_links);
int cblx_gfa_to_fd(cblx_ctx* ctx, int fd, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* bytes);
int cblx_gfa_to_file(cblx_ctx* ctx, const char* path, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* n_links, uint64_t* bytes);
/* ---- tip clipping on the compacted graph. The form follows the index as in the link table: unitig numbers, lengths, `reversed` and the
 * refusals are those of cblx_unitig_table (a non-canonical index) or cblx_biunitig_table (a canonical one).
 *   right[u]   uint8: the out-degree of the last oriented k-mer of unitig u's kept image = link_start[2 u + 1] - link_start[2 u]
 *   left[u]    uint8: the in-degree of its first one; bidirected form: link_start[2 u + 2] - link_start[2 u + 1]; plain form: the links whose link_to is u
 * Self-edges and hairpins count, so a circular unitig has left, right >= 1. With max_kmers >= 1, kind[u] (uint8) is 1, a TIP, when length[u] <= max_kmers and
 * exactly one of left[u], right[u] is 0; 2, ISOLATED, when length[u] <= max_kmers and both are 0; 0 otherwise. counts = {tips, k-mers of the tips, isolated
 * unitigs, k-mers of the isolated unitigs}. Observers with the conventions of cblx_unitig_table: any array may be NULL, *n_unitigs (and counts, unless NULL) is
 * always set, cap_unitigs < U with an array given is CBLX_ERANGE with the need reported and nothing written. max_kmers == 0 is CBLX_EINVAL. */
int cblx_unitig_ends(cblx_ctx* ctx, uint8_t* left, uint8_t* right, uint64_t cap_unitigs, uint64_t* n_unitigs);
int cblx_unitig_ends_device(cblx_ctx* ctx, uint8_t* d_left, uint8_t* d_right, uint64_t cap_unitigs, uint64_t* n_unitigs);
int cblx_tips_mark(cblx_ctx* ctx, uint64_t max_kmers, uint8_t* kind, uint64_t cap_unitigs, uint64_t* n_unitigs, uint64_t counts[4]);
int cblx_tips_mark_device(cblx_ctx* ctx, uint64_t max_kmers, uint8_t* d_kind, uint64_t cap_unitigs, uint64_t* n_unitigs, uint64_t counts[4]);
/* A ROUND compacts the index, marks the unitigs, takes the k-mers of the tips — with CBLX_CLIP_ISOLATED those of the isolated unitigs too — in iteration
 * order and removes their words as ONE WordSet::remove_batch (one group per bucket: the bytes afterwards are what cblx_remove_words_device leaves of that
 * batch). All marked unitigs of a compaction go together: a short stem that forks into two short dead ends is three tips. Round r stops the call with
 * fixpoint = 1 when it selects nothing, and with fixpoint = 0 after its removal when r + 1 == max_rounds; max_rounds == 0 runs until the fixpoint.
 * tips .. isolated_kmers count what was REMOVED, summed over the rounds (the isolated pair stays 0 without the flag); rounds = compactions run. `stats` may be
 * NULL. max_kmers == 0 and unknown flag bits are CBLX_EINVAL; the form's refusals come before anything changes. An empty index: rounds = 1, fixpoint = 1. */
#define CBLX_CLIP_ISOLATED 1u
typedef struct cblx_clip_stats { uint64_t rounds, tips, tip_kmers, isolated, isolated_kmers, kmers_left, fixpoint; } cblx_clip_stats;
int cblx_clip_tips(cblx_ctx* ctx, uint64_t max_kmers, uint32_t flags, uint32_t max_rounds, cblx_clip_stats* stats);
/* ---- connected components of the compacted graph. The form follows the index as in the link table: unitig numbers, lengths, the
 * links and the refusals are those of cblx_gfa_links; the index must also have fewer than 2^31 unitigs (CBLX_ERANGE).
 *   component        a class of the smallest equivalence on the unitigs in which u ~ link_to[l] for every link l that leaves slot 2 u or 2 u + 1: the weakly
 *                    connected components of the de Bruijn graph on the stored k-mers (a unitig and its mirror are one node). Numbered 0 .. C - 1 by
 *                    ascending smallest unitig.
 *   component[u]     uint32, U entries; kmer_component[i] = component[unitig[i]], uint32 per k-mer in iteration order
 *   first[c]         uint32: the smallest unitig of c (strictly ascending); unitigs[c] uint32; kmers[c] uint64 = the sum of length over its unitigs
 *   counts           {k-mers, unitigs U, links L, components C, k-mers of the largest component (0 for an empty index), rounds of the labelling}
 * Observers with the conventions of cblx_unitig_table: any array may be NULL, all NULL counts only, counts (unless NULL) is always set, a capacity below the
 * need with its array given is CBLX_ERANGE with nothing written; capacities are checked before any output is touched. */
int cblx_components(cblx_ctx* ctx, uint32_t* component, uint64_t cap_unitigs, uint32_t* kmer_component, uint64_t cap_kmers, uint32_t* first, uint32_t* unitigs,
                    uint64_t* kmers, uint64_t cap_components, uint64_t counts[6]);
int cblx_components_device(cblx_ctx* ctx, uint32_t* d_component, uint64_t cap_unitigs, uint32_t* d_kmer_component, uint64_t cap_kmers, uint32_t* d_first,
                           uint32_t* d_unitigs, uint64_t* d_kmers, uint64_t cap_components, uint64_t counts[6]);
/* Removes whole components: with min_kmers >= 1 every k-mer of every component with kmers[c] < min_kmers; with CBLX_COMPONENTS_LARGEST (min_kmers must be 0)
 * every k-mer outside the component of most k-mers (a tie goes to the lower number). The selected k-mers are taken in iteration order and their words removed
 * as ONE WordSet::remove_batch, as a round of cblx_clip_tips does. One call is the fixpoint: no other component changes. `stats` may be NULL; largest_kmers is
 * the size before the removal. Unknown flag bits, min_kmers == 0 without the flag and min_kmers != 0 with it are CBLX_EINVAL with nothing removed; min_kmers ==
 * 1 removes nothing. The form's refusals come before anything changes. An empty index: all-zero stats. */
#define CBLX_COMPONENTS_LARGEST 1u
typedef struct cblx_component_stats { uint64_t components, removed_components, removed_kmers, kmers_left, largest_kmers, rounds; } cblx_component_stats;
int cblx_components_filter(cblx_ctx* ctx, uint64_t min_kmers, uint32_t flags, cblx_component_stats* stats);
/* ---- k-mer abundances from reads. The index stays a set: the counts belong to the CALLER, a DEVICE array `d_counts` of n_counts
 * uint32, one per stored k-mer by ORDINAL (its index in the iteration order of the moment, as in cblx_rank_kmers). Every call applies pending inserts first and
 * then refuses n_counts != the number of stored k-mers with CBLX_EINVAL and nothing written or removed: the guard against an array from before a change of
 * the index. Nothing in the index is modified or sorted by the observers: cblx_serialize gives the same bytes afterwards.
 *   occurrence   one k-mer of the batch as cblx_contains_seqs enumerates it: sequence after sequence, get_seq_words order; bytes that are not ACGT are skipped
 *                as there; a sequence shorter than K gives none (it is not refused); a canonical index counts both strands for the one stored k-mer
 *   tally        d_counts[i] = min(2^32 - 1, d_counts[i] + occ_i), occ_i = the occurrences whose word has ordinal i. The call ACCUMULATES; the caller zeroes.
 *                *total = the occurrences, *found = those the index holds. `bases` / `offsets` are host arrays in cblx_abundance_seqs and device arrays (d_bases
 *                16-byte aligned) in the _device form, with the conventions of cblx_contains_seqs*; a batch takes fewer than 2^32 - 16 k-mers (CBLX_ERANGE,
 *                nothing written). An empty index with n_counts == 0 tallies nothing: *found = 0.
 *   spectrum     hist[j] (256 uint64 on the host) = the ordinals with d_counts[i] == j for j < 255; hist[255] = those with d_counts[i] >= 255 */
int cblx_abundance_seqs(cblx_ctx* ctx, const uint8_t* bases, const uint64_t* offsets, uint64_t n, uint32_t* d_counts, uint64_t n_counts, uint64_t* total,
                        uint64_t* found);
int cblx_abundance_seqs_device(cblx_ctx* ctx, const uint8_t* d_bases, const uint64_t* d_offsets, uint64_t n, uint32_t* d_counts, uint64_t n_counts, uint64_t* total,
                               uint64_t* found);
int cblx_abundance_histogram(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, uint64_t hist[256]);
/* Unitig coverage. The form follows the index as in cblx_gfa_links: unitig numbers, lengths and the refusals are those of cblx_unitig_table (a non-canonical
 * index) or cblx_biunitig_table (a canonical one). kc[u] (uint64; a host array, a device array in the _device form) = the sum of d_counts[i] over the k-mers of
 * unitig u, so the sum of kc is the sum of the counts and kc[u] <= length[u] (2^32 - 1); mean coverage is kc[u] / length[u]. *n_unitigs = U is always set. A NULL
 * kc only counts; cap_unitigs < U with kc given is CBLX_ERANGE with the need reported and nothing written. */
int cblx_unitig_coverage(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, uint64_t* kc, uint64_t cap_unitigs, uint64_t* n_unitigs);
int cblx_unitig_coverage_device(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, uint64_t* d_kc, uint64_t cap_unitigs, uint64_t* n_unitigs);
/* The GFA text of cblx_gfa_text_device byte for byte, except that every S line reads "S\t<u>\t<letters>\tLN:i:<length[u] + K - 1>\tKC:i:<kc[u]>\n" (decimal without
 * padding). With d_counts NULL the KC tag and its tab are absent, LN stays, and n_counts is not looked at. The H line and the L lines are as they were, and
 * *n_links keeps its meaning. The other parameters as in cblx_gfa_text_device / cblx_gfa_to_fd / cblx_gfa_to_file; a refused cblx_gfa_tagged_to_file does not
 * create the file. */
int cblx_gfa_tagged_text_device(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, uint8_t* d_buf, uint64_t cap, uint64_t* bytes, uint64_t* n_unitigs,
                                uint64_t* n_links);
int cblx_gfa_tagged_to_fd(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, int fd, uint64_t chunk_bytes, uint64_t* n_unitigs, uint64_t* n_links,
                          uint64_t* bytes);
int cblx_gfa_tagged_to_file(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, const char* path, uint64_t chunk_bytes, uint64_t* n_unitigs,
                            uint64_t* n_links, uint64_t* bytes);
/* Removes the weakly supported k-mers, min_count >= 1. K-mer rule (flags == 0): every ordinal with d_counts[i] < min_count; it works on any index and runs no
 * compaction (unitigs and removed_unitigs stay 0). Unitig rule (CBLX_ABUNDANCE_UNITIGS): every k-mer of every unitig with kc[u] < min_count * length[u], that is
 * mean coverage below min_count in integers. The selected k-mers are taken in iteration order and their words removed as ONE WordSet::remove_batch, as a round
 * of cblx_clip_tips does. d_counts is read, never written; after a call that removed something it no longer matches the index (a Vec bucket loses by
 * swap_remove, so ordinals move): tally again — the n_counts guard refuses the stale array. `stats` may be NULL; kmers is the count before. min_count == 0,
 * unknown flag bits and n_counts != the stored k-mers are CBLX_EINVAL with nothing removed; the form's refusals (unitig rule only) come before anything changes.
 * An empty index: all-zero stats. */
#define CBLX_ABUNDANCE_UNITIGS 1u
typedef struct cblx_abundance_stats { uint64_t kmers, removed_kmers, unitigs, removed_unitigs, kmers_left, min_count; } cblx_abundance_stats;
int cblx_abundance_filter(cblx_ctx* ctx, const uint32_t* d_counts, uint64_t n_counts, uint32_t min_count, uint32_t flags, cblx_abundance_stats* stats);
/* ---- bubble popping on the compacted graph. The form, the unitig numbers, `length`, the slots and the link table are those of
 * cblx_gfa_links; kc is cblx_unitig_coverage's. For an image slot x = 2 p + s: out(x) = the links of slot x, in(x) = the in-degree of that image's head (the
 * links of slot x ^ 1 in the bidirected form, `left` of cblx_unitig_ends in the plain one). Image x of unitig p is a qualified arm from source slot a to target
 * slot T when a -> x is a link, in(x) == out(x) == 1, the one link of x enters T, length[p] <= max_kmers, and p is neither the unitig of a nor that of T. The
 * qualified arms that share (a, T) form a group of distinct unitigs (at most 4; in the bidirected form (a, T) and its mirror (T ^ 1, a ^ 1) are one group, and a
 * unitig is never compared with its own other image). With counts (d_counts: one uint32 per stored k-mer by ordinal, n_counts == the stored k-mers, as in
 * cblx_abundance_seqs) u ranks above v when kc[u] length[v] > kc[v] length[u] (mean coverage, compared exactly in 128-bit integers), then when it is longer,
 * then when u < v; d_counts == NULL with n_counts == 0 selects the length rule, which starts at the second clause. kind[u] = 2 (kept) when u is in a group of
 * two or more unitigs and ranks above all the others, 1 (popped) when another member ranks above it, 0 elsewhere: every such group has exactly one kept arm.
 * counts = { kept arms, popped arms, the k-mers of the popped arms }, always reported. kind may be NULL (counts only); cap_unitigs below the unitigs is
 * CBLX_ERANGE with the need in *n_unitigs and nothing written. The index is not modified. max_kmers == 0, NULL counts with n_counts != 0 and n_counts != the
 * stored k-mers are CBLX_EINVAL. */
int cblx_bubbles_mark(cblx_ctx* ctx, uint64_t max_kmers, const uint32_t* d_counts, uint64_t n_counts, uint8_t* kind, uint64_t cap_unitigs, uint64_t* n_unitigs,
                      uint64_t counts[3]);
int cblx_bubbles_mark_device(cblx_ctx* ctx, uint64_t max_kmers, const uint32_t* d_counts, uint64_t n_counts, uint8_t* d_kind, uint64_t cap_unitigs,
                             uint64_t* n_unitigs, uint64_t counts[3]);
/* Pops the bubbles: a round compacts, marks, takes the k-mers of ALL popped arms of that compaction in iteration order and removes their words as ONE
 * WordSet::remove_batch, as a round of cblx_clip_tips does. max_rounds = 0 repeats until a round pops nothing. stats (may be NULL): rounds = compactions run,
 * bubbles / popped / popped_kmers = what was removed, summed over the rounds, kmers_left, fixpoint = 1 when the last round popped nothing; an empty index gives
 * rounds = 1, fixpoint = 1. With counts the array is carried: behind every removing round d_counts[j], j < kmers_left, is the count the surviving k-mer of NEW
 * ordinal j had before, and the elements from kmers_left up to the n_counts given are 0; the caller goes on with n_counts = kmers_left. A call that removes
 * nothing does not write the array. flags must be 0. max_kmers == 0, flags != 0, NULL counts with n_counts != 0 and n_counts != the stored k-mers are
 * CBLX_EINVAL with nothing changed; the form's refusals come from the first compaction, before anything changes. */
typedef struct cblx_bubble_stats { uint64_t rounds, bubbles, popped, popped_kmers, kmers_left, fixpoint; } cblx_bubble_stats;
int cblx_pop_bubbles(cblx_ctx* ctx, uint64_t max_kmers, uint32_t* d_counts, uint64_t n_counts, uint32_t flags, uint32_t max_rounds, cblx_bubble_stats* stats);
/* CBL::buckets_nodes (src/cbl.rs:386-390): per non-empty prefix ascending, TrieVec::count_nodes (src/trievec/mod.rs:37-42) — a Vec's length, a Trie's
 * nodes (src/trie.rs:90-102: the root and one node per distinct proper byte prefix of its suffixes). Pairs with cblx_bucket_sizes. */
int cblx_bucket_nodes(cblx_ctx* ctx, uint64_t* nodes, uint64_t cap, uint64_t* n);
/* Bucket table only (CBL::buckets_sizes src/cbl.rs:370-373 and the statistics built on it): per non-empty prefix in
 * ascending order its value, the bucket's length and kind (0 = Vec, 1 = Trie). Any of the arrays may be NULL. */
int cblx_bucket_sizes(cblx_ctx* ctx, uint32_t* prefix, uint32_t* len, uint8_t* kind, uint64_t cap, uint64_t* n);

/* Full-size parity properties (no reference counterpart): an order-independent checksum of the set (sum over the
 * resident words of a 64-bit hash, mod 2^64), the same sum over a device array of words, and a structural check of the
 * resident buckets (Trie buckets strictly ascending, Vec buckets pairwise distinct, and with `strict` the insert-only
 * rule Vec <= 1024 < Trie of src/wordset/mod.rs:240-244). */
int cblx_checksum(cblx_ctx* ctx, uint64_t* sum);
int cblx_checksum_words_device(cblx_ctx* ctx, const uint64_t* d_lo, const void* d_hi, uint64_t n, uint64_t* sum);
int cblx_validate(cblx_ctx* ctx, int strict, uint64_t* violations);

/* Derived constants (src/cbl.rs:16-32,65-67), for shims and tests. */
typedef struct cblx_consts {
    uint32_t kmer_bits, pos_bits, word_bits, suffix_bits, bytes, chunk_size, threshold, hi_bytes;
} cblx_consts;
int cblx_get_consts(const cblx_ctx* ctx, cblx_consts* out);

/* Per-stage device time (ms, HIP events on the ctx's stream) accumulated since the last reset; needs
 * CBLX_FLAG_PROFILE. names[i] points to static storage. Returns the number of stages in *n (<= cap). */
int cblx_stage_times(cblx_ctx* ctx, const char** names, double* ms, uint64_t* launches, uint32_t cap, uint32_t* n);
int cblx_stage_times_reset(cblx_ctx* ctx);
/* Words the kernels of every stage were given since the last reset, in the order of cblx_stage_times, where the pipeline counts them
 * (today: radix_scatter — records through a partition pass, summed over the passes: how many a record takes depends on the route
 * (PREFIX_BITS > 24: the FINE-bins build sorts most of them in three passes, the rest in four); and, with CBLX_FLAG_PROFILE, `self |= other`,
 * whose bucket classes split the words between the stages — merge_gather: the words of the one-sided buckets it copies, bucket_medium:
 * the words of both-sided buckets with a Vec side, bucket_big: the OUTPUT words of the Trie |= Trie unions, bucket_huge: the rest).
 * 0 = not counted: the caller prices the stage on the whole batch. */
int cblx_stage_units(cblx_ctx* ctx, uint64_t* units, uint32_t cap, uint32_t* n);
/* k-mers (words) consumed by insert calls since creation — the numerator of the throughput metric. */
int cblx_kmers_inserted(cblx_ctx* ctx, uint64_t* out);
/* Batches this ctx built through the FINE-bins route (PREFIX_BITS > 24, empty index, a batch of CBLX_FINE_MIN k-mers or more — default
 * 2^22 —, CBLX_FINE_BINS != 0): the first partition pass runs on 253 intervals of the prefix space — aligned blocks of 2^16 prefixes
 * where the necklace prefixes are dense — so that most words need two more passes instead of three. Same index either way. */
int cblx_fine_builds(cblx_ctx* ctx, uint64_t* out);
/* Insert batches of this ctx whose chunk plan was ARITHMETIC: every sequence of the batch had the same length L with K <= L <= K + 2047 and
 * no byte outside ACGTacgt, so KRN-1 took chunk and tile positions from (offsets[0], L, K) and no chunk table was built. Any other batch
 * builds the tables; CBLX_UNIFORM_PLAN=0 (read per call) makes every batch do so. Same index either way. */
int cblx_uniform_plans(cblx_ctx* ctx, uint64_t* out);
/* Release cached device workspace (kept between flushes to avoid hipMalloc in the hot path). */
int cblx_trim(cblx_ctx* ctx);
/* Back to the state of CBL::new(): drops the resident index and anything enqueued, keeps the cached workspace. */
int cblx_clear(cblx_ctx* ctx);

#ifdef __cplusplus
}
#endif
#endif /* CBLX_H */
