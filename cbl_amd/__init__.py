"""cbl_amd — MI355X-native bulk k-mer insertion for CBL indexes (host-side mirror of the reference API).

`CBL` mirrors the method surface of the reference's `CBL<K, T, PREFIX_BITS>` for the build / insert / merge path
(/root/reference/src/cbl.rs:71-79 new/new_canonical, :127-160 save_to_file/load_from_file, :164-177
count/is_empty/is_canonical, :311-324 contains_seq, :328-339 insert_seq, :433-449 `|=`) on top of the C ABI in
include/cblx.h (libcblx.so, hand-written HIP for gfx950). There is NO CPU fallback: importing works anywhere, but
creating a `CBL` without the built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

_HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ["CBLX_LIB_PATH"]) if os.environ.get("CBLX_LIB_PATH") else _HERE / "libcblx.so"  # override: tuning variants (tools/)
_LIB = None

OK, EINVAL, ESHORT, EFORMAT, EDEVICE, ENOMEM, ERANGE = range(7)
FLAG_PROFILE = 1
RANK_ABSENT = (1 << 64) - 1  # what rank_np gives for a k-mer the set does not hold


class CblxError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(msg)
        self.code = code


class Params(C.Structure):
    _fields_ = [("k", C.c_uint32), ("prefix_bits", C.c_uint32), ("canonical", C.c_uint32), ("device", C.c_int32),
                ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class Consts(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("kmer_bits", "pos_bits", "word_bits", "suffix_bits", "bytes", "chunk_size",
                                          "threshold", "hi_bytes")]


class ShardInfo(C.Structure):
    _fields_ = [("header_entries", C.c_uint64), ("local_entries", C.c_uint64), ("begin_off", C.c_uint64), ("end_off", C.c_uint64),
                ("first_prefix", C.c_uint32), ("last_prefix", C.c_uint32), ("exact", C.c_uint32), ("canonical", C.c_uint32)]


class BucketView(C.Structure):
    _fields_ = [("n_buckets", C.c_uint64), ("n_words", C.c_uint64), ("d_prefix", C.c_void_p), ("d_count", C.c_void_p), ("d_kind", C.c_void_p),
                ("d_suffix", C.c_void_p)]


class ExchangeStats(C.Structure):
    _fields_ = [("sent_bytes", C.c_uint64), ("recv_bytes", C.c_uint64), ("messages", C.c_uint64)]


_ALL_REDUCE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.c_uint64)
_ALL_TO_ALL_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_uint64)
_EXCHANGE_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(C.c_uint64))


class Transport(C.Structure):
    _fields_ = [("user", C.c_void_p), ("all_reduce_sum_u64", _ALL_REDUCE_CB), ("all_to_all_u64", _ALL_TO_ALL_CB), ("exchange", _EXCHANGE_CB)]


class BatchView(C.Structure):
    _fields_ = [("n_buckets", C.c_uint64), ("n_words", C.c_uint64), ("d_prefix", C.c_void_p), ("d_count", C.c_void_p), ("d_suffix", C.c_void_p)]


class ClipStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rounds", "tips", "tip_kmers", "isolated", "isolated_kmers", "kmers_left", "fixpoint")]


CLIP_ISOLATED = 1  # CBLX_CLIP_ISOLATED of include/cblx.h
TIP_COUNTS = ("tips", "tip_kmers", "isolated", "isolated_kmers")


class ComponentStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("components", "removed_components", "removed_kmers", "kmers_left", "largest_kmers", "rounds")]


COMPONENTS_LARGEST = 1  # CBLX_COMPONENTS_LARGEST of include/cblx.h
COMPONENT_COUNTS = ("kmers", "unitigs", "links", "components", "largest_kmers", "rounds")


class AbundanceStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("kmers", "removed_kmers", "unitigs", "removed_unitigs", "kmers_left", "min_count")]


ABUNDANCE_UNITIGS = 1  # CBLX_ABUNDANCE_UNITIGS of include/cblx.h


class BubbleStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rounds", "bubbles", "popped", "popped_kmers", "kmers_left", "fixpoint")]


BUBBLE_COUNTS = ("bubbles", "popped", "popped_kmers")

BUCKET_CB = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64))

ABI_VERSION = 3  # include/cblx.h CBLX_ABI_VERSION

# name -> (restype, argtypes): every symbol include/cblx.h declares
SETOPS = {"or": 0, "and": 1, "sub": 2, "xor": 3}  # CBLX_SETOP_* of include/cblx.h

SIGNATURES = {
    "cblx_abi_version": (C.c_uint32, []),
    "cblx_last_global_error": (C.c_char_p, []),
    "cblx_create": (C.c_int, [C.POINTER(Params), C.POINTER(C.c_void_p)]),
    "cblx_destroy": (None, [C.c_void_p]),
    "cblx_last_error": (C.c_char_p, [C.c_void_p]),
    "cblx_insert_seq": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "cblx_insert_seqs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_insert_seqs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_insert_fastx_file": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]),
    "cblx_stage_fastx_blocks": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                          C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_stage_fastx_blocks_comm": (C.c_int, [C.c_void_p, C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_stage_release": (C.c_int, [C.c_void_p]),
    "cblx_flush": (C.c_int, [C.c_void_p]),
    "cblx_insert_words_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_seq_words_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
                                        C.POINTER(C.c_uint64)]),
    "cblx_partition_words_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "cblx_seq_words_partitioned_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                                    C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_sorted_batch_begin": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint32, C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "cblx_sorted_batch_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cblx_insert_sorted_batches_device": (C.c_int, [C.c_void_p, C.POINTER(BatchView), C.c_uint32]),
    "cblx_load_shard_from_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.POINTER(ShardInfo)]),
    "cblx_index_shard_cuts": (C.c_int, [C.POINTER(Params), C.c_char_p, C.c_uint32, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_int)]),
    "cblx_resident_split": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_resident_export": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "cblx_install_buckets_device": (C.c_int, [C.c_void_p, C.POINTER(BucketView), C.c_uint32]),
    "cblx_serialized_body_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_write_body_at": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "cblx_comm_unique_id": (C.c_int, [C.c_void_p]),
    "cblx_comm_init_rccl": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32]),
    "cblx_comm_init_transport": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(Transport), C.c_uint32, C.c_uint32, C.c_int32]),
    "cblx_comm_destroy": (None, [C.c_void_p]),
    "cblx_comm_last_error": (C.c_char_p, [C.c_void_p]),
    "cblx_comm_stats": (C.c_int, [C.c_void_p, C.POINTER(ExchangeStats), C.c_int]),
    "cblx_comm_set_protocol": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cblx_comm_init_sim": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32, C.c_int32, C.c_uint64, C.c_double]),
    "cblx_sim_store_free": (C.c_int, [C.c_uint64]),
    "cblx_comm_set_recv_groups": (C.c_int, [C.c_void_p, C.c_uint32]),
    "cblx_comm_groups_used": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "cblx_comm_groups_fine": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "cblx_comm_protocol_used": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint32)]),
    "cblx_fine_builds": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_uniform_plans": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_sharded_insert_seqs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.POINTER(C.c_int)]),
    "cblx_count": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_num_buckets": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_is_empty": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cblx_is_canonical": (C.c_int, [C.c_void_p, C.POINTER(C.c_int)]),
    "cblx_serialized_size": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_serialize": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_save_to_file": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cblx_load": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_load_from_file": (C.c_int, [C.c_void_p, C.c_char_p]),
    "cblx_merge_assign": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cblx_merge_from": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "cblx_set_op": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32]),
    "cblx_set_op_assign": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint32]),
    "cblx_set_op_many": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32]),
    "cblx_set_at_least": (C.c_int, [C.c_void_p, C.POINTER(C.c_void_p), C.c_uint32, C.c_uint32]),
    "cblx_occupancy_counts": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint64)]),
    "cblx_intersection_count": (C.c_int, [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_intersection_counts": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_uint64)]),
    "cblx_get_device": (C.c_int, [C.c_void_p, C.POINTER(C.c_int32)]),
    "cblx_stage_units": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64), C.c_uint32, C.POINTER(C.c_uint32)]),
    "cblx_export_buckets": (C.c_int, [C.c_void_p, BUCKET_CB, C.c_void_p]),
    "cblx_contains_seq": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    "cblx_query_fastx_file": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                            C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs_counts_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64),
                                                   C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs_flags_counts_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                                         C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_query_fastx_file_counts": (C.c_int, [C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                               C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs_counts_many": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_contains_seqs_counts_many_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_contains_all": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_int)]),
    "cblx_insert_kmers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_remove_words_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_remove_seq": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64]),
    "cblx_remove_seqs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_remove_seqs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    "cblx_remove_fastx_file": (C.c_int, [C.c_void_p, C.c_char_p, C.POINTER(C.c_uint64)]),
    "cblx_remove_kmers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_contains_kmers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_export_kmers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_export_kmers_range": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_export_kmers_range_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_neighbors_kmers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_neighbors_kmers_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_neighbors_range": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_neighbors_range_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_degree_table": (C.c_int, [C.c_void_p, C.c_void_p]),
    "cblx_rank_kmers": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_rank_kmers_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    "cblx_unitig_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_unitig_table_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64),
                                           C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_unitigs_text_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_unitigs_to_fd": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_unitigs_to_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_biunitig_table": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                      C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_biunitig_table_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                             C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_biunitigs_text_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_biunitigs_to_fd": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_biunitigs_to_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_gfa_links": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_gfa_links_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_gfa_text_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_gfa_to_fd": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_gfa_to_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_unitig_ends": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_unitig_ends_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_tips_mark": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_tips_mark_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_clip_tips": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(ClipStats)]),
    "cblx_components": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_components_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_components_filter": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(ComponentStats)]),
    "cblx_abundance_seqs": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_abundance_seqs_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_abundance_histogram": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_unitig_coverage": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_unitig_coverage_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_gfa_tagged_text_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint64)]),
    "cblx_gfa_tagged_to_fd": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_gfa_tagged_to_file": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_uint64)]),
    "cblx_abundance_filter": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(AbundanceStats)]),
    "cblx_bubbles_mark": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_bubbles_mark_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "cblx_pop_bubbles": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(BubbleStats)]),
    "cblx_list_range": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_list_range_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_list_to_fd": (C.c_int, [C.c_void_p, C.c_int, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_list_to_file": (C.c_int, [C.c_void_p, C.c_char_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_bucket_nodes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_bucket_sizes": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_checksum": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_checksum_words_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
    "cblx_validate": (C.c_int, [C.c_void_p, C.c_int, C.POINTER(C.c_uint64)]),
    "cblx_get_consts": (C.c_int, [C.c_void_p, C.POINTER(Consts)]),
    "cblx_stage_times": (C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.c_uint32,
                                   C.POINTER(C.c_uint32)]),
    "cblx_stage_times_reset": (C.c_int, [C.c_void_p]),
    "cblx_kmers_inserted": (C.c_int, [C.c_void_p, C.POINTER(C.c_uint64)]),
    "cblx_trim": (C.c_int, [C.c_void_p]),
    "cblx_clear": (C.c_int, [C.c_void_p]),
}


def lib() -> C.CDLL:
    """Load libcblx.so (built in-tree by __graft_entry__.build()). Fails loudly when it is missing."""
    global _LIB
    if _LIB is None:
        if not LIB_PATH.exists():
            raise ImportError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950). cbl_amd has no CPU fallback.")
        L = C.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            if os.environ.get("CBLX_LIB_PATH") and not hasattr(L, name):
                continue  # an older build loaded for comparison (tools/): its missing entry points are simply not bound
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if not os.environ.get("CBLX_LIB_PATH") and L.cblx_abi_version() != ABI_VERSION:
            raise ImportError(f"{LIB_PATH} reports ABI version {L.cblx_abi_version()}, this binding was written against {ABI_VERSION} "
                              "(include/cblx.h CBLX_ABI_VERSION): rebuild with __graft_entry__.build()")
        _LIB = L
    return _LIB


def _ptr(x):
    """Raw address of a torch tensor / numpy array / int."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    if hasattr(x, "ctypes"):
        return x.ctypes.data
    return int(x)


def index_shard_cuts(path, k: int, prefix_bits: int, world: int, bounds=None, sequential: bool = False):
    """Where `world` prefix ranges cut the entries of an index file (host only, no GPU): (byte offsets[world + 1],
    first prefixes[world + 1], ok)."""
    import numpy as np

    L = lib()
    p = Params(k, prefix_bits, 0, -1, 0, 0)
    b = np.ascontiguousarray(bounds, dtype=np.uint32) if bounds is not None else None
    offs = np.zeros(world + 1, dtype=np.uint64)
    first = np.zeros(world + 1, dtype=np.uint32)
    ok = C.c_int(0)
    rc = L.cblx_index_shard_cuts(C.byref(p), os.fsencode(path), world, b.ctypes.data if b is not None and len(b) else None, int(sequential),
                                 offs.ctypes.data, first.ctypes.data, C.byref(ok))
    if rc != OK:
        raise CblxError(rc, L.cblx_last_global_error().decode())
    return offs, first, bool(ok.value)


class Comm:
    """One rank's communicator of the multi-GPU build behind the C ABI (include/cblx.h: cblx_comm).

    `Comm.rccl(id, rank, world, device)`: RCCL over xGMI, `id` = Comm.unique_id() of rank 0 shipped to every rank by the host
    program. `Comm.over_group(dist, rank, world, device)`: host callbacks that move the bytes through a torch.distributed-like
    group, staged through the host (how several ranks share one GPU in the tests; not a production transport)."""

    def __init__(self, handle, keep=None):
        self._L, self._h, self._keep = lib(), handle, keep

    @staticmethod
    def unique_id() -> bytes:
        L = lib()
        buf = (C.c_uint8 * 128)()
        rc = L.cblx_comm_unique_id(buf)
        if rc != OK:
            raise CblxError(rc, L.cblx_last_global_error().decode())
        return bytes(buf)

    @classmethod
    def rccl(cls, uid: bytes, rank: int, world: int, device: int = -1) -> "Comm":
        L = lib()
        h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        rc = L.cblx_comm_init_rccl(C.byref(h), buf, rank, world, device)
        if rc != OK:
            raise CblxError(rc, L.cblx_last_global_error().decode())
        return cls(h)

    @classmethod
    def over_group(cls, dist, rank: int, world: int, device: int = -1) -> "Comm":
        import numpy as np
        import torch

        dev = torch.device("cuda", torch.cuda.current_device() if device < 0 else device)

        def view(ptr, n):
            from .sharded import _DeviceArray

            return torch.as_tensor(_DeviceArray(ptr, n, "|u1"), device=dev)

        def all_reduce(_u, vals, n):
            try:
                a = np.ctypeslib.as_array(vals, (n,))
                t = torch.from_numpy(a.astype(np.int64))
                dist.all_reduce(t)
                a[:] = t.numpy().astype(np.uint64)
                return 0
            except Exception:  # noqa: BLE001 - must not unwind into C
                return 1

        def all_to_all(_u, send, recv, per):
            try:
                s = torch.from_numpy(np.ctypeslib.as_array(send, (per * world,)).astype(np.int64))
                r = torch.empty_like(s)
                dist.all_to_all_single(r, s)
                np.ctypeslib.as_array(recv, (per * world,))[:] = r.numpy().astype(np.uint64)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        def exchange(_u, d_src, so, d_dst, ro):
            try:
                so = [int(so[i]) for i in range(world + 1)]
                ro = [int(ro[i]) for i in range(world + 1)]
                src = view(d_src, max(so[world], 1)) if so[world] else None
                dst = view(d_dst, max(ro[world], 1)) if ro[world] else None
                if so[rank + 1] > so[rank]:
                    dst[ro[rank]: ro[rank + 1]].copy_(src[so[rank]: so[rank + 1]])
                works, landing = [], []
                for k in range(1, world):
                    to, frm = (rank + k) % world, (rank - k) % world
                    if so[to + 1] > so[to]:
                        works.append(dist.isend(src[so[to]: so[to + 1]].cpu().contiguous(), to))
                    if ro[frm + 1] > ro[frm]:
                        h = torch.empty(ro[frm + 1] - ro[frm], dtype=torch.uint8)
                        works.append(dist.irecv(h, frm))
                        landing.append((frm, h))
                for w in works:
                    w.wait()
                for frm, h in landing:
                    dst[ro[frm]: ro[frm + 1]].copy_(h)
                torch.cuda.synchronize(dev)
                return 0
            except Exception:  # noqa: BLE001
                return 1

        cbs = (_ALL_REDUCE_CB(all_reduce), _ALL_TO_ALL_CB(all_to_all), _EXCHANGE_CB(exchange))
        t = Transport(None, *cbs)
        L = lib()
        h = C.c_void_p()
        rc = L.cblx_comm_init_transport(C.byref(h), C.byref(t), rank, world, device)
        if rc != OK:
            raise CblxError(rc, L.cblx_last_global_error().decode())
        return cls(h, keep=cbs)

    @classmethod
    def sim(cls, rank: int, world: int, store_id: int, link_gbps: float = 0.0, device: int = -1) -> "Comm":
        """Rehearsal of one rank of a `world`-GPU job on one GPU (include/cblx.h: cblx_comm_init_sim): ranks 1 .. world-1 record what they
        would send rank 0, rank 0 replays it paced at `link_gbps` GB/s per source rank."""
        L = lib()
        h = C.c_void_p()
        rc = L.cblx_comm_init_sim(C.byref(h), rank, world, device, store_id, link_gbps)
        if rc != OK:
            raise CblxError(rc, L.cblx_last_global_error().decode())
        return cls(h)

    @staticmethod
    def sim_store_free(store_id: int):
        lib().cblx_sim_store_free(store_id)

    PROTOCOLS = {"sorted": 0, "bins": 1, "auto": 2, "replicate": 3}  # CBLX_PROTO_SORTED / _BINS / _AUTO / _REPLICATE (include/cblx.h)

    @staticmethod
    def auto_protocol(world: int) -> str:
        """What "auto" resolves to (the library's rule, restated for callers that shape their slices by it): "replicate" on 2 - 3 ranks
        (one link per pair of GPUs bounds every protocol that ships words: the reads cross instead), "sorted" on 4, "bins" otherwise."""
        return "replicate" if 2 <= world <= 3 else ("sorted" if world == 4 else "bins")

    def protocol_used(self) -> str:
        """What the last sharded insert of this rank ran on ("auto" resolved; "bins" falls back to "sorted" at PREFIX_BITS <= 8)."""
        v = C.c_uint32(0)
        self._L.cblx_comm_protocol_used(self._h, C.byref(v))
        return {0: "sorted", 1: "bins", 3: "replicate"}[v.value]

    def set_protocol(self, name: str):
        """What crosses the links in sharded_insert_seqs_device: "bins" (exchange between the first and the second partition pass),
        "sorted" (full partition on the sender, packed suffixes on the wire) or "auto" (default: sorted on 2 - 4 ranks, bins
        otherwise). The same on every rank."""
        rc = self._L.cblx_comm_set_protocol(self._h, self.PROTOCOLS[name])
        if rc != OK:
            raise CblxError(rc, "cblx_comm_set_protocol")

    def set_recv_groups(self, groups: int):
        """Groups per rank of the "bins" receiver (0 = default: CBLX_RECV_GROUPS or 4; 1 = ungrouped): the data crosses the links
        group-major and the receiver works on group g while g + 1 .. are still on the wire. The same on every rank."""
        rc = self._L.cblx_comm_set_recv_groups(self._h, groups)
        if rc != OK:
            raise CblxError(rc, "cblx_comm_set_recv_groups")

    def groups_used(self) -> int:
        """Groups the last sharded insert of this rank worked through (0: the ungrouped path)."""
        g = C.c_uint32(0)
        self._L.cblx_comm_groups_used(self._h, C.byref(g))
        return g.value

    def groups_fine(self) -> int:
        """... of which sorted 16 prefix bits behind the senders' first pass (FINE bins, PREFIX_BITS > 24: two passes instead of three)."""
        g = C.c_uint32(0)
        self._L.cblx_comm_groups_fine(self._h, C.byref(g))
        return g.value

    def stats(self, reset: bool = False) -> dict:
        st = ExchangeStats()
        self._L.cblx_comm_stats(self._h, C.byref(st), int(reset))
        return {"sent_bytes": st.sent_bytes, "recv_bytes": st.recv_bytes, "messages": st.messages}

    def close(self):
        if getattr(self, "_h", None):
            self._L.cblx_comm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class CBL:
    """A set of k-mers backed by an index resident in the HBM of one MI355X.

    `CBL(k, prefix_bits=24)` = `CBL::<K, T, PREFIX_BITS>::new()`; `canonical=True` = `new_canonical()`.
    The reference picks T from K (build.rs:34-41); here the word width follows from k the same way.
    """

    def __init__(self, k: int, prefix_bits: int = 24, canonical: bool = False, device: int = -1, profile: bool = False):
        self._L = lib()
        self.k, self.prefix_bits = k, prefix_bits
        p = Params(k, prefix_bits, int(canonical), device, FLAG_PROFILE if profile else 0, 0)
        h = C.c_void_p()
        rc = self._L.cblx_create(C.byref(p), C.byref(h))
        if rc != OK:
            raise CblxError(rc, self._L.cblx_last_global_error().decode())
        self._h = h

    @classmethod
    def new_canonical(cls, k: int, prefix_bits: int = 24, **kw) -> "CBL":
        return cls(k, prefix_bits, canonical=True, **kw)

    def close(self):
        if getattr(self, "_h", None):
            self._L.cblx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc: int):
        if rc != OK:
            raise CblxError(rc, self._L.cblx_last_error(self._h).decode())

    # ---- src/cbl.rs:328-339 ---------------------------------------------------------------------------------
    def insert_seq(self, seq: bytes):
        """Adds all the k-mers of a sequence to the set (enqueued; materialised by the next observer)."""
        self._chk(self._L.cblx_insert_seq(self._h, seq, len(seq)))

    def insert_seqs(self, bases, offsets):
        """The caller loop of examples/cbl.rs:160-163 in one call. numpy uint8 / uint64 (host) arrays."""
        import numpy as np

        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(self._L.cblx_insert_seqs(self._h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1))

    def insert_fastx_file(self, path) -> int:
        """`for record in parse_fastx_file(path): insert_seq(record.seq())` (examples/cbl.rs:154-163); returns #records."""
        n = C.c_uint64(0)
        self._chk(self._L.cblx_insert_fastx_file(self._h, os.fsencode(path), C.byref(n)))
        return n.value

    # ---- src/cbl.rs:343-354: pending inserts are applied first, the removal runs before the call returns ------------
    def remove_seq(self, seq: bytes):
        """Removes all the k-mers of a sequence from the set. One device round trip per call: remove_seqs batches."""
        self._chk(self._L.cblx_remove_seq(self._h, seq, len(seq)))

    def remove_seqs(self, bases, offsets):
        """`for seq in seqs: remove_seq(seq)` in one call. numpy uint8 / uint64 (host) arrays."""
        import numpy as np

        bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        self._chk(self._L.cblx_remove_seqs(self._h, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1))

    def remove_seqs_device(self, d_bases, d_offsets, n: int):
        """Same with inputs resident in HBM (torch uint8 / int64 CUDA tensors or raw device addresses)."""
        self._chk(self._L.cblx_remove_seqs_device(self._h, _ptr(d_bases), _ptr(d_offsets), n))

    def remove_words_device(self, d_lo, d_hi, n: int):
        """WordSet::remove_batch (src/wordset/mod.rs:218-237) on device-resident words: one call = one batch."""
        self._chk(self._L.cblx_remove_words_device(self._h, _ptr(d_lo), _ptr(d_hi), n))

    def remove_fastx_file(self, path) -> int:
        """`for record in parse_fastx_file(path): remove_seq(record.seq())` (examples/cbl.rs:250-265); returns #records."""
        n = C.c_uint64(0)
        self._chk(self._L.cblx_remove_fastx_file(self._h, os.fsencode(path), C.byref(n)))
        return n.value

    def count_fastx_records(self, path) -> int:
        n = C.c_uint64(0)
        self._chk(self._L.cblx_stage_fastx_blocks(self._h, os.fsencode(path), 0, 0, 1, None, None, None, C.byref(n)))
        return n.value

    def stage_fastx_blocks(self, path, block: int, rank: int, world: int):
        """Parse a FASTA/FASTQ(.gz) file and stage this rank's block-cyclic share in HBM without inserting it. Returns
        (device address of the bases, device address of the n + 1 uint64 offsets, n staged, records in the file); the arrays
        stay valid until stage_release()."""
        pb, po = C.c_void_p(), C.c_void_p()
        n, tot = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_stage_fastx_blocks(self._h, os.fsencode(path), block, rank, world, C.byref(pb), C.byref(po), C.byref(n), C.byref(tot)))
        return pb.value or 0, po.value or 0, n.value, tot.value

    def stage_fastx_blocks_comm(self, comm, path, block: int = 0, slices: int = 4):
        """The same staging with the parse shared between the ranks of `comm` (every rank reads 1 / world of the file). Returns
        (device address of the bases, of the offsets, n staged, records in the file, block size used)."""
        pb, po = C.c_void_p(), C.c_void_p()
        n, tot, blk = C.c_uint64(0), C.c_uint64(0), C.c_uint64(block)
        self._chk(self._L.cblx_stage_fastx_blocks_comm(self._h, comm._h, os.fsencode(path), C.byref(blk), slices, C.byref(pb), C.byref(po), C.byref(n), C.byref(tot)))
        return pb.value or 0, po.value or 0, n.value, tot.value, blk.value

    def stage_release(self):
        self._chk(self._L.cblx_stage_release(self._h))

    def insert_seqs_device(self, d_bases, d_offsets, n: int):
        """Same with inputs resident in HBM (torch uint8 / int64 CUDA tensors or raw device addresses)."""
        self._chk(self._L.cblx_insert_seqs_device(self._h, _ptr(d_bases), _ptr(d_offsets), n))

    def insert_words_device(self, d_lo, d_hi, n: int):
        """WordSet::insert_batch (src/wordset/mod.rs:187-216) on device-resident words."""
        self._chk(self._L.cblx_insert_words_device(self._h, _ptr(d_lo), _ptr(d_hi), n))

    def seq_words_device(self, d_bases, d_offsets, n: int, d_lo, d_hi, cap: int) -> int:
        """CBL::get_seq_words over every chunk (src/cbl.rs:239-289) into device arrays; returns the word count."""
        nw = C.c_uint64(0)
        self._chk(self._L.cblx_seq_words_device(self._h, _ptr(d_bases), _ptr(d_offsets), n, _ptr(d_lo), _ptr(d_hi), cap, C.byref(nw)))
        return nw.value

    def partition_words_device(self, d_lo, d_hi, n: int, bounds, nd: int, d_out_lo, d_out_hi):
        """Stable partition of device words by destination prefix range; returns the nd run lengths."""
        import numpy as np

        b = np.ascontiguousarray(bounds, dtype=np.uint32)
        counts = np.zeros(nd, dtype=np.uint64)
        self._chk(self._L.cblx_partition_words_device(self._h, _ptr(d_lo), _ptr(d_hi), n, b.ctypes.data if len(b) else None, nd,
                                                      _ptr(d_out_lo), _ptr(d_out_hi), counts.ctypes.data))
        return [int(x) for x in counts]

    def seq_words_partitioned_device(self, d_bases, d_offsets, n: int, bounds, nd: int, d_out_lo, d_out_hi, cap: int):
        """get_seq_words of the sequences, grouped by destination prefix range; returns (n_words, run lengths)."""
        import numpy as np

        b = np.ascontiguousarray(bounds, dtype=np.uint32)
        counts = np.zeros(nd, dtype=np.uint64)
        nw = C.c_uint64(0)
        self._chk(self._L.cblx_seq_words_partitioned_device(self._h, _ptr(d_bases), _ptr(d_offsets), n, b.ctypes.data if len(b) else None, nd,
                                                            _ptr(d_out_lo), _ptr(d_out_hi), cap, counts.ctypes.data, C.byref(nw)))
        return nw.value, [int(x) for x in counts]

    # ---- multi-GPU build, sorted-batch protocol (include/cblx.h) -----------------------------------------------------
    def sorted_batch_begin(self, d_bases, d_offsets, n: int, bounds, nd: int):
        """KRN-1 + full partition; returns (bucket_split, word_split): nd + 1 host entries each."""
        import numpy as np

        b = np.ascontiguousarray(bounds, dtype=np.uint32)
        bs = (C.c_uint64 * (nd + 1))()
        ws = (C.c_uint64 * (nd + 1))()
        self._chk(self._L.cblx_sorted_batch_begin(self._h, _ptr(d_bases), _ptr(d_offsets), n, b.ctypes.data_as(C.POINTER(C.c_uint32)), nd, bs, ws))
        return list(bs), list(ws)

    def sorted_batch_export(self, d_prefix, d_count, d_suffix):
        self._chk(self._L.cblx_sorted_batch_export(self._h, _ptr(d_prefix), _ptr(d_count), _ptr(d_suffix)))

    def insert_sorted_batches_device(self, batches):
        """batches: [(n_buckets, n_words, d_prefix, d_count, d_suffix)] in stream order."""
        arr = (BatchView * max(len(batches), 1))()
        for i, (nb, nw, p, c, s) in enumerate(batches):
            arr[i] = BatchView(nb, nw, _ptr(p) if nb else None, _ptr(c) if nb else None, _ptr(s) if nw else None)
        self._chk(self._L.cblx_insert_sorted_batches_device(self._h, arr, len(batches)))

    # ---- prefix-range sharded indexes (include/cblx.h): one rank's share -------------------------------------------------
    def load_shard_from_file(self, path, rank: int, world: int, bounds=None, sequential: bool = False):
        """This rank's prefix range of an index file. Returns (info dict, bounds as a numpy uint32 array of world-1 values).
        The caller checks info["exact"] and the entry counts over all ranks (cbl_amd.sharded.ShardedIndex does)."""
        import numpy as np

        b = np.ascontiguousarray(bounds, dtype=np.uint32) if bounds is not None else None
        out = np.zeros(max(world - 1, 1), dtype=np.uint32)
        info = ShardInfo()
        self._chk(self._L.cblx_load_shard_from_file(self._h, os.fsencode(path), rank, world, b.ctypes.data if b is not None and len(b) else None,
                                                    int(sequential), out.ctypes.data, C.byref(info)))
        return {n: getattr(info, n) for n, _ in ShardInfo._fields_}, out[: world - 1]

    def resident_split(self, bounds, nd: int):
        """(bucket_split, word_split), nd + 1 entries each: where the bounds cut the resident index."""
        import numpy as np

        b = np.ascontiguousarray(bounds, dtype=np.uint32)
        bs = (C.c_uint64 * (nd + 1))()
        ws = (C.c_uint64 * (nd + 1))()
        self._chk(self._L.cblx_resident_split(self._h, b.ctypes.data if len(b) else None, nd, bs, ws))
        return list(bs), list(ws)

    def resident_export(self, d_prefix, d_count, d_kind, d_suffix):
        self._chk(self._L.cblx_resident_export(self._h, _ptr(d_prefix), _ptr(d_count), _ptr(d_kind), _ptr(d_suffix)))

    def install_buckets_device(self, parts):
        """parts: [(n_buckets, n_words, d_prefix, d_count, d_kind, d_suffix)], ascending prefixes over the concatenation."""
        arr = (BucketView * max(len(parts), 1))()
        for i, (nb, nw, p, c, k, s) in enumerate(parts):
            arr[i] = BucketView(nb, nw, _ptr(p) if nb else None, _ptr(c) if nb else None, _ptr(k) if nb else None, _ptr(s) if nw else None)
        self._chk(self._L.cblx_install_buckets_device(self._h, arr, len(parts)))

    def serialized_body_size(self):
        """(entries, bytes) of the serialized index without its header."""
        ne, nb = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_serialized_body_size(self._h, C.byref(ne), C.byref(nb)))
        return ne.value, nb.value

    def write_body_at(self, path, file_off: int):
        self._chk(self._L.cblx_write_body_at(self._h, os.fsencode(path), file_off))

    def sharded_insert_seqs_device(self, comm: "Comm", d_bases, d_offsets, n: int, slice_cuts, bounds, bounds_valid: bool):
        """The multi-GPU build step behind the ABI (cblx_sharded_insert_seqs_device): every rank calls it with its shard.
        `bounds`: numpy uint32 array of world - 1 entries, updated in place when bounds_valid is False. Returns True
        (the bounds are valid from now on)."""
        import numpy as np

        cuts = np.ascontiguousarray(slice_cuts, dtype=np.uint64)
        assert bounds.dtype == np.uint32 and bounds.flags["C_CONTIGUOUS"]
        bv = C.c_int(int(bounds_valid))
        self._chk(self._L.cblx_sharded_insert_seqs_device(self._h, comm._h, _ptr(d_bases), _ptr(d_offsets), n, cuts.ctypes.data, len(cuts) - 1,
                                                          bounds.ctypes.data if len(bounds) else None, C.byref(bv)))
        return bool(bv.value)

    def flush(self):
        self._chk(self._L.cblx_flush(self._h))

    # ---- src/cbl.rs:164-177 ---------------------------------------------------------------------------------
    def count(self) -> int:
        v = C.c_uint64(0)
        self._chk(self._L.cblx_count(self._h, C.byref(v)))
        return v.value

    def num_buckets(self) -> int:
        v = C.c_uint64(0)
        self._chk(self._L.cblx_num_buckets(self._h, C.byref(v)))
        return v.value

    def is_empty(self) -> bool:
        v = C.c_int(0)
        self._chk(self._L.cblx_is_empty(self._h, C.byref(v)))
        return bool(v.value)

    def is_canonical(self) -> bool:
        v = C.c_int(0)
        self._chk(self._L.cblx_is_canonical(self._h, C.byref(v)))
        return bool(v.value)

    def contains_seq(self, seq: bytes):
        """For each k-mer of a sequence, True if it is in the set (src/cbl.rs:311-324)."""
        return self.contains_seq_np(seq).tolist()

    def contains_seq_np(self, seq: bytes):
        """contains_seq as a numpy bool array (no per-element Python objects)."""
        import numpy as np

        cap = max(len(seq), 1)
        out = np.empty(cap, dtype=np.uint8)
        n = C.c_uint64(0)
        self._chk(self._L.cblx_contains_seq(self._h, seq, len(seq), out.ctypes.data_as(C.POINTER(C.c_uint8)), cap, C.byref(n)))
        return out[: n.value].astype(bool)

    def contains_seqs(self, bases, offsets, flags: bool = True):
        """contains_seq for a batch (bases: uint8 array, offsets: uint64 array of n+1 entries). Returns
        (flags as a numpy bool array or None, k-mers queried, positives)."""
        import numpy as np

        n = len(offsets) - 1
        cap = max(int(offsets[-1] - offsets[0]), 1) if n > 0 else 1
        out = np.empty(cap, dtype=np.uint8) if flags else None
        tot, pos = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_contains_seqs(self._h, _ptr(bases), _ptr(offsets), max(n, 0), _ptr(out) if flags else None, cap, C.byref(tot), C.byref(pos)))
        return (out[: tot.value].astype(bool) if flags else None), tot.value, pos.value

    def contains_seqs_device(self, d_bases, d_offsets, n: int, d_out=None, cap: int = 0):
        """Device-resident batch; returns (k-mers queried, positives). d_out (uint8 tensor) receives the flags when given."""
        tot, pos = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_contains_seqs_device(self._h, _ptr(d_bases), _ptr(d_offsets), n, _ptr(d_out), cap, C.byref(tot), C.byref(pos)))
        return tot.value, pos.value

    def query_fastx_file(self, path):
        """`cbl query`: (records, k-mers queried, positives) for a FASTA/FASTQ(.gz) file; the index is not modified."""
        import os

        nrec, tot, pos = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_query_fastx_file(self._h, os.fsencode(path), C.byref(nrec), C.byref(tot), C.byref(pos)))
        return nrec.value, tot.value, pos.value

    # ---- per-sequence tallies: (k-mers queried, k-mers found) of every sequence; the flags never leave the device ------------------
    def contains_seqs_counts(self, bases, offsets):
        """contains_seq for a batch, reduced per sequence on the device: (total uint32[n], positive uint32[n]) — the k-mers of every
        sequence queried and found (include/cblx.h cblx_contains_seqs_counts)."""
        import numpy as np

        n = max(len(offsets) - 1, 0)
        total, positive = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint32)
        tot, pos = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_contains_seqs_counts(self._h, _ptr(bases), _ptr(offsets), n, _ptr(total), _ptr(positive), C.byref(tot), C.byref(pos)))
        return total, positive

    def contains_seqs_counts_device(self, d_bases, d_offsets, n: int, d_total=None, d_positive=None, d_flags=None):
        """Device-resident batch; returns the two tensors (n uint32 each, int32 storage: torch has no arithmetic on uint32), allocated on
        d_bases' device when not given. d_flags (uint8 tensor) also receives the flags, as contains_seqs_device's d_out does."""
        import torch

        if d_total is None:
            d_total = torch.empty(n, dtype=torch.int32, device=d_bases.device)
        if d_positive is None:
            d_positive = torch.empty(n, dtype=torch.int32, device=d_bases.device)
        tot, pos = C.c_uint64(0), C.c_uint64(0)
        if d_flags is None:
            self._chk(self._L.cblx_contains_seqs_counts_device(self._h, _ptr(d_bases), _ptr(d_offsets), n, _ptr(d_total), _ptr(d_positive), C.byref(tot), C.byref(pos)))
        else:
            self._chk(self._L.cblx_contains_seqs_flags_counts_device(self._h, _ptr(d_bases), _ptr(d_offsets), n, _ptr(d_flags), d_flags.numel(), _ptr(d_total),
                                                                     _ptr(d_positive), C.byref(tot), C.byref(pos)))
        return d_total, d_positive

    def query_fastx_file_counts(self, path):
        """`cbl query` per record: (total uint32[records], positive uint32[records]) of a FASTA/FASTQ(.gz) file, record i = the i-th
        record of the file. The arrays are sized with count_fastx_records; the index is not modified."""
        import numpy as np

        cap = self.count_fastx_records(path)
        total, positive = np.empty(cap, dtype=np.uint32), np.empty(cap, dtype=np.uint32)
        nrec, tot, pos = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_query_fastx_file_counts(self._h, os.fsencode(path), _ptr(total), _ptr(positive), cap, C.byref(nrec), C.byref(tot), C.byref(pos)))
        return total[: nrec.value], positive[: nrec.value]

    @staticmethod
    def matching(total, positive, min_fraction: float = 0.5, min_hits: int = 0):
        """The screening rule on per-sequence counts (host, numpy): positive >= max(min_hits, ceil(min_fraction * total)) and
        total > 0 — a sequence without a k-mer never matches."""
        import numpy as np

        total, positive = np.asarray(total, dtype=np.int64), np.asarray(positive, dtype=np.int64)
        need = np.maximum(np.ceil(min_fraction * total).astype(np.int64), int(min_hits))
        return (total > 0) & (positive >= need)

    def matching_seqs(self, bases, offsets, min_fraction: float = 0.5, min_hits: int = 0):
        """Which sequences of the batch match the index: the boolean mask `matching` of contains_seqs_counts."""
        return self.matching(*self.contains_seqs_counts(bases, offsets), min_fraction=min_fraction, min_hits=min_hits)

    # ---- a batch against a panel of up to 64 indexes in one pass (ours) ----------------------------------------
    @staticmethod
    def contains_seqs_counts_many(cbls, bases, offsets, masks: bool = False):
        """contains_seqs_counts against every index of `cbls` at once: (total uint32[nseq], positive uint32[n, nseq]) — row j is what
        cbls[j].contains_seqs_counts(bases, offsets) returns — and with `masks` also mask uint64[nk]: one word per k-mer, in the order of
        contains_seqs' flags, bit j = cbls[j] holds it. The k-mers are encoded and partitioned once for the whole panel; no index is modified or
        sorted, an empty one counts and holds nothing (include/cblx.h cblx_contains_seqs_counts_many)."""
        import numpy as np

        cbls = CBL._many_operands(cbls, "contains_seqs_counts_many")
        n, nseq = len(cbls), max(len(offsets) - 1, 0)
        total, positive = np.empty(nseq, dtype=np.uint32), np.empty((n, nseq), dtype=np.uint32)
        mask, cap = None, 0
        if masks:
            lens = np.diff(np.asarray(offsets).astype(np.int64)) if nseq else np.zeros(0, dtype=np.int64)
            cap = int(np.maximum(lens - cbls[0].k + 1, 0).sum())  # no sequence holds more k-mers
            mask = np.empty(max(cap, 1), dtype=np.uint64)
        srcs = (C.c_void_p * n)(*[c._h for c in cbls])
        tot = C.c_uint64(0)
        cbls[0]._chk(cbls[0]._L.cblx_contains_seqs_counts_many(srcs, n, _ptr(bases), _ptr(offsets), nseq, _ptr(total), _ptr(positive), _ptr(mask), cap, C.byref(tot), None))
        return (total, positive, mask[: tot.value]) if masks else (total, positive)

    @staticmethod
    def contains_seqs_counts_many_device(cbls, d_bases, d_offsets, n: int, d_total=None, d_positive=None, d_mask=None):
        """Device-resident batch of `n` sequences; returns (d_total int32[n], d_positive int32[len(cbls), n]) — uint32 values in int32 storage,
        as contains_seqs_counts_device — allocated on d_bases' device when not given. d_mask (int64 tensor of at least as many words as the
        batch has k-mers) also receives the masks; it is then returned as a third value."""
        import torch

        cbls = CBL._many_operands(cbls, "contains_seqs_counts_many_device")
        if d_total is None:
            d_total = torch.empty(n, dtype=torch.int32, device=d_bases.device)
        if d_positive is None:
            d_positive = torch.empty((len(cbls), n), dtype=torch.int32, device=d_bases.device)
        srcs = (C.c_void_p * len(cbls))(*[c._h for c in cbls])
        tot = C.c_uint64(0)
        cbls[0]._chk(cbls[0]._L.cblx_contains_seqs_counts_many_device(srcs, len(cbls), _ptr(d_bases), _ptr(d_offsets), n, _ptr(d_total), _ptr(d_positive), _ptr(d_mask),
                                                                      d_mask.numel() if d_mask is not None else 0, C.byref(tot), None))
        return (d_total, d_positive) if d_mask is None else (d_total, d_positive, d_mask)

    @staticmethod
    def classify(total, positive, min_fraction: float = 0.5, min_hits: int = 0):
        """One index per sequence from the table of contains_seqs_counts_many (host, numpy): int64[nseq], the index with the most hits among
        those whose row passes `matching`'s rule — positive >= max(min_hits, ceil(min_fraction * total)) and total > 0 — ties to the lowest
        index, -1 where no index passes."""
        import numpy as np

        total = np.asarray(total, dtype=np.int64)
        positive = np.atleast_2d(np.asarray(positive, dtype=np.int64))
        if positive.shape[1] != len(total):
            raise ValueError("classify: positive is [n, nseq] for total[nseq]")
        if positive.shape[0] == 0 or len(total) == 0:
            return np.full(len(total), -1, dtype=np.int64)
        ok = np.stack([CBL.matching(total, row, min_fraction=min_fraction, min_hits=min_hits) for row in positive])
        score = np.where(ok, positive, -1)
        best = np.argmax(score, axis=0).astype(np.int64)  # (argmax keeps the first of equal maxima: the lowest index)
        return np.where(ok.any(axis=0), best, -1).astype(np.int64)

    def contains_all(self, seq: bytes) -> bool:
        """True if the set contains all the k-mers of a sequence (src/cbl.rs:293-307)."""
        v = C.c_int(0)
        self._chk(self._L.cblx_contains_all(self._h, seq, len(seq), C.byref(v)))
        return bool(v.value)

    # ---- packed k-mers (IntKmer::to_int(): 2K bits, first base most significant) — src/cbl.rs:219-228,358-361 ------------
    @staticmethod
    def _split_kmers(kmers):
        import numpy as np

        ks = [int(x) for x in kmers]
        lo = np.array([x & 0xFFFFFFFFFFFFFFFF for x in ks], dtype=np.uint64)
        hi = np.array([x >> 64 for x in ks], dtype=np.uint64)
        return lo, hi

    def insert_kmers(self, kmers):
        """n successive `insert` calls; returns their results as a numpy bool array (True = the k-mer was absent)."""
        import numpy as np

        lo, hi = self._split_kmers(kmers)
        out = np.zeros(max(len(lo), 1), dtype=np.uint8)
        self._chk(self._L.cblx_insert_kmers(self._h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)))
        return out[: len(lo)].astype(bool)

    def contains_kmers(self, kmers):
        import numpy as np

        lo, hi = self._split_kmers(kmers)
        out = np.zeros(max(len(lo), 1), dtype=np.uint8)
        self._chk(self._L.cblx_contains_kmers(self._h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)))
        return out[: len(lo)].astype(bool)

    def remove_kmers(self, kmers):
        """n successive `remove` calls; returns their results as a numpy bool array (True = the k-mer was present)."""
        import numpy as np

        lo, hi = self._split_kmers(kmers)
        out = np.zeros(max(len(lo), 1), dtype=np.uint8)
        self._chk(self._L.cblx_remove_kmers(self._h, _ptr(lo), _ptr(hi) if (self.k > 31 or hi.any()) else None, len(lo), _ptr(out)))
        return out[: len(lo)].astype(bool)

    def remove(self, kmer: int) -> bool:
        """Removes a packed k-mer; True if it was present (src/cbl.rs:233-235)."""
        return bool(self.remove_kmers([kmer])[0])

    def insert(self, kmer: int) -> bool:
        """Adds a packed k-mer; True if it was absent (src/cbl.rs:226-228)."""
        return bool(self.insert_kmers([kmer])[0])

    def contains(self, kmer: int) -> bool:
        """True if the set contains the packed k-mer (src/cbl.rs:219-221)."""
        return bool(self.contains_kmers([kmer])[0])

    def kmers_np(self, first: int = 0, n=None):
        """The k-mers of the set in the reference's iteration order as (lo, hi) uint64 arrays (hi is None for K <= 31): all of them, or
        with `first` / `n` elements [first, first + n) of that order (clamped at the end; `first` past the end raises). A ranged call
        takes device and host memory for its n elements only."""
        import numpy as np

        if first == 0 and n is None:
            n = self.count()
            lo = np.empty(max(n, 1), dtype=np.uint64)
            hi = np.empty(max(n, 1), dtype=np.uint64) if self.k > 31 else None
            got = C.c_uint64(0)
            self._chk(self._L.cblx_export_kmers(self._h, _ptr(lo), _ptr(hi) if hi is not None else None, n, C.byref(got)))
            return lo[: got.value], (hi[: got.value] if hi is not None else None)
        total = self.count()
        n = max(min(total - first, total if n is None else n), 0)  # (first > count: the library refuses it)
        lo = np.empty(max(n, 1), dtype=np.uint64)
        hi = np.empty(max(n, 1), dtype=np.uint64) if self.k > 31 else None
        got = self.export_kmers_range(first, n, lo, hi)
        return lo[:got], (hi[:got] if hi is not None else None)

    def export_kmers_range(self, first: int, n: int, lo, hi=None) -> int:
        """Elements [first, first + n) of the iteration order into the caller's uint64 numpy arrays (`hi` may be None for K <= 31);
        returns how many were written: min(n, count - first)."""
        got = C.c_uint64(0)
        self._chk(self._L.cblx_export_kmers_range(self._h, first, n, _ptr(lo), _ptr(hi), C.byref(got)))
        return got.value

    def export_kmers_range_device(self, first: int, n: int, d_lo, d_hi=None) -> int:
        """The same into device arrays (torch int64 / uint64 CUDA tensors or raw device addresses)."""
        got = C.c_uint64(0)
        self._chk(self._L.cblx_export_kmers_range_device(self._h, first, n, _ptr(d_lo), _ptr(d_hi), C.byref(got)))
        return got.value

    # ---- the index as the node set of a de Bruijn graph (Kmer::successors / predecessors, src/kmer.rs:82-90) ---------
    @staticmethod
    def neighbor_kmers(kmer: int, k: int):
        """The eight packed neighbours of a packed k-mer in the bit order of a neighbour mask (host only): [0 .. 3] the successors
        ((x << 2) | c) & MASK, [4 .. 7] the predecessors (x >> 2) | (c << 2 (K - 1)), c = 0 .. 3 (A C T G)."""
        x = int(kmer)
        if k < 1 or x < 0 or x >> (2 * k):
            raise ValueError("neighbor_kmers: a packed k-mer has 2K bits")
        mask = (1 << (2 * k)) - 1
        return [((x << 2) | c) & mask for c in range(4)] + [(x >> 2) | (c << (2 * (k - 1))) for c in range(4)]

    def neighbors_np(self, kmers):
        """The neighbour mask of every packed k-mer, a uint8 array: bit c = the set holds the successor by base c, bit 4 + c = the
        predecessor by base c (a canonical index canonicalises the neighbour; the k-mer itself is taken as given and need not be in
        the set). `kmers`: an iterable of Python ints, or the (lo, hi) uint64 arrays kmers_np returns (hi None for K <= 31)."""
        import numpy as np

        if isinstance(kmers, tuple) and len(kmers) == 2 and hasattr(kmers[0], "dtype"):
            lo = np.ascontiguousarray(kmers[0], dtype=np.uint64)
            hi = None if kmers[1] is None else np.ascontiguousarray(kmers[1], dtype=np.uint64)
            if hi is not None and len(hi) != len(lo):
                raise ValueError("neighbors_np: lo and hi differ in length")
        else:
            lo, hi = self._split_kmers(kmers)
        out = np.zeros(max(len(lo), 1), dtype=np.uint8)
        self._chk(self._L.cblx_neighbors_kmers(self._h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)))
        return out[: len(lo)]

    def neighbors_device(self, d_lo, d_hi, n: int, d_masks=None):
        """The same on device arrays (torch int64 / uint64 CUDA tensors or raw device addresses; d_hi may be None for K <= 31);
        returns d_masks, a torch uint8 CUDA tensor of n bytes allocated here when it is not given."""
        if d_masks is None:
            import torch

            d_masks = torch.empty(max(n, 1), dtype=torch.uint8, device=torch.device("cuda", self.device()))[:n]
        self._chk(self._L.cblx_neighbors_kmers_device(self._h, _ptr(d_lo), _ptr(d_hi), n, _ptr(d_masks)))
        return d_masks

    def neighbors_range_np(self, first: int = 0, n=None):
        """The neighbour masks of elements [first, first + n) of the iteration order, a uint8 array: entry i belongs to k-mer i of
        kmers_np(first, n). The k-mers never leave the device."""
        import numpy as np

        total = self.count()
        n = max(min(total - first, total if n is None else n), 0)  # (first > count: the library refuses it)
        out = np.zeros(max(n, 1), dtype=np.uint8)
        got = C.c_uint64(0)
        self._chk(self._L.cblx_neighbors_range(self._h, first, n, _ptr(out), C.byref(got)))
        return out[: got.value]

    def neighbors_range_device(self, first: int, n: int, d_masks) -> int:
        """The same into device memory (a torch uint8 CUDA tensor or raw device address of n bytes); returns the masks written."""
        got = C.c_uint64(0)
        self._chk(self._L.cblx_neighbors_range_device(self._h, first, n, _ptr(d_masks), C.byref(got)))
        return got.value

    def degree_table(self):
        """table[out, in] = the k-mers of the set with `out` successors and `in` predecessors in the set: a (5, 5) uint64 array that sums to
        count(). Computed on the device over the whole index; 200 bytes come back."""
        import numpy as np

        table = np.zeros(25, dtype=np.uint64)
        self._chk(self._L.cblx_degree_table(self._h, _ptr(table)))
        return table.reshape(5, 5)

    @staticmethod
    def degree_summary(table) -> dict:
        """What a degree table says about the graph (host only): nodes; out_edges = sum of out * T and in_edges = sum of in * T; isolated
        (out = in = 0), sources (in = 0 < out), sinks (out = 0 < in), simple (out = in = 1) and branching (out > 1 or in > 1) nodes. Every
        node is in at least one class, and in two only where a source or a sink has degree 2 or more: it is branching as well."""
        import numpy as np

        t = np.asarray(table, dtype=np.uint64).reshape(5, 5)
        T = [[int(v) for v in row] for row in t.tolist()]
        cells = [(o, i, T[o][i]) for o in range(5) for i in range(5)]
        return {
            "nodes": sum(v for _, _, v in cells),
            "out_edges": sum(o * v for o, _, v in cells),
            "in_edges": sum(i * v for _, i, v in cells),
            "isolated": T[0][0],
            "sources": sum(v for o, i, v in cells if i == 0 and o > 0),
            "sinks": sum(v for o, i, v in cells if o == 0 and i > 0),
            "simple": T[1][1],
            "branching": sum(v for o, i, v in cells if o > 1 or i > 1),
        }

    def _held_neighbors(self, kmer: int, shift: int):
        mask = int(self.neighbors_np([kmer])[0]) >> shift
        nb = self.neighbor_kmers(kmer, self.k)[shift: shift + 4]
        return [nb[c] for c in range(4) if (mask >> c) & 1]

    def successors(self, kmer: int):
        """The successors of a packed k-mer that the set holds, as packed k-mers in ascending base code (src/kmer.rs:82-85)."""
        return self._held_neighbors(kmer, 0)

    def predecessors(self, kmer: int):
        """The predecessors of a packed k-mer that the set holds, as packed k-mers in ascending base code (src/kmer.rs:87-90)."""
        return self._held_neighbors(kmer, 4)

    def iter(self, chunk: int = 1 << 22):
        """Iterator over the packed k-mers of the set (src/cbl.rs:358-361), pulled from the device `chunk` k-mers at a time: the first
        one is there after one chunk, and no more than a chunk is held at once. The index must not change while the generator is
        alive (the reference's `iter` borrows the set: the borrow checker enforces there what is a rule here) — an insert, a removal
        or a set operation in between makes the rest of the sequence meaningless."""
        if chunk < 1:
            raise ValueError("iter: chunk must be at least 1")
        import numpy as np

        first, total = 0, self.count()
        cap = max(min(chunk, total), 1)
        lo = np.empty(cap, dtype=np.uint64)
        hi = np.empty(cap, dtype=np.uint64) if self.k > 31 else None
        while first < total:
            got = self.export_kmers_range(first, cap, lo, hi)
            if got == 0:
                return
            if hi is None:
                yield from lo[:got].tolist()
            else:
                for l, h in zip(lo[:got].tolist(), hi[:got].tolist()):
                    yield (h << 64) | l
            first += got

    def __iter__(self):
        return self.iter()

    # ---- `cbl list` (examples/cbl.rs:177-201): one line per k-mer, K bytes of IntKmer::to_nucs + '\n' -------------------------
    def list_range(self, first: int, n: int, buf, cap=None) -> int:
        """The lines of elements [first, first + n) of the iteration order into the caller's uint8 numpy array; returns the bytes
        written. A buffer too small raises CblxError(ERANGE) and is left untouched."""
        got = C.c_uint64(0)
        self._chk(self._L.cblx_list_range(self._h, first, n, _ptr(buf), buf.size if cap is None else cap, C.byref(got)))
        return got.value

    def list_range_device(self, first: int, n: int, d_buf, cap: int) -> int:
        """The same into device memory (a 16-byte aligned torch uint8 CUDA tensor or raw device address of `cap` bytes)."""
        got = C.c_uint64(0)
        self._chk(self._L.cblx_list_range_device(self._h, first, n, _ptr(d_buf), cap, C.byref(got)))
        return got.value

    def list_np(self, first: int = 0, n=None):
        """Elements [first, first + n) of the iteration order as text: a uint8 array of shape (written, K + 1), row = the k-mer's
        bases (b"ACTG"[code], first base first) and '\\n'."""
        import numpy as np

        total = self.count()
        n = max(min(total - first, total if n is None else n), 0)
        buf = np.empty(max(n, 1) * (self.k + 1), dtype=np.uint8)
        got = self.list_range(first, n, buf)
        return buf[:got].reshape(-1, self.k + 1)

    def list_to_file(self, path, chunk: int = 0) -> int:
        """Writes every k-mer as a line to `path` (created / truncated), streamed from the device `chunk` k-mers at a time (0 = the
        library's default); returns the number of k-mers."""
        n = C.c_uint64(0)
        self._chk(self._L.cblx_list_to_file(self._h, os.fsencode(path), chunk, C.byref(n)))
        return n.value

    def list_to_fd(self, fd: int, chunk: int = 0) -> int:
        """The same to an open file descriptor (flush any Python-level buffer over it first)."""
        n = C.c_uint64(0)
        self._chk(self._L.cblx_list_to_fd(self._h, fd, chunk, C.byref(n)))
        return n.value

    # ---- unitigs: the non-branching paths of the de Bruijn graph -----------------------------------------
    def rank_np(self, kmers):
        """The ordinal of every packed k-mer in the iteration order — the index at which kmers_np / iter give it — as a uint64 array;
        RANK_ABSENT (2^64 - 1) where the set does not hold the k-mer. A canonical index canonicalises the query, as contains does.
        `kmers`: an iterable of Python ints, or the (lo, hi) uint64 arrays kmers_np returns (hi None for K <= 31)."""
        import numpy as np

        if isinstance(kmers, tuple) and len(kmers) == 2 and hasattr(kmers[0], "dtype"):
            lo = np.ascontiguousarray(kmers[0], dtype=np.uint64)
            hi = None if kmers[1] is None else np.ascontiguousarray(kmers[1], dtype=np.uint64)
            if hi is not None and len(hi) != len(lo):
                raise ValueError("rank_np: lo and hi differ in length")
        else:
            lo, hi = self._split_kmers(kmers)
        out = np.zeros(max(len(lo), 1), dtype=np.uint64)
        self._chk(self._L.cblx_rank_kmers(self._h, _ptr(lo), _ptr(hi), len(lo), _ptr(out)))
        return out[: len(lo)]

    def rank_device(self, d_lo, d_hi, n: int, d_rank=None):
        """The same on device arrays (torch int64 / uint64 CUDA tensors or raw device addresses; d_hi may be None for K <= 31); returns
        d_rank, a torch int64 CUDA tensor of n elements allocated here when it is not given (an absent k-mer reads -1 in it)."""
        if d_rank is None:
            import torch

            d_rank = torch.empty(max(n, 1), dtype=torch.int64, device=torch.device("cuda", self.device()))[:n]
        self._chk(self._L.cblx_rank_kmers_device(self._h, _ptr(d_lo), _ptr(d_hi), n, _ptr(d_rank)))
        return d_rank

    # The plain form (a non-canonical index) and the bidirected one (`bi`: a canonical index, section 6l) go through the same four helpers.
    def _unitig_fn(self, bi: bool, name: str):
        """The library's cblx_`name`, or its bidirected twin (unitig_table -> cblx_biunitig_table)."""
        return getattr(self._L, "cblx_" + ("bi" if bi else "") + name)

    def _unitig_counts(self, bi: bool, device: bool = False, per_kmer=None, per_unitig=(None, None, None), cap: int = 0):
        """(k-mers, unitigs, circular unitigs) from the table call, which fills the arrays it is given (`reversed` exists only with bi)."""
        per_kmer = per_kmer or (None,) * (3 if bi else 2)
        n, u, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(self._unitig_fn(bi, "unitig_table_device" if device else "unitig_table")(
            self._h, *map(_ptr, per_kmer), cap, *map(_ptr, per_unitig), cap, C.byref(n), C.byref(u), C.byref(c)))
        return n.value, u.value, c.value

    def _unitig_table(self, xp, bi: bool) -> dict:
        """The compaction table in arrays of `xp`: numpy (host, zeroed) or torch (tensors on the index's device)."""
        device = xp.__name__ == "torch"
        cap = max(self.count(), 1)
        if device:
            dev = xp.device("cuda", self.device())
            new, own = (lambda dtype: xp.empty(cap, dtype=dtype, device=dev)), (lambda a: a.clone())
        else:
            new, own = (lambda dtype: xp.zeros(cap, dtype=dtype)), (lambda a: a.copy())
        unitig, offset, head, length = (new(xp.int32 if device else xp.uint32) for _ in range(4))
        rev, flags = (new(xp.uint8) if bi else None), new(xp.uint8)
        n, u, c = self._unitig_counts(bi, device, (unitig, offset, rev) if bi else (unitig, offset), (head, length, flags), cap)
        out = {"unitig": unitig[:n], "offset": offset[:n]}
        if bi:
            out["reversed"] = rev[:n]
        out.update(head=own(head[:u]), length=own(length[:u]), flags=own(flags[:u]), n_circular=c)
        return out

    def _unitig_sizes(self, bi: bool, name: str, *args):
        """cblx_`name`(handle, *args, &a, &b) -> (a, b): (bytes, unitigs) of the text-device call, (unitigs, bytes) of the to-file / to-fd calls."""
        a, b = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._unitig_fn(bi, name)(self._h, *args, C.byref(a), C.byref(b)))
        return a.value, b.value

    def _text_lines(self, text_np):
        """Generator of the lines of the uint8 array text_np() returns, as str."""
        for line in text_np().tobytes().split(b"\n")[:-1]:
            yield line.decode("ascii")

    def unitig_counts(self):
        """(k-mers, unitigs, circular unitigs) of a non-canonical index; the whole compaction runs on the device, three numbers come back."""
        return self._unitig_counts(False)

    def unitig_table_np(self) -> dict:
        """The compaction table of a non-canonical index: per k-mer, by ordinal, `unitig` and `offset` (uint32); per unitig `head` (the
        ordinal of its first k-mer), `length` (k-mers; uint32) and `flags` (uint8, bit 0 = circular); and `n_circular`. The unitigs are
        the paths and cycles of the simple edges (x -> y with one successor of x and one predecessor of y in the set), numbered by
        ascending ordinal of their heads; the head of a cycle is its member with the smallest ordinal."""
        import numpy as np

        return self._unitig_table(np, False)

    def unitig_table_device(self) -> dict:
        """The same table as torch CUDA tensors (int32 holding the unsigned 32-bit values, uint8 for `flags`); nothing crosses to the host but
        the three counts."""
        import torch

        return self._unitig_table(torch, False)

    def unitigs_text_device(self, d_buf=None, cap: int = 0):
        """(bytes, unitigs) of the unitig text: count() + unitigs * K bytes, one line per unitig — the K letters of its head, the last
        letter of every following k-mer, '\n'. With d_buf (a torch uint8 CUDA tensor or raw device address of `cap` bytes) the text is
        written there; without, only the two sizes are computed. A buffer too small raises CblxError(ERANGE) and is left untouched."""
        return self._unitig_sizes(False, "unitigs_text_device", _ptr(d_buf), cap)

    def _text_np(self, to_fd):
        """What to_fd(descriptor) writes, as a uint8 array: a pipe, read by a thread while the library streams into it."""
        import threading

        import numpy as np

        r, w = os.pipe()
        got = []

        def reader():
            with os.fdopen(r, "rb") as f:
                got.append(f.read())

        t = threading.Thread(target=reader)
        t.start()
        try:
            to_fd(w)
        finally:
            os.close(w)
            t.join()
        return np.frombuffer(got[0], dtype=np.uint8)

    def unitigs_text_np(self):
        """The unitig text as a uint8 array (see unitigs_text_device), built on the device and streamed out once."""
        return self._text_np(self.unitigs_to_fd)

    def unitigs(self):
        """Generator of the unitigs as str, in unitig order (the text is built once, before the first one is yielded)."""
        return self._text_lines(self.unitigs_text_np)

    def unitigs_to_file(self, path, chunk_bytes: int = 0):
        """Writes the unitig text to `path` (created / truncated), streamed from the device in chunks of chunk_bytes (0 = the library's
        default); returns (unitigs, bytes)."""
        return self._unitig_sizes(False, "unitigs_to_file", os.fsencode(path), chunk_bytes)

    def unitigs_to_fd(self, fd: int, chunk_bytes: int = 0):
        """The same to an open file descriptor (flush any Python-level buffer over it first)."""
        return self._unitig_sizes(False, "unitigs_to_fd", fd, chunk_bytes)

    @staticmethod
    def unitig_summary(length, flags, k: int) -> dict:
        """What the `length` and `flags` of a compaction table — unitig_table_np's or biunitig_table_np's — say (host only): unitigs, circular ones, kmers = sum of the lengths,
        bases = sum of (length + k - 1), the longest unitig in k-mers, and n50: the largest L in bases such that the unitigs of at
        least L bases hold at least half of all bases (0 for an empty table)."""
        ls = [int(v) for v in length]
        fs = [int(v) for v in flags]
        if len(ls) != len(fs):
            raise ValueError("unitig_summary: length and flags differ in length")
        if k < 1 or any(v < 1 for v in ls):
            raise ValueError("unitig_summary: k and every length are at least 1")
        bases = sorted((v + k - 1 for v in ls), reverse=True)
        total, acc, n50 = sum(bases), 0, 0
        for b in bases:
            acc += b
            if 2 * acc >= total:
                n50 = b
                break
        return {"unitigs": len(ls), "circular": sum(f & 1 for f in fs), "kmers": sum(ls), "bases": total, "longest": max(ls, default=0), "n50": n50}

    # ---- bidirected unitigs: the unitigs of a canonical index with odd K --------------------------------------
    def biunitig_counts(self):
        """(k-mers, unitigs, circular unitigs) of a canonical index with odd K: the compaction over oriented k-mers runs on the device,
        three numbers come back."""
        return self._unitig_counts(True)

    def biunitig_table_np(self) -> dict:
        """The compaction table of a canonical index: the dict of unitig_table_np plus `reversed` (uint8 per k-mer, by ordinal): 1 where the
        unitig runs through the reverse complement of the stored form. An edge joins two ORIENTED k-mers; it is simple when the one has
        one successor, the other one predecessor, and they are not the same stored k-mer (so poly-A alone is a unitig of length 1 that is
        not circular, unlike unitig_table_np). Of a unitig's two mirror images the one whose head has the smaller ordinal than its tail
        is kept (a cycle: the one whose smallest member is not reversed)."""
        import numpy as np

        return self._unitig_table(np, True)

    def biunitig_table_device(self) -> dict:
        """The same table as torch CUDA tensors (int32 holding the unsigned 32-bit values, uint8 for `reversed` and `flags`); nothing crosses
        to the host but the three counts."""
        import torch

        return self._unitig_table(torch, True)

    def biunitigs_text_device(self, d_buf=None, cap: int = 0):
        """(bytes, unitigs) of the bidirected unitig text: count() + unitigs * K bytes, one line per unitig — the K letters its head spells
        in its orientation, the last letter every following member spells in its own, '\n'. d_buf and cap as in unitigs_text_device."""
        return self._unitig_sizes(True, "unitigs_text_device", _ptr(d_buf), cap)

    def biunitigs_text_np(self):
        """The bidirected unitig text as a uint8 array, built on the device and streamed out once."""
        return self._text_np(self.biunitigs_to_fd)

    def biunitigs(self):
        """Generator of the bidirected unitigs as str, in unitig order (the text is built once, before the first one is yielded)."""
        return self._text_lines(self.biunitigs_text_np)

    def biunitigs_to_file(self, path, chunk_bytes: int = 0):
        """Writes the bidirected unitig text to `path` (created / truncated), streamed from the device in chunks of chunk_bytes (0 = the
        library's default); returns (unitigs, bytes)."""
        return self._unitig_sizes(True, "unitigs_to_file", os.fsencode(path), chunk_bytes)

    def biunitigs_to_fd(self, fd: int, chunk_bytes: int = 0):
        """The same to an open file descriptor (flush any Python-level buffer over it first)."""
        return self._unitig_sizes(True, "unitigs_to_fd", fd, chunk_bytes)

    # ---- the links between the unitigs and the GFA text of the compacted graph; the form follows the index -----------
    def _gfa_links(self, device: bool, link_start=None, cap_starts: int = 0, link_to=None, link_rev=None, cap_links: int = 0):
        u, ln = C.c_uint64(0), C.c_uint64(0)
        fn = self._L.cblx_gfa_links_device if device else self._L.cblx_gfa_links
        self._chk(fn(self._h, _ptr(link_start), cap_starts, _ptr(link_to), _ptr(link_rev), cap_links, C.byref(u), C.byref(ln)))
        return u.value, ln.value

    def _gfa_sizes(self, name: str, *args):
        """cblx_`name`(handle, *args, &a, &b, &c) -> (a, b, c)."""
        a, b, c = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        self._chk(getattr(self._L, "cblx_" + name)(self._h, *args, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def gfa_counts(self):
        """(unitigs, links) of the compacted de Bruijn graph: the unitigs of unitig_table_np (a non-canonical index) or biunitig_table_np (a
        canonical one), and the edges between them — every edge of the graph that does not join two consecutive k-mers of one unitig."""
        return self._gfa_links(False)

    def _gfa_table(self, xp) -> dict:
        device = xp.__name__ == "torch"
        u, ln = self._gfa_links(device)
        if device:
            dev = xp.device("cuda", self.device())
            new = lambda count, dtype: xp.empty(max(count, 1), dtype=dtype, device=dev)  # noqa: E731
            start, to, rev = new(2 * u + 1, xp.int64), new(ln, xp.int32), new(ln, xp.uint8)
        else:
            start, to, rev = xp.zeros(2 * u + 1, dtype=xp.uint64), xp.zeros(max(ln, 1), dtype=xp.uint32), xp.zeros(max(ln, 1), dtype=xp.uint8)
        u2, ln2 = self._gfa_links(device, start, 2 * u + 1, to, rev, ln)
        assert (u2, ln2) == (u, ln)
        return {"link_start": start[: 2 * u + 1], "link_to": to[:ln], "link_rev": rev[:ln], "n_unitigs": u, "n_links": ln}

    def gfa_links_np(self) -> dict:
        """The link table between the unitigs. Unitig u has slot 2 u ('+', the image the unitig text spells) and, of a canonical index, slot
        2 u + 1 ('-', its reverse complement). `link_start` (uint64, 2 U + 1 entries) is the CSR over the slots: the links leaving slot a are
        [link_start[a], link_start[a + 1]); `link_to` (uint32) is the unitig a link enters and `link_rev` (uint8) is 0 where it enters it at the
        head of '+' and 1 at the head of '-'. Links of a slot are in ascending code of the appended base. Also `n_unitigs` and `n_links`.
        Bidirected links come in mirror pairs (see gfa_link_tuples)."""
        import numpy as np

        return self._gfa_table(np)

    def gfa_links_device(self) -> dict:
        """The same table as torch CUDA tensors (int64 / int32 holding the unsigned values, uint8 for `link_rev`); only the two counts cross
        to the host."""
        import torch

        return self._gfa_table(torch)

    @staticmethod
    def gfa_link_tuples(link_start, link_to, link_rev):
        """Generator of (u, '+' | '-', v, '+' | '-') over a link table in table order (host only): the link leaves the end of unitig u read in
        the first orientation and enters the start of unitig v read in the second. The table of a canonical index holds both members of
        every mirror pair, (u, a, v, b) and (v, not b, u, not a)."""
        starts = [int(s) for s in link_start]
        for slot in range(len(starts) - 1):
            for ln in range(starts[slot], starts[slot + 1]):
                yield slot >> 1, "-" if slot & 1 else "+", int(link_to[ln]), "-" if int(link_rev[ln]) else "+"

    def gfa_text_device(self, d_buf=None, cap: int = 0):
        """(bytes, unitigs, L lines) of the GFA 1.0 text: a header, an S line per unitig carrying its line of the unitig text, an L line per
        link with the overlap (K - 1)M — of a mirror pair of links one line. d_buf and cap as in unitigs_text_device."""
        return self._gfa_sizes("gfa_text_device", _ptr(d_buf), cap)

    def gfa_text_np(self):
        """The GFA text as a uint8 array, built on the device and streamed out once."""
        return self._text_np(self.gfa_to_fd)

    def gfa_to_file(self, path, chunk_bytes: int = 0):
        """Writes the GFA text to `path` (created / truncated), streamed from the device in chunks of chunk_bytes (0 = the library's
        default); returns (unitigs, L lines, bytes)."""
        return self._gfa_sizes("gfa_to_file", os.fsencode(path), chunk_bytes)

    def gfa_to_fd(self, fd: int, chunk_bytes: int = 0):
        """The same to an open file descriptor (flush any Python-level buffer over it first)."""
        return self._gfa_sizes("gfa_to_fd", fd, chunk_bytes)

    # ---- tip clipping on the compacted graph; the form follows the index ---------------------------------------------
    def _max_kmers(self, max_kmers):
        return self.k - 1 if max_kmers is None else int(max_kmers)

    def _unitig_ends(self, xp) -> dict:
        device = xp.__name__ == "torch"
        fn = self._L.cblx_unitig_ends_device if device else self._L.cblx_unitig_ends
        u = C.c_uint64(0)
        self._chk(fn(self._h, None, None, 0, C.byref(u)))
        cap = max(u.value, 1)
        if device:
            dev = xp.device("cuda", self.device())
            left, right = (xp.empty(cap, dtype=xp.uint8, device=dev) for _ in range(2))
        else:
            left, right = (xp.zeros(cap, dtype=xp.uint8) for _ in range(2))
        self._chk(fn(self._h, _ptr(left), _ptr(right), cap, C.byref(u)))
        return {"left": left[: u.value], "right": right[: u.value], "n_unitigs": u.value}

    def unitig_ends_np(self) -> dict:
        """The degrees at the two ends of every unitig of unitig_table_np (a non-canonical index) or biunitig_table_np (a canonical one), as uint8
        arrays: `right` = the out-degree of the last k-mer of the unitig as its text spells it, `left` = the in-degree of its first one — the
        links that leave and that enter the unitig in the link table of gfa_links_np. Self-edges and hairpins count. Also `n_unitigs`."""
        import numpy as np

        return self._unitig_ends(np)

    def unitig_ends_device(self) -> dict:
        """The same as torch uint8 CUDA tensors; only the count crosses to the host."""
        import torch

        return self._unitig_ends(torch)

    def _tips_mark(self, device: bool, max_kmers, kind=None, cap: int = 0):
        u, counts = C.c_uint64(0), (C.c_uint64 * 4)()
        fn = self._L.cblx_tips_mark_device if device else self._L.cblx_tips_mark
        self._chk(fn(self._h, self._max_kmers(max_kmers), _ptr(kind), cap, C.byref(u), counts))
        return u.value, dict(zip(TIP_COUNTS, (int(v) for v in counts)))

    def tip_counts(self, max_kmers=None) -> dict:
        """tips, tip_kmers, isolated, isolated_kmers of tips_np, and n_unitigs: the marks are made on the device, five numbers come back."""
        u, counts = self._tips_mark(False, max_kmers)
        return dict(counts, n_unitigs=u)

    def tips_np(self, max_kmers=None) -> dict:
        """`kind` (uint8 per unitig of the index's compaction table): 1, a tip, where the unitig has at most max_kmers k-mers (None: K - 1, unitigs
        shorter than K k-mers) and exactly one of its ends (unitig_ends_np) has degree 0; 2, isolated, where it is that short and both have; 0
        elsewhere. A circular unitig is never marked. Also the counts of tip_counts."""
        import numpy as np

        u, _ = self._tips_mark(False, max_kmers)
        kind = np.zeros(max(u, 1), dtype=np.uint8)
        u, counts = self._tips_mark(False, max_kmers, kind, max(u, 1))
        return dict(counts, kind=kind[:u], n_unitigs=u)

    def tips_mark_device(self, max_kmers=None, d_kind=None, cap: int = 0) -> dict:
        """The marks into d_kind (a torch uint8 CUDA tensor or raw device address of `cap` elements; None: counts only); returns the counts of
        tip_counts. A capacity too small raises CblxError(ERANGE) and leaves d_kind untouched."""
        u, counts = self._tips_mark(True, max_kmers, d_kind, cap)
        return dict(counts, n_unitigs=u)

    @staticmethod
    def tip_kinds(length, flags, left, right, max_kmers: int):
        """The rule of tips_np restated in numpy on a compaction table's `length` and `flags` and on unitig_ends_np's arrays (host only): a uint8
        array of kinds. The circular flag is not consulted — a circular unitig has both degrees >= 1 — but a marked circular unitig raises."""
        import numpy as np

        if max_kmers < 1:
            raise ValueError("tip_kinds: max_kmers is at least 1")
        length, left, right = np.asarray(length).astype(np.int64), np.asarray(left).astype(np.int64), np.asarray(right).astype(np.int64)
        short = length <= max_kmers
        kind = np.where(short & (left == 0) & (right == 0), 2, np.where(short & ((left == 0) != (right == 0)), 1, 0)).astype(np.uint8)
        if ((np.asarray(flags) & 1).astype(bool) & (kind != 0)).any():
            raise ValueError("tip_kinds: a circular unitig without a link")
        return kind

    def clip_tips(self, max_kmers=None, isolated: bool = False, rounds: int = 1) -> dict:
        """Removes the k-mers of the tips (tips_np; with `isolated` those of the isolated unitigs too) from the index, on the device: a round
        compacts, marks and removes every marked unitig of that compaction as one batch, so a short stem that forks into two short dead ends goes
        whole. `rounds` = 0 repeats until a round finds nothing. Returns rounds (compactions run), tips, tip_kmers, isolated, isolated_kmers (what
        was removed), kmers_left and fixpoint (1 when the last round found nothing)."""
        st = ClipStats()
        self._chk(self._L.cblx_clip_tips(self._h, self._max_kmers(max_kmers), CLIP_ISOLATED if isolated else 0, int(rounds), C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in ClipStats._fields_}

    # ---- connected components of the compacted graph; the form follows the index -------------------------------------
    def _components(self, device: bool, component=None, cap_unitigs: int = 0, kmer_component=None, cap_kmers: int = 0, first=None, unitigs=None, kmers=None,
                    cap_components: int = 0) -> dict:
        counts = (C.c_uint64 * 6)()
        fn = self._L.cblx_components_device if device else self._L.cblx_components
        self._chk(fn(self._h, _ptr(component), cap_unitigs, _ptr(kmer_component), cap_kmers, _ptr(first), _ptr(unitigs), _ptr(kmers), cap_components, counts))
        return dict(zip(COMPONENT_COUNTS, (int(v) for v in counts)))

    def component_counts(self) -> dict:
        """kmers, unitigs, links, components, largest_kmers and rounds of the connected components of the compacted de Bruijn graph: the labelling
        runs on the device, six numbers come back. `rounds` is the number of hook-and-compress rounds the labelling took (the last one, which
        changes nothing, included; 0 for an empty index)."""
        return self._components(False)

    def _component_table(self, xp, per_kmer: bool) -> dict:
        device = xp.__name__ == "torch"
        ct = self._components(device)
        n, u, nc = ct["kmers"], ct["unitigs"], ct["components"]
        if device:
            dev = xp.device("cuda", self.device())
            new = lambda count, dtype: xp.empty(max(count, 1), dtype=dtype, device=dev)  # noqa: E731
            i32, i64 = xp.int32, xp.int64
        else:
            new = lambda count, dtype: xp.zeros(max(count, 1), dtype=dtype)  # noqa: E731
            i32, i64 = xp.uint32, xp.uint64
        component, first, unitigs, kmers = new(u, i32), new(nc, i32), new(nc, i32), new(nc, i64)
        kc = new(n, i32) if per_kmer else None
        ct2 = self._components(device, component, u, kc, n if per_kmer else 0, first, unitigs, kmers, nc)
        assert ct2 == ct
        out = {"component": component[:u], "first": first[:nc], "unitigs": unitigs[:nc], "kmers": kmers[:nc], "n_kmers": n, "n_unitigs": u, "n_links": ct["links"],
               "n_components": nc, "largest_kmers": ct["largest_kmers"], "rounds": ct["rounds"]}
        if per_kmer:
            out["kmer_component"] = kc[:n]
        return out

    def components_np(self, per_kmer: bool = False) -> dict:
        """The connected components of the compacted graph — the weakly connected components of the de Bruijn graph on the stored k-mers; a
        unitig and its reverse complement are one node. `component` (uint32 per unitig of unitig_table_np / biunitig_table_np), and per
        component `first` (its smallest unitig; the components are numbered by ascending `first`), `unitigs` (uint32) and `kmers` (uint64, the
        sum of its unitigs' lengths). With per_kmer also `kmer_component` (uint32 per k-mer, by ordinal). Also n_kmers, n_unitigs, n_links,
        n_components, largest_kmers and rounds."""
        import numpy as np

        return self._component_table(np, per_kmer)

    def components_device(self, per_kmer: bool = False) -> dict:
        """The same table as torch CUDA tensors (int32 / int64 holding the unsigned values); only the six counts cross to the host."""
        import torch

        return self._component_table(torch, per_kmer)

    def components_filter(self, min_kmers=None, largest: bool = False) -> dict:
        """Removes whole components from the index, on the device: with min_kmers every component of fewer than min_kmers k-mers, with `largest`
        every component but the one of most k-mers (a tie: the lower number). Exactly one of the two is given. The k-mers go as one batch, in
        iteration order. Returns components, removed_components, removed_kmers, kmers_left, largest_kmers (before the removal) and rounds."""
        st = ComponentStats()
        self._chk(self._L.cblx_components_filter(self._h, 0 if min_kmers is None else int(min_kmers), COMPONENTS_LARGEST if largest else 0, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in ComponentStats._fields_}

    @staticmethod
    def component_summary(kmers, unitigs) -> dict:
        """What the per-component `kmers` and `unitigs` of components_np say (host only): components, largest (the k-mers of the largest one),
        singletons (components of one unitig) and largest_fraction (the k-mers held by the largest as a fraction of all; 0.0 for no component)."""
        ks, us = [int(v) for v in kmers], [int(v) for v in unitigs]
        if len(ks) != len(us):
            raise ValueError("component_summary: kmers and unitigs differ in length")
        if any(v < 1 for v in ks) or any(v < 1 for v in us) or any(k < u for k, u in zip(ks, us)):
            raise ValueError("component_summary: every component has at least one unitig and at least as many k-mers as unitigs")
        total, big = sum(ks), max(ks, default=0)
        return {"components": len(ks), "largest": big, "singletons": sum(1 for u in us if u == 1), "largest_fraction": big / total if total else 0.0}

    # ---- k-mer abundances from reads: the counts are the caller's tensor, one uint32 per stored k-mer by ordinal ---------
    def _counts(self, counts):
        """(tensor, address, length) of an abundance array: a torch int32 CUDA tensor holding the unsigned values; None -> zero-filled, count() long."""
        import torch

        if counts is None:
            counts = torch.zeros(self.count(), dtype=torch.int32, device=torch.device("cuda", self.device()))
        if not (counts.is_cuda and counts.dtype == torch.int32 and counts.is_contiguous()):
            raise ValueError("counts is a contiguous torch int32 CUDA tensor (it holds the unsigned 32-bit values)")
        return counts, (counts.data_ptr() if counts.numel() else None), counts.numel()

    def abundance_seqs(self, bases, offsets, counts=None):
        """Adds to counts[i] the occurrences of stored k-mer i (by ordinal, the index in the iteration order) in a host batch of reads (bases: uint8
        array, offsets: uint64 array of n + 1 entries), saturating at 2^32 - 1: k-mers as contains_seqs enumerates them, both strands for a
        canonical index; a read shorter than K gives none. The call accumulates into `counts` (None: a zero-filled tensor made here) and refuses
        a tensor whose length is not count(). Returns (counts, k-mers of the batch, those the index holds). The index is not modified."""
        counts, p, m = self._counts(counts)
        tot, found = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_abundance_seqs(self._h, _ptr(bases), _ptr(offsets), max(len(offsets) - 1, 0), p, m, C.byref(tot), C.byref(found)))
        return counts, tot.value, found.value

    def abundance_seqs_device(self, d_bases, d_offsets, n: int, counts=None):
        """The same for a device-resident batch (d_bases 16-byte aligned); nothing crosses to the host but the two totals."""
        counts, p, m = self._counts(counts)
        tot, found = C.c_uint64(0), C.c_uint64(0)
        self._chk(self._L.cblx_abundance_seqs_device(self._h, _ptr(d_bases), _ptr(d_offsets), n, p, m, C.byref(tot), C.byref(found)))
        return counts, tot.value, found.value

    def abundance_histogram(self, counts):
        """The abundance spectrum as a uint64 array of 256: hist[j] = the stored k-mers with counts[i] == j for j < 255, hist[255] = those with
        counts[i] >= 255."""
        import numpy as np

        counts, p, m = self._counts(counts)
        hist = np.zeros(256, dtype=np.uint64)
        self._chk(self._L.cblx_abundance_histogram(self._h, p, m, hist.ctypes.data_as(C.POINTER(C.c_uint64))))
        return hist

    def _unitig_coverage(self, xp, counts):
        device = xp.__name__ == "torch"
        counts, p, m = self._counts(counts)
        fn = self._L.cblx_unitig_coverage_device if device else self._L.cblx_unitig_coverage
        u = C.c_uint64(0)
        self._chk(fn(self._h, p, m, None, 0, C.byref(u)))
        cap = max(u.value, 1)
        kc = xp.zeros(cap, dtype=xp.int64, device=counts.device) if device else xp.zeros(cap, dtype=xp.uint64)
        self._chk(fn(self._h, p, m, _ptr(kc), cap, C.byref(u)))
        return kc[: u.value]

    def unitig_coverage_np(self, counts):
        """kc (uint64 per unitig of unitig_table_np / biunitig_table_np): the sum of counts over the unitig's k-mers. Mean coverage is kc / length."""
        import numpy as np

        return self._unitig_coverage(np, counts)

    def unitig_coverage_device(self, counts):
        """The same as a torch int64 CUDA tensor holding the unsigned values; only the number of unitigs crosses to the host."""
        import torch

        return self._unitig_coverage(torch, counts)

    def _counts_or_none(self, counts):
        return (None, 0) if counts is None else self._counts(counts)[1:]

    def gfa_tagged_text_device(self, counts=None, d_buf=None, cap: int = 0):
        """(bytes, unitigs, L lines) of the tagged GFA text; d_buf and cap as in gfa_text_device."""
        p, m = self._counts_or_none(counts)
        return self._gfa_sizes("gfa_tagged_text_device", p, m, _ptr(d_buf), cap)

    def gfa_tagged_to_fd(self, fd: int, counts=None, chunk_bytes: int = 0):
        """The tagged GFA text to an open file descriptor; returns (unitigs, L lines, bytes)."""
        p, m = self._counts_or_none(counts)
        return self._gfa_sizes("gfa_tagged_to_fd", p, m, fd, chunk_bytes)

    def gfa_tagged_to_file(self, path, counts=None, chunk_bytes: int = 0):
        """Writes the GFA text of gfa_to_file with the tags LN:i:<bases> and, with `counts`, KC:i:<the unitig's coverage sum> on every S line."""
        p, m = self._counts_or_none(counts)
        return self._gfa_sizes("gfa_tagged_to_file", p, m, os.fsencode(path), chunk_bytes)

    def gfa_tagged_text_np(self, counts=None):
        """The tagged GFA text as a uint8 array, built on the device and streamed out once."""
        return self._text_np(lambda fd: self.gfa_tagged_to_fd(fd, counts))

    def abundance_filter(self, counts, min_count: int, unitigs: bool = False) -> dict:
        """Removes the weakly supported k-mers, on the device, as one batch in iteration order: every k-mer with counts[i] < min_count, or with
        `unitigs` every k-mer of every unitig whose mean coverage is below min_count (kc < min_count * length). `counts` is only read; after a
        call that removed something it no longer matches the index: tally again. Returns kmers, removed_kmers, unitigs, removed_unitigs (both 0
        under the k-mer rule), kmers_left and min_count."""
        counts, p, m = self._counts(counts)
        st = AbundanceStats()
        self._chk(self._L.cblx_abundance_filter(self._h, p, m, int(min_count), ABUNDANCE_UNITIGS if unitigs else 0, C.byref(st)))
        return {name: int(getattr(st, name)) for name, _ in AbundanceStats._fields_}

    # ---- bubble popping on the compacted graph; the form follows the index ------------------------------------------
    def _bubble_max(self, max_kmers):
        return 2 * self.k if max_kmers is None else int(max_kmers)

    def _bubbles_mark(self, device: bool, max_kmers, counts=None, kind=None, cap: int = 0):
        p, m = self._counts_or_none(counts)
        u, out = C.c_uint64(0), (C.c_uint64 * 3)()
        fn = self._L.cblx_bubbles_mark_device if device else self._L.cblx_bubbles_mark
        self._chk(fn(self._h, self._bubble_max(max_kmers), p, m, _ptr(kind), cap, C.byref(u), out))
        return u.value, dict(zip(BUBBLE_COUNTS, (int(v) for v in out)))

    def bubble_counts(self, max_kmers=None, counts=None) -> dict:
        """bubbles, popped, popped_kmers of bubbles_np, and n_unitigs: the marks are made on the device, four numbers come back."""
        u, out = self._bubbles_mark(False, max_kmers, counts)
        return dict(out, n_unitigs=u)

    def bubbles_np(self, max_kmers=None, counts=None):
        """(kind, counts_dict). `kind` (uint8 per unitig of the index's compaction table) marks the simple bubbles of the compacted graph: arms are
        unitigs of at most max_kmers k-mers (None: 2 K — the arms of a SNP have K k-mers, those of a small indel a few more) with one link in and one
        link out, and the arms that share their source and their target are a group. In a group of two or more, kind = 2 (kept) for the arm of the
        highest mean coverage kc / length under `counts` (a tensor as abundance_seqs fills it; ties and counts=None: the longest, then the lowest
        number) and 1 (popped) for the others; 0 elsewhere. counts_dict: bubbles (kept arms), popped, popped_kmers, n_unitigs."""
        import numpy as np

        u, _ = self._bubbles_mark(False, max_kmers, counts)
        kind = np.zeros(max(u, 1), dtype=np.uint8)
        u, out = self._bubbles_mark(False, max_kmers, counts, kind, max(u, 1))
        return kind[:u], dict(out, n_unitigs=u)

    def bubbles_mark_device(self, max_kmers=None, counts=None, d_kind=None, cap: int = 0) -> dict:
        """The marks into d_kind (a torch uint8 CUDA tensor or raw device address of `cap` elements; None: counts only); returns the counts of
        bubble_counts. A capacity too small raises CblxError(ERANGE) and leaves d_kind untouched."""
        u, out = self._bubbles_mark(True, max_kmers, counts, d_kind, cap)
        return dict(out, n_unitigs=u)

    @staticmethod
    def bubble_kinds(link_start, link_to, link_rev, length, left, kc, max_kmers: int):
        """The rule of bubbles_np restated on the arrays of gfa_links_np and a compaction table's `length` (host only): a uint8 array of kinds.
        `left` (unitig_ends_np) is given for a non-canonical index and None for a canonical one, where the in-degree of an image is the out-degree
        of its other image; `kc` (unitig_coverage_np) or None for the length rule."""
        import numpy as np

        if max_kmers < 1:
            raise ValueError("bubble_kinds: max_kmers is at least 1")
        start = [int(v) for v in link_start]
        to, rev, length = [int(v) for v in link_to], [int(v) for v in link_rev], [int(v) for v in length]
        cov = None if kc is None else [int(v) for v in kc]
        links = lambda x: [2 * to[j] + rev[j] for j in range(start[x], start[x + 1])]  # noqa: E731
        indeg = (lambda x: start[(x ^ 1) + 1] - start[x ^ 1]) if left is None else (lambda x: int(left[x >> 1]))
        groups = {}
        for a in range(len(start) - 1):
            for x in links(a):
                p = x >> 1
                if indeg(x) != 1 or len(links(x)) != 1 or length[p] > max_kmers:
                    continue
                t = links(x)[0]
                if p in (a >> 1, t >> 1):
                    continue
                key = (a, t) if left is not None else min((a, t), (t ^ 1, a ^ 1))
                groups.setdefault(key, set()).add(p)

        def above(u, v):
            if cov is not None and cov[u] * length[v] != cov[v] * length[u]:
                return cov[u] * length[v] > cov[v] * length[u]
            return (length[u], -u) > (length[v], -v)

        kind = np.zeros(len(length), dtype=np.uint8)
        for members in groups.values():
            if len(members) >= 2:
                for u in members:
                    kind[u] = 1 if any(above(v, u) for v in members if v != u) else 2
        return kind

    def pop_bubbles(self, max_kmers=None, counts=None, rounds: int = 1):
        """Removes the k-mers of the popped arms (bubbles_np) from the index, on the device: a round compacts, marks and removes every popped arm of
        that compaction as one batch. `rounds` = 0 repeats until a round pops nothing. Returns rounds (compactions run), bubbles, popped,
        popped_kmers (what was removed), kmers_left and fixpoint (1 when the last round popped nothing). With `counts` the coverage rule decides
        and the tensor is carried through the removals in place: returns (stats, counts[:kmers_left]), a view of the caller's tensor whose element
        j is the count of the k-mer of the new ordinal j; the elements behind it are 0."""
        p, m = self._counts_or_none(counts)
        st = BubbleStats()
        self._chk(self._L.cblx_pop_bubbles(self._h, self._bubble_max(max_kmers), p, m, 0, int(rounds), C.byref(st)))
        out = {name: int(getattr(st, name)) for name, _ in BubbleStats._fields_}
        return out if counts is None else (out, counts[: out["kmers_left"]])

    @staticmethod
    def solid_threshold(hist):
        """The first local minimum of an abundance spectrum after bin 0 (host only): the smallest j >= 1 whose bin is followed by a higher one,
        moved back to the first bin of a plateau of equal bins — where the descent from the error peak ends and the rise to the coverage peak
        begins. Bin 0 is not looked at. None when no bin from 1 on is followed by a higher one."""
        h = [int(v) for v in hist]
        j = 1
        while j + 1 < len(h):
            if h[j + 1] > h[j]:  # the spectrum rises behind j: j ends a descent or a plateau
                while j > 1 and h[j - 1] == h[j]:
                    j -= 1  # the first bin of the plateau
                return j
            j += 1
        return None

    # ---- bucket statistics (src/cbl.rs:364-386) ---------------------------------------------------------------------
    def bucket_table_np(self):
        """(prefix, length, kind) arrays of the non-empty buckets, ascending prefixes."""
        import numpy as np

        nb = self.num_buckets()
        prefix = np.empty(max(nb, 1), dtype=np.uint32)
        length = np.empty(max(nb, 1), dtype=np.uint32)
        kind = np.empty(max(nb, 1), dtype=np.uint8)
        got = C.c_uint64(0)
        self._chk(self._L.cblx_bucket_sizes(self._h, _ptr(prefix), _ptr(length), _ptr(kind), nb, C.byref(got)))
        return prefix[: got.value], length[: got.value], kind[: got.value]

    def prefix_load(self) -> float:
        """Proportion of available prefixes used in the set (src/cbl.rs:364-367)."""
        return self.num_buckets() / float(1 << self.prefix_bits)

    def buckets_sizes(self):
        """(prefix, bucket length) pairs, ascending prefixes (src/cbl.rs:370-373)."""
        p, l, _ = self.bucket_table_np()
        return list(zip(p.tolist(), l.tolist()))

    def buckets_size_count(self) -> dict:
        """bucket length -> number of buckets of that length, sorted by length (src/cbl.rs:376-379)."""
        import numpy as np

        _, l, _ = self.bucket_table_np()
        v, c = np.unique(l, return_counts=True)
        return dict(zip(v.tolist(), c.tolist()))

    def buckets_load_repartition(self) -> dict:
        """bucket length -> share of the k-mers held by buckets of that length (src/cbl.rs:382-385)."""
        total = float(max(self.count(), 1))
        return {size: size * n / total for size, n in self.buckets_size_count().items()}

    def bucket_nodes_np(self):
        """Node count of every non-empty bucket, ascending prefixes, as a uint64 array (pairs with bucket_table_np)."""
        import numpy as np

        nb = self.num_buckets()
        nodes = np.empty(max(nb, 1), dtype=np.uint64)
        got = C.c_uint64(0)
        self._chk(self._L.cblx_bucket_nodes(self._h, _ptr(nodes), nb, C.byref(got)))
        return nodes[: got.value]

    def buckets_nodes(self):
        """(prefix, node count) pairs, ascending prefixes (src/cbl.rs:386-390): a Vec bucket counts its words, a Trie bucket its nodes."""
        p, _, _ = self.bucket_table_np()
        return list(zip(p.tolist(), self.bucket_nodes_np().tolist()))

    def buckets_node_count(self) -> dict:
        """node count -> number of buckets with that many nodes, sorted by node count (src/cbl.rs:392-396)."""
        import numpy as np

        v, c = np.unique(self.bucket_nodes_np(), return_counts=True)
        return dict(zip(v.tolist(), c.tolist()))

    # ---- src/cbl.rs:127-160 ---------------------------------------------------------------------------------
    def serialize(self) -> bytes:
        """The exact bytes `save_to_file` writes (bincode DefaultOptions + varint)."""
        return self.serialize_np().tobytes()

    def serialized_size(self) -> int:
        n = C.c_uint64(0)
        self._chk(self._L.cblx_serialized_size(self._h, C.byref(n)))
        return n.value

    def serialize_np(self, out=None):
        """serialize() into a numpy uint8 array (`out` if given and large enough); returns the filled view."""
        import numpy as np

        n = self.serialized_size()
        if out is None or out.size < n:
            out = np.empty(max(n, 1), dtype=np.uint8)
        w = C.c_uint64(0)
        self._chk(self._L.cblx_serialize(self._h, out.ctypes.data_as(C.POINTER(C.c_uint8)), n, C.byref(w)))
        return out[: w.value]

    def save_to_file(self, path):
        self._chk(self._L.cblx_save_to_file(self._h, os.fsencode(path)))

    def load(self, data):
        """Replace the index by a serialized one (bytes, or a numpy uint8 array: no copy is made)."""
        if hasattr(data, "ctypes"):
            self._chk(self._L.cblx_load(self._h, data.ctypes.data, data.size))
        else:
            self._chk(self._L.cblx_load(self._h, data, len(data)))

    @classmethod
    def load_from_file(cls, path, k: int, prefix_bits: int = 24, **kw) -> "CBL":
        """K / PREFIX_BITS are compile-time constants of the reference and not stored in the file."""
        c = cls(k, prefix_bits, **kw)
        c._chk(c._L.cblx_load_from_file(c._h, os.fsencode(path)))
        return c

    # ---- src/cbl.rs:433-449 ---------------------------------------------------------------------------------
    def __ior__(self, other: "CBL") -> "CBL":
        self._chk(self._L.cblx_merge_assign(self._h, other._h))
        return self

    def merge_from(self, a: "CBL", b: "CBL") -> "CBL":
        """self = what `a |= b` would leave in a, with a untouched (b as `|=` leaves it): `self = a.clone(); self |= b` without the copy."""
        self._chk(self._L.cblx_merge_from(self._h, a._h, b._h))
        return self

    # ---- src/cbl.rs:411-431, 451-471, 491-511, 531-551: the operator forms `&mut a OP &mut b` ---------------------
    @staticmethod
    def set_op(a: "CBL", b: "CBL", op: str, out: "CBL" = None) -> "CBL":
        """`a OP b` into a new index (op: "or" | "and" | "sub" | "xor"), or into `out`, whose content is replaced. A bucket only one operand
        holds is cloned as stored; a bucket both hold becomes an ascending Vec and is dropped when empty. `a` and `b` keep their sets; their
        Vec buckets on the prefixes both hold end up sorted, as the reference leaves them."""
        if op not in SETOPS:
            raise ValueError("set_op: op must be one of %s" % ", ".join(repr(o) for o in SETOPS))
        if out is None:
            out = CBL(a.k, a.prefix_bits, canonical=a.is_canonical(), device=a.device())
        out._chk(out._L.cblx_set_op(out._h, a._h, b._h, SETOPS[op]))
        return out

    # ---- src/cbl.rs:106-124: CBL::merge / CBL::intersect of many indexes ------------------------------------------------
    @staticmethod
    def _set_op_many(cbls, op: str, out: "CBL" = None) -> "CBL":
        cbls = list(cbls)
        if not cbls:
            raise ValueError("%s: at least one index" % ("merge" if op == "or" else "intersect"))
        if len(set(map(id, cbls))) != len(cbls):
            raise ValueError("%s: the same index twice" % ("merge" if op == "or" else "intersect"))
        if out is None:
            a = cbls[0]
            out = CBL(a.k, a.prefix_bits, canonical=a.is_canonical(), device=a.device())
        srcs = (C.c_void_p * len(cbls))(*[c._h for c in cbls])
        out._chk(out._L.cblx_set_op_many(out._h, srcs, len(cbls), SETOPS[op]))
        return out

    @staticmethod
    def merge(cbls, out: "CBL" = None) -> "CBL":
        """The union of up to 64 indexes into a new one (or into `out`, whose content is replaced), as the reference's `CBL::merge`: a bucket one index
        holds is cloned as stored; a bucket several hold becomes an ascending Vec, and the Vec buckets of exactly those holders end up sorted."""
        return CBL._set_op_many(cbls, "or", out)

    @staticmethod
    def intersect(cbls, out: "CBL" = None) -> "CBL":
        """The k-mers all of up to 64 indexes hold, as the reference's `CBL::intersect`: only prefixes every index holds are visited; there every Vec
        bucket ends up sorted and the result is an ascending Vec, dropped when empty."""
        return CBL._set_op_many(cbls, "and", out)

    # ---- between merge and intersect: held by at least t of n, and the occupancy histogram (ours) -------
    @staticmethod
    def _many_operands(cbls, who: str):
        cbls = list(cbls)
        if not cbls:
            raise ValueError("%s: at least one index" % who)
        if len(set(map(id, cbls))) != len(cbls):
            raise ValueError("%s: the same index twice" % who)
        return cbls

    @staticmethod
    def at_least(cbls, t: int, out: "CBL" = None) -> "CBL":
        """The k-mers at least `t` of up to 64 indexes hold (1 <= t <= n) into a new index, or into `out`, whose content is replaced. t = 1 is `CBL.merge`
        and, for n >= 2, t = n is `CBL.intersect`, byte for byte, operands included. In between: a prefix fewer than t indexes hold is not visited; on
        the others every holder's Vec bucket ends up sorted and the result bucket is an ascending Vec, dropped when empty. Empty indexes count
        towards n."""
        cbls = CBL._many_operands(cbls, "at_least")
        t = int(t)
        if not 1 <= t <= len(cbls):
            raise ValueError("at_least: the threshold is 1 to the number of indexes (%d), not %d" % (len(cbls), t))
        if out is None:
            a = cbls[0]
            out = CBL(a.k, a.prefix_bits, canonical=a.is_canonical(), device=a.device())
        srcs = (C.c_void_p * len(cbls))(*[c._h for c in cbls])
        out._chk(out._L.cblx_set_at_least(out._h, srcs, len(cbls), t))
        return out

    @staticmethod
    def occupancy(cbls):
        """numpy uint64 [n + 1]: entry j = the distinct k-mers exactly j of the n indexes hold (entry 0 is 0). Their sum is the size of the merge,
        entry n the size of the intersection, the sum of j * entry j the sum of the counts. No index is built, but this is NOT
        `intersection_count`'s untouched-operands guarantee: the operands are left as `CBL.merge` leaves them — on every prefix two or more
        indexes hold, their Vec buckets end up sorted; the sets are unchanged."""
        import numpy as np

        cbls = CBL._many_operands(cbls, "occupancy")
        n = len(cbls)
        hist = np.zeros(n + 1, dtype=np.uint64)
        srcs = (C.c_void_p * n)(*[c._h for c in cbls])
        cbls[0]._chk(cbls[0]._L.cblx_occupancy_counts(srcs, n, hist.ctypes.data_as(C.POINTER(C.c_uint64))))
        return hist

    # ---- comparing two sets: |a AND b| without building an index and without touching the operands -------
    COMMON_ROUTES = ("wave", "workgroup", "merge_path", "sliced")  # cblx_intersection_count's stats[1 .. 4]

    def intersection_count(self, other: "CBL", stats: bool = False):
        """The number of k-mers `self` and `other` both hold. Nothing is built and nothing is sorted: unlike `&`, both operands serialize to the same
        bytes before and after. With `stats`: (count, {"both": prefixes both hold, "wave" | "workgroup" | "merge_path" | "sliced": buckets by route})."""
        n = C.c_uint64(0)
        st = (C.c_uint64 * 5)()
        self._chk(self._L.cblx_intersection_count(self._h, other._h, C.byref(n), st if stats else None))
        if not stats:
            return n.value
        return n.value, dict(zip(("both",) + CBL.COMMON_ROUTES, (int(v) for v in st)))

    @staticmethod
    def similarity(na: int, nb: int, common: int) -> dict:
        """Everything the three sizes |A|, |B|, |A AND B| say about two sets (host only, pure): the sizes of union, differences and symmetric
        difference, Jaccard (1.0 for two empty sets) and the two containments (1.0 for an empty contained set)."""
        na, nb, common = int(na), int(nb), int(common)
        if common < 0 or common > min(na, nb):
            raise ValueError("similarity: 0 <= common <= min(na, nb)")
        union = na + nb - common
        return {"common": common, "union": union, "only_a": na - common, "only_b": nb - common, "sym_diff": na + nb - 2 * common,
                "jaccard": common / union if union else 1.0, "containment_a_in_b": common / na if na else 1.0,
                "containment_b_in_a": common / nb if nb else 1.0}

    @staticmethod
    def set_op_count(a: "CBL", b: "CBL", op: str) -> int:
        """The size `a OP b` would have (op: "or" | "and" | "sub" | "xor"), from the two counts and the intersection: no index is built."""
        if op not in SETOPS:
            raise ValueError("set_op_count: op must be one of %s" % ", ".join(repr(o) for o in SETOPS))
        s = CBL.similarity(a.count(), b.count(), a.intersection_count(b))
        return s[{"or": "union", "and": "common", "sub": "only_a", "xor": "sym_diff"}[op]]

    def jaccard(self, other: "CBL") -> float:
        return CBL.similarity(self.count(), other.count(), self.intersection_count(other))["jaccard"]

    def containment(self, other: "CBL") -> float:
        """The fraction of self's k-mers that `other` holds (1.0 for an empty self)."""
        return CBL.similarity(self.count(), other.count(), self.intersection_count(other))["containment_a_in_b"]

    @staticmethod
    def intersection_matrix(cbls):
        """numpy uint64 (n, n): entry [i, j] = the k-mers indexes i and j share, the diagonal their counts; 1 to 64 different indexes."""
        import numpy as np

        cbls = list(cbls)
        n = len(cbls)
        out = np.zeros((n, n), dtype=np.uint64)
        srcs = (C.c_void_p * max(n, 1))(*[c._h for c in cbls])
        L = cbls[0]._L if cbls else lib()
        rc = L.cblx_intersection_counts(srcs, n, out.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc != 0:
            raise CblxError(rc, (L.cblx_last_error(cbls[0]._h) if cbls else L.cblx_last_global_error()).decode())
        return out

    def device(self) -> int:
        """The HIP device ordinal the index lives on (`device=-1` resolved when it was created)."""
        v = C.c_int32(0)
        self._chk(self._L.cblx_get_device(self._h, C.byref(v)))
        return v.value

    def __or__(self, other: "CBL") -> "CBL":
        return CBL.set_op(self, other, "or")

    def __and__(self, other: "CBL") -> "CBL":
        return CBL.set_op(self, other, "and")

    def __sub__(self, other: "CBL") -> "CBL":
        return CBL.set_op(self, other, "sub")

    def __xor__(self, other: "CBL") -> "CBL":
        return CBL.set_op(self, other, "xor")

    # ---- src/cbl.rs:473-489, 513-529, 553-569: the assigning forms `a OP= &mut b` --------------------------------------
    def set_op_assign(self, other: "CBL", op: str) -> "CBL":
        """`self OP= other` in place (op: "and" | "sub" | "xor" | "or"; "or" is `|=`), as the reference's `&=`, `-=`, `^=` leave both operands:
        a bucket both hold keeps self's kind — a Trie stays ascending, a Vec gets the reference's swap_remove order — and is dropped when empty;
        `other` keeps its set, its Vec buckets on the prefixes both hold end up sorted. Returns self."""
        if op not in SETOPS:
            raise ValueError("set_op_assign: op must be one of %s" % ", ".join(repr(o) for o in SETOPS))
        if op == "or":
            return self.__ior__(other)
        self._chk(self._L.cblx_set_op_assign(self._h, other._h, SETOPS[op]))
        return self

    def _no_assigning_form(self, other):
        # without these Python would rebind `a = a & b`, which is the operator's bucket layout under the assigning form's name
        raise NotImplementedError("`&=`, `-=` and `^=` are spelled a.set_op_assign(b, \"and\" | \"sub\" | \"xor\") (the reference's in-place bucket layout); `a = a & b` is the operator form")

    __iand__ = __isub__ = __ixor__ = _no_assigning_form

    # ---- inspection -------------------------------------------------------------------------------------------
    def consts(self) -> dict:
        c = Consts()
        self._chk(self._L.cblx_get_consts(self._h, C.byref(c)))
        return {n: getattr(c, n) for n, _ in Consts._fields_}

    def buckets(self):
        """[(prefix, kind, [suffix, ...])] in ascending prefix order; kind 0 = Vec (stored order), 1 = Trie (ascending)."""
        out = []

        def cb(_u, prefix, kind, n, lo, hi):
            if hi:
                out.append((prefix, kind, [lo[i] | (hi[i] << 64) for i in range(n)]))
            else:
                out.append((prefix, kind, [lo[i] for i in range(n)]))
            return 0

        self._chk(self._L.cblx_export_buckets(self._h, BUCKET_CB(cb), None))
        return out

    def checksum(self) -> int:
        """Order-independent 64-bit checksum of the set (sum of a hash of every resident word)."""
        v = C.c_uint64(0)
        self._chk(self._L.cblx_checksum(self._h, C.byref(v)))
        return v.value

    def checksum_words_device(self, d_lo, d_hi, n: int) -> int:
        v = C.c_uint64(0)
        self._chk(self._L.cblx_checksum_words_device(self._h, _ptr(d_lo), _ptr(d_hi), n, C.byref(v)))
        return v.value

    def validate(self, strict: bool = True) -> int:
        """Number of structural violations in the resident buckets (0 = sound)."""
        v = C.c_uint64(0)
        self._chk(self._L.cblx_validate(self._h, int(strict), C.byref(v)))
        return v.value

    def stage_times(self) -> dict:
        """{stage: (ms, launches)} accumulated HIP-event time per pipeline stage (needs profile=True)."""
        names = (C.c_char_p * 16)()
        ms = (C.c_double * 16)()
        ln = (C.c_uint64 * 16)()
        n = C.c_uint32(0)
        self._chk(self._L.cblx_stage_times(self._h, names, ms, ln, 16, C.byref(n)))
        return {names[i].decode(): (ms[i], ln[i]) for i in range(n.value)}

    def stage_units(self) -> dict:
        """{stage: words} the stage's kernels were given since the last reset, where the pipeline counts them (`|=`); 0 = not counted."""
        names = (C.c_char_p * 16)()
        n = C.c_uint32(0)
        self._chk(self._L.cblx_stage_times(self._h, names, None, None, 16, C.byref(n)))
        un = (C.c_uint64 * 16)()
        self._chk(self._L.cblx_stage_units(self._h, un, 16, C.byref(n)))
        return {names[i].decode(): un[i] for i in range(n.value)}

    def stage_times_reset(self):
        self._chk(self._L.cblx_stage_times_reset(self._h))

    def kmers_inserted(self) -> int:
        v = C.c_uint64(0)
        self._chk(self._L.cblx_kmers_inserted(self._h, C.byref(v)))
        return v.value

    def fine_builds(self) -> int:
        """Batches built through the FINE-bins route (PREFIX_BITS > 24, empty index, CBLX_FINE_MIN k-mers or more)."""
        v = C.c_uint64(0)
        self._chk(self._L.cblx_fine_builds(self._h, C.byref(v)))
        return v.value

    def uniform_plans(self) -> int:
        """Insert batches whose chunk plan was arithmetic (reads of one length, no invalid byte): no chunk table was built."""
        v = C.c_uint64(0)
        self._chk(self._L.cblx_uniform_plans(self._h, C.byref(v)))
        return v.value

    def trim(self):
        self._chk(self._L.cblx_trim(self._h))

    def clear(self):
        """Back to `CBL::new()`: empty set, cached device workspace kept."""
        self._chk(self._L.cblx_clear(self._h))
