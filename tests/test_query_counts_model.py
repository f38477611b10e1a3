"""The per-sequence query tallies without a GPU: the numpy model of the two-level tally in tests/query_counts_shapes.py equals a
direct per-sequence count from the oracle, the crafted batch holds every named length and edge, and the three entry points exist
in the header, the bindings and the CLI."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cbl_amd
import query_counts_shapes as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cblx_contains_seqs_counts", "cblx_contains_seqs_counts_device", "cblx_query_fastx_file_counts")


@pytest.mark.parametrize("k,pb,canonical", qc.CONFIGS)
def test_model_equals_direct_count(k, pb, canonical):
    b, o, want = qc.case(k, pb, canonical)
    seq_chunk, kmer_off = qc.chunk_tables(b.bases, b.offsets, k)
    assert len(seq_chunk) == len(b.seqs) + 1 and kmer_off[-1] == len(want.flags)
    total, positive, chunk_pos = qc.tally_model(want.flags, kmer_off, seq_chunk)
    assert np.array_equal(total, want.total) and np.array_equal(positive, want.positive)
    assert int(chunk_pos.sum()) == int(want.flags.sum()) == int(want.positive.sum())
    # both outcomes occur: every second sequence is resident and found whole, the others miss most of their k-mers
    assert np.array_equal(want.positive[::2], want.total[::2])
    assert int(want.positive[1::2].sum()) < int(want.total[1::2].sum()) // 10


@pytest.mark.parametrize("k", sorted({c[0] for c in qc.CONFIGS}))
def test_batch_holds_every_named_length_and_edge(k):
    b = qc.batch(k)
    C = qc.CHUNK_KMERS
    ix = {n: i for i, n in enumerate(b.names)}
    assert len(ix) == len(b.names) == len(b.seqs) == len(b.offsets) - 1
    ln = {n: len(b.seqs[i]) for n, i in ix.items()}
    seq_chunk, kmer_off = qc.chunk_tables(b.bases, b.offsets, k)
    nch = {n: int(seq_chunk[i + 1] - seq_chunk[i]) for n, i in ix.items()}
    tot = {n: int(kmer_off[seq_chunk[i + 1]] - kmer_off[seq_chunk[i]]) for n, i in ix.items()}
    chunk_nk = np.diff(kmer_off)
    assert (ln["len-K"], tot["len-K"], ln["len-K+1"], tot["len-K+1"]) == (k, 1, k + 1, 2)
    assert (ln["one-chunk"], nch["one-chunk"], tot["one-chunk"]) == (C + k - 1, 1, C)
    assert (ln["chunk+1"], nch["chunk+1"], tot["chunk+1"]) == (C + k, 2, C + 1)
    assert int(chunk_nk[seq_chunk[ix["chunk+1"]] + 1]) == 1  # a second chunk of one k-mer
    assert (ln["three-chunks+5"], nch["three-chunks+5"], tot["three-chunks+5"]) == (3 * C + k + 5, 4, 3 * C + 6)
    assert nch["lane-max"] == qc.LANE_MAX and nch["lane-max+1"] == qc.LANE_MAX + 1 and tot["lane-max+1"] == qc.LANE_MAX * C + 1
    assert (ln["long-35-chunks"], nch["long-35-chunks"]) == (70_000, 35)
    assert ix["short-a"] + 1 == ix["long-35-chunks"] == ix["short-b"] - 1
    assert ln["short-a"] == ln["short-b"] == (40 if k <= 40 else k + 9) and nch["short-a"] == 1
    reads = [ix["read-%d" % i] for i in range(qc.N_READS)]
    assert reads == [i for i in range(reads[0], reads[0] + 301) if i != ix["parity"]] and all(len(b.seqs[i]) == k + 9 for i in reads)
    assert ix["parity"] == reads[0] + 150 and tot["parity"] == 1
    # ... so that the reads' sequence indices fall on every position of a wave and of a workgroup, and their flag segments start
    # at every offset relative to a 16-byte boundary
    run = reads + [ix["parity"]]  # 301 one-chunk sequences in a row
    assert {i % 64 for i in run} == set(range(64)) and {i % 256 for i in run} == set(range(256))
    assert {int(kmer_off[seq_chunk[i]]) % 16 for i in reads} == set(range(16))
    # N and lower case at the first base, the last base and mid-chunk: a skipped byte behind the first K costs one k-mer, lower case none
    clean = C + C // 2 + 1
    assert nch["N-first"] == 2 and b.seqs[ix["N-first"]][0] == ord("N") and tot["N-first"] == clean
    assert b.seqs[ix["N-last"]][-1] == ord("N") and tot["N-last"] == clean - 1
    assert b.seqs[ix["N-mid"]][C // 2 + 7] == ord("N") and tot["N-mid"] == clean - 1  # (it lies in chunk 0 alone)
    for n, at in (("lower-first", 0), ("lower-last", -1), ("lower-mid", C // 2 + 7)):
        assert chr(b.seqs[ix[n]][at]) in "acgt" and tot[n] == clean
    # a run of N longer than a chunk: chunk 1 of the sequence has no valid byte at all and keeps the one k-mer of its first K bytes,
    # inside a sequence whose other chunks have more
    c0 = int(seq_chunk[ix["N-run"]])
    run = b.seqs[ix["N-run"]]
    assert nch["N-run"] == 5 and set(run[C: 2 * C + k - 1]) == {ord("N")} and int(chunk_nk[c0 + 1]) == 1
    assert int(chunk_nk[c0]) > 1 and int(chunk_nk[c0 + 3]) == C and int(chunk_nk[c0 + 4]) == 301
    assert set(b.seqs[ix["all-N"]]) == {ord("N")} and ln["all-N"] == k + 20 and tot["all-N"] == 1
    assert b.names[-1] == "tail-read"
    assert int(kmer_off[-1]) <= 200_000


def test_constants_mirror_the_kernels():
    with open(os.path.join(ROOT, "cbl_amd", "csrc", "kernels_kmer.hpp")) as f:
        kk = f.read()
    with open(os.path.join(ROOT, "cbl_amd", "csrc", "common.hpp")) as f:
        cm = f.read()

    def const(text, name):
        return int(re.search(r"\b%s = (\d+)\b" % name, text).group(1))

    assert const(kk, "SEQ_TALLY_LANE_MAX") == qc.LANE_MAX and const(kk, "SEQ_TALLY_LONG_THREADS") == qc.LONG_THREADS
    assert const(cm, "CHUNK_KMERS") == qc.CHUNK_KMERS
    for kernel in ("k_chunk_tally", "k_seq_tally", "k_seq_tally_long"):
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kk), kernel


def test_header_declares_the_entry_points_under_abi_3():
    with open(os.path.join(ROOT, "include", "cblx.h")) as f:
        header = f.read()
    version_at = header.index("#define CBLX_ABI_VERSION 3")
    note = header[:version_at]
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert name in note, f"{name} is not named in the 'Added under 3' note in front of CBLX_ABI_VERSION"
        assert re.search(r"\bint %s\s*\(" % name, body), f"{name} is not declared"
    assert "src/cbl.rs:311-324" in header[header.index("cblx_contains_seqs_counts", version_at) - 2500:] and "examples/cbl.rs:205-228" in header


def test_bindings_and_methods_exist():
    for name in NEW:
        assert name in cbl_amd.SIGNATURES, name
        assert hasattr(cbl_amd.lib(), name), name
    for meth in ("contains_seqs_counts", "contains_seqs_counts_device", "query_fastx_file_counts", "matching_seqs"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth


def test_matching_rule_on_the_host():
    """positive >= max(min_hits, ceil(min_fraction * total)) with total > 0: a record without a k-mer never matches."""
    total = np.array([0, 0, 1, 10, 10, 10, 120, 120], dtype=np.uint32)
    positive = np.array([0, 5, 1, 4, 5, 6, 60, 59], dtype=np.uint32)
    assert cbl_amd.CBL.matching(total, positive, min_fraction=0.5).tolist() == [False, False, True, False, True, True, True, False]
    assert cbl_amd.CBL.matching(total, positive, min_fraction=0.0, min_hits=0).tolist() == [False, False, True, True, True, True, True, True]
    assert cbl_amd.CBL.matching(total, positive, min_fraction=0.0, min_hits=6).tolist() == [False, False, False, False, False, True, True, True]
    assert cbl_amd.CBL.matching(total, positive, min_fraction=1.0).tolist() == [False, False, True, False, False, False, False, False]


def test_cli_lists_per_record():
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "query", "--help"], capture_output=True, text=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0 and "--per-record" in r.stdout, r.stdout + r.stderr
