"""The panel query on the CPU: the numpy model of the mask tallies (tests/panel_query_model.py) held against a direct per-index count from the
oracle, CBL.classify and classify_report on hand-made tables, and the new names where the sources, the header and the bindings carry them."""
import os
import re

import numpy as np
import pytest

import cbl_amd
from cbl_amd.__main__ import classify_report
from oracle import Oracle

import panel_query_model as pm
import query_counts_shapes as qc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cblx_contains_seqs_counts_many", "cblx_contains_seqs_counts_many_device")
KERNELS = ("k_panel_join", "k_mask_or_flags", "k_chunk_tally_mask", "k_seq_tally_mask", "k_seq_tally_long_mask")


def _panel_oracles(b, k, pb, canonical, n):
    """n indexes from different overlapping parts of the batch's resident sequences (index j: every sequence whose position is not j mod n + 1)."""
    res = qc.resident_seqs(b)
    out = []
    for j in range(n):
        o = Oracle(k, pb, canonical)
        o.insert_seqs(*qc.as_arrays([s for i, s in enumerate(res) if i % (n + 1) != j]))
        out.append(o)
    return out


@pytest.mark.parametrize("k,pb,canonical", [(31, 24, False), (11, 8, True)])
def test_mask_tallies_match_a_direct_count(k, pb, canonical):
    b = qc.batch(k)
    n = 3
    oracles = _panel_oracles(b, k, pb, canonical, n)
    # the direct count: per sequence and per index, straight from the oracle
    direct_total, direct_pos, flags = [], [[] for _ in range(n)], [[] for _ in range(n)]
    for s in b.seqs:
        words = oracles[0].seq_words(s)
        direct_total.append(len(words))
        for j, o in enumerate(oracles):
            f = [o.contains_word(w) for w in words]
            direct_pos[j].append(sum(f))
            flags[j] += f
    want = pm.expect(oracles, b.seqs)
    assert np.array_equal(want.total, np.array(direct_total, dtype=np.uint32))
    assert np.array_equal(want.positive, np.array(direct_pos, dtype=np.uint32))
    assert np.array_equal(want.flags, np.array(flags, dtype=bool))
    assert 0 < int(want.positive.sum()) < n * int(want.total.sum()) and len({tuple(r) for r in want.positive.tolist()}) == n  # the rows differ
    # the model of the device's two levels, ballot transpose included
    seq_chunk, kmer_off = qc.chunk_tables(b.bases, b.offsets.astype(np.int64), k)
    total, positive = pm.tallies_from_masks(want.mask, kmer_off, seq_chunk, n)
    assert np.array_equal(total, want.total) and np.array_equal(positive, want.positive)
    counts = np.diff(kmer_off)
    assert (counts % pm.WAVE != 0).any() and (counts > pm.WAVE).any() and (counts < pm.WAVE).any()  # short last rounds, several rounds, one short round
    assert (np.diff(seq_chunk) > qc.LANE_MAX).any()  # the workgroup route of a long sequence


def test_ballot_transpose_on_a_full_width_panel():
    """64 indexes, masks with every bit in use: bit 63, the 31 / 32 edge, a chunk of 64 + 1 words."""
    rng = np.random.default_rng(5)
    kmer_off = np.array([0, 1, 65, 130, 258, 259], dtype=np.int64)
    seq_chunk = np.array([0, 1, 3, 5], dtype=np.int64)
    mask = rng.integers(0, 1 << 63, size=int(kmer_off[-1]), dtype=np.uint64) | (rng.integers(0, 2, size=int(kmer_off[-1]), dtype=np.uint64) << np.uint64(63))
    for n in (1, 31, 32, 33, 64):
        cp = pm.chunk_tally_mask(mask, kmer_off, n)
        bits = ((mask[None, :] >> np.arange(n, dtype=np.uint64)[:, None]) & np.uint64(1)).astype(np.int64)  # [n, nk]
        run = np.concatenate([np.zeros((n, 1), dtype=np.int64), np.cumsum(bits, axis=1)], axis=1)
        assert np.array_equal(cp.T, run[:, kmer_off[1:]] - run[:, kmer_off[:-1]]), n
        pos = pm.seq_tally_mask(cp, seq_chunk)
        assert np.array_equal(pos.astype(np.int64), run[:, kmer_off[seq_chunk[1:]]] - run[:, kmer_off[seq_chunk[:-1]]]), n


def test_classify_on_hand_made_tables():
    total = np.array([10, 10, 0, 10, 10, 10, 120], dtype=np.uint32)
    positive = np.array([[5, 7, 0, 4, 6, 9, 60],
                         [5, 9, 0, 4, 2, 9, 61],
                         [1, 9, 3, 4, 6, 3, 59]], dtype=np.uint32)
    #                    tie 0/1 -> 0; tie 1/2 -> 1; total 0 -> -1; nobody reaches 5 -> -1; tie 0/2 -> 0; tie 0/1 -> 0; 61 of 120 -> 1
    got = cbl_amd.CBL.classify(total, positive)
    assert got.dtype == np.int64 and got.tolist() == [0, 1, -1, -1, 0, 0, 1]
    assert np.array_equal(got, pm.classify_model(total, positive))
    # min_hits decides: with a fraction of 0 every index with total > 0 passes, min_hits then drops the weak rows
    assert cbl_amd.CBL.classify(total, positive, min_fraction=0.0).tolist() == [0, 1, -1, 0, 0, 0, 1]
    assert cbl_amd.CBL.classify(total, positive, min_fraction=0.0, min_hits=8).tolist() == [-1, 1, -1, -1, -1, 0, 1]
    assert cbl_amd.CBL.classify(total, positive, min_fraction=0.0, min_hits=62).tolist() == [-1] * 7
    assert cbl_amd.CBL.classify(total, positive, min_fraction=1.0).tolist() == [-1] * 7
    for frac, hits in ((0.5, 0), (0.0, 0), (0.0, 8), (0.3, 5), (1.0, 0)):
        assert np.array_equal(cbl_amd.CBL.classify(total, positive, min_fraction=frac, min_hits=hits), pm.classify_model(total, positive, frac, hits)), (frac, hits)
    # each row is judged by CBL.matching on its own
    for j in range(3):
        alone = cbl_amd.CBL.classify(total, positive[j: j + 1])
        assert np.array_equal(alone >= 0, cbl_amd.CBL.matching(total, positive[j]))
    assert cbl_amd.CBL.classify(np.zeros(0, dtype=np.uint32), np.zeros((2, 0), dtype=np.uint32)).tolist() == []


def test_classify_report():
    total = [10, 10, 0, 7]
    positive = [[5, 2, 0, 7], [1, 9, 0, 7]]
    lines, summary, human = classify_report(total, positive, [0, 1, -1, 0])
    assert lines == ["0\t10\t5\t1\t0", "1\t10\t2\t9\t1", "2\t0\t0\t0\t-", "3\t7\t7\t7\t0"]
    assert summary == ["0\t2", "1\t1", "unassigned\t1"]
    assert human[0] == "4 records against 2 indexes: 3 assigned, 1 unassigned" and len(human) == 3
    lines, summary, _ = classify_report([], [[], [], []], [])
    assert lines == [] and summary == ["0\t0", "1\t0", "2\t0", "unassigned\t0"]
    with pytest.raises(ValueError):
        classify_report(total, positive, [0, 2, -1, 0])  # an index the panel does not have
    with pytest.raises(ValueError):
        classify_report(total, [[1, 2, 3]], [0, 0, 0, 0])


def test_bindings_header_and_kernels_carry_the_new_names():
    for name in NEW:
        assert name in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES[name][1]) == 11, name
        assert hasattr(cbl_amd.lib(), name), name
    with open(os.path.join(ROOT, "include", "cblx.h")) as f:
        header = f.read()
    note = header[: header.index("#define CBLX_ABI_VERSION 3")]
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\b(?!_)" % name, note), f"{name} is not named in the 'Added under 3' note in front of CBLX_ABI_VERSION"
        assert re.search(r"\bint %s\s*\(" % name, body), f"{name} is not declared"
    with open(os.path.join(ROOT, "cbl_amd", "csrc", "kernels_kmer.hpp")) as f:
        kk = f.read()
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kk), kernel
    for meth in ("contains_seqs_counts_many", "contains_seqs_counts_many_device", "classify"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
