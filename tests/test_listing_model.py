"""tests/listing_model.py against itself, the CPU oracle and hand-made tables: the text line of a k-mer, the closed form of a Trie's
node count (what k_bucket_nodes computes), the `repartition` report. No GPU."""

import random

import numpy as np
import pytest

from cbl_amd import synth
from cbl_amd.__main__ import repartition_report as cli_report
from oracle import Oracle, pyref

import listing_model as lm  # tests/


def test_to_nucs_first_base_most_significant():
    assert lm.to_nucs(0b0001101100, 5) == b"ACTGA"  # codes 0 1 2 3 0
    assert lm.line(0b0001101100, 5) == b"ACTGA\n"
    k = 45  # 90 bits: bases on both sides of bit 64
    seq = bytes(random.Random(1).choice(b"ACTG") for _ in range(k))
    x = 0
    for b in seq:
        x = (x << 2) | b"ACTG".index(b)
    assert lm.to_nucs(x, k) == seq and x >> 64
    assert lm.text([x, x ^ 3], k) == seq + b"\n" + seq[:-1] + bytes([b"ACTG"[b"ACTG".index(seq[-1]) ^ 3]]) + b"\n"


@pytest.mark.parametrize("nbytes", [1, 2, 3, 6, 12, 13, 16])
def test_closed_form_equals_plain_count(nbytes):
    """nbytes + sum(nbytes - 1 - lcp) == 1 + number of distinct proper byte prefixes, on sets that share long prefixes and on random ones."""
    rng = random.Random(nbytes)
    top = 1 << (8 * nbytes)
    for trial in range(40):
        n = rng.choice((1, 2, 3, 50, 257))
        if trial % 2:  # clustered: few distinct values per byte, so that many prefixes are shared
            s = {sum(rng.choice((0, 1, 255)) << (8 * i) for i in range(nbytes)) for _ in range(n)}
        else:
            s = {rng.randrange(top) for _ in range(n)}
        s = sorted(s)
        assert lm.trie_nodes(s, nbytes) == lm.trie_nodes_plain(s, nbytes), (nbytes, s[:4])
    assert lm.trie_nodes([7], nbytes) == nbytes
    if nbytes == 1:  # one level: the root's bitvector holds every suffix
        assert lm.trie_nodes(list(range(256)), 1) == 1
    else:
        assert lm.trie_nodes([0, 1], nbytes) == nbytes and lm.trie_nodes([0, top - 1], nbytes) == 2 * nbytes - 1


# the read sets of test_index_shard_cuts_speculative_equals_sequential; (7, 4) adds two-byte suffixes. Suffix bytes: 3, 4, 6, 13, 2 —
# a Trie of one-byte suffixes cannot come out of an insertion (at most 256 suffixes, a Trie needs 1025), the model covers it above.
@pytest.mark.parametrize("k,pb,nreads,L,nbytes", [(9, 4, 1500, 100, 3), (15, 6, 1500, 150, 4), (31, 24, 3000, 150, 6), (59, 28, 400, 250, 13), (7, 4, 1500, 100, 2)])
def test_closed_form_equals_the_oracles_serialized_tries(k, pb, nreads, L, nbytes):
    """The node count parsed out of Oracle.serialize() — every Trie entry walked node by node — equals the closed form over the bucket's
    suffixes, and a Vec entry counts its words."""
    P = pyref.params(k, pb)
    sb = P["SB"]
    assert (sb + 7) // 8 == nbytes
    o = Oracle(k, pb)
    b, off = synth.reads(5, nreads, L)
    o.insert_seqs(b, off)
    by = {}
    for w in o.iter_words():
        by.setdefault(w >> sb, []).append(w & ((1 << sb) - 1))
    got = lm.serialized_bucket_nodes(o.serialize(), nbytes)
    assert [p for p, _, _, _ in got] == sorted(by)
    tries = 0
    for prefix, kind, length, nodes in got:
        assert length == len(by[prefix])
        assert nodes == lm.bucket_nodes(kind, by[prefix], nbytes), (prefix, kind, length)
        if kind == lm.TRIE:
            tries += 1
            assert nodes == lm.trie_nodes_plain(by[prefix], nbytes)
            assert by[prefix] == sorted(by[prefix])  # a Trie iterates ascending
    if pb <= 6:
        assert tries >= 1, "the shape was chosen for its Tries"


SINGLE = (4, [(3, 5, lm.VEC, 5)])
NO_TRIE = (6, [(0, 1, lm.VEC, 1), (5, 1, lm.VEC, 1), (9, 3, lm.VEC, 3), (63, 3, lm.VEC, 3)])
MIXED = (10, [(p, 1, lm.VEC, 1) for p in range(250)] + [(250, 2, lm.VEC, 2)] + [(p, 1100, lm.TRIE, 3000) for p in range(300, 348)]
         + [(400, 2000, lm.TRIE, 1000)])


def test_repartition_single_bucket():
    lines, out = lm.repartition_report(*SINGLE)
    assert lines == ["6.2% of the available prefixes are used", "The average bucket size is 5.0 items",
                     "100.0% of items are in a bucket of size ≤ 5 (100.0% of buckets)", "The biggest bucket (of size 5) corresponds to prefix 3",
                     "1 vecs, average node count = 5.0", "0 tries, average node count = NaN", "6 nodes in total"]
    assert out == "0.0625 1 5 3 5 1 5 0 0 6"


def test_repartition_without_a_trie_prints_nan_and_keeps_the_last_maximum():
    lines, out = lm.repartition_report(*NO_TRIE)
    assert lines == ["6.2% of the available prefixes are used", "The average bucket size is 2.0 items",
                     "25.0% of items are in a bucket of size ≤ 1 (50.0% of buckets)", "100.0% of items are in a bucket of size ≤ 3 (100.0% of buckets)",
                     "The biggest bucket (of size 3) corresponds to prefix 63", "4 vecs, average node count = 2.0", "0 tries, average node count = NaN",
                     "12 nodes in total"]
    assert out == "0.0625 4 8 63 3 4 8 0 0 12"


def test_repartition_thresholds_and_the_node_count_rule():
    """300 buckets: a size is reported when it holds more than total / 100 / 2 buckets (1) or items (275), or is the last one; the Trie
    of 2000 words with 1000 nodes counts as a "vec" (examples/cbl.rs:348 tests the node count)."""
    lines, out = lm.repartition_report(*MIXED)
    assert lines == ["29.3% of the available prefixes are used", "The average bucket size is 183.5 items",
                     "0.5% of items are in a bucket of size ≤ 1 (83.3% of buckets)", "96.4% of items are in a bucket of size ≤ 1100 (99.7% of buckets)",
                     "100.0% of items are in a bucket of size ≤ 2000 (100.0% of buckets)", "The biggest bucket (of size 2000) corresponds to prefix 400",
                     "252 vecs, average node count = 5.0", "48 tries, average node count = 3000.0", "145552 nodes in total"]
    assert out == "0.29296875 300 55052 400 2000 252 1252 48 144000 145552"


def test_repartition_of_an_empty_index_divides_by_nothing():
    assert lm.repartition_report(24, []) == (["0.0% of the available prefixes are used"], "0.0 0 0 0 0 0 0 0 0 0")


def test_the_cli_computes_the_models_report():
    rng = random.Random(3)
    tables = [SINGLE, NO_TRIE, MIXED, (24, [])]
    for _ in range(5):
        n = rng.randrange(1, 400)
        rows = []
        for p in sorted(rng.sample(range(1 << 12), n)):
            length = rng.choice((1, 2, 3, 7, 1024, 1025, 5000))
            rows.append((p, length, lm.VEC if length <= 1024 else lm.TRIE, length if length <= 1024 else rng.randrange(900, 20000)))
        tables.append((12, rows))
    for pb, rows in tables:
        prefix = np.array([r[0] for r in rows], dtype=np.uint32)
        length = np.array([r[1] for r in rows], dtype=np.uint32)
        nodes = np.array([r[3] for r in rows], dtype=np.uint64)
        assert cli_report(pb, prefix, length, nodes) == lm.repartition_report(pb, rows)
