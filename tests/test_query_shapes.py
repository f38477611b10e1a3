"""What tests/query_shapes.py delivers for every parameter set of tests/test_gpu_query_classes.py, checked on the CPU: every named
bucket length with its kind, hits and misses in every targeted bucket, keys on both borders. A change of seed or genome size that
drops a class fails here, without a GPU."""
import os
import re

import pytest

import query_shapes as qs
from oracle import pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ALL12 = (1, 8, 9, 1024, 1025, 2729, 2730, 2731, 4094, 4095, 4096, 4097)
# name -> (SB, WB, lengths delivered, lengths with an "outer" bucket: hits on the first and the last element); the "-b" rounds
# serve "outer" buckets first, every other shape gives each length an "inner" bucket
EDGE_REACH = {
    "15-6": (29, 35, ALL12, ALL12[3:]),
    "31-5": (63, 68, ALL12, ()),
    "31-4-a": (64, 68, (1, 9, 1025, 2731, 4095, 4096), ()),
    "31-4-b": (64, 68, (8, 1024, 2730, 4094, 4097), (8, 1024, 2730, 4094, 4097)),
    "31-3-a": (65, 68, (9, 1025, 4095, 4096), ()),
    "31-3-b": (65, 68, (8, 1024, 4094, 4097), (8, 1024, 4094, 4097)),
    "33-16": (57, 73, ALL12, ALL12),
    "45-6": (91, 97, ALL12, ALL12[4:]),
    "15-6-canonical": (29, 35, ALL12, (9,) + ALL12[4:]),
}


def _check_buckets(s, kind_of):
    """Every bucket holds exactly its length of distinct words of its prefix; the genome queries it with hits, with misses between
    its elements, and on both borders: misses below the first and above the last element ("inner"), hits on them ("outer")."""
    rs = set(s.resident)
    assert len(rs) == len(s.resident) == sum(b.length for b in s.buckets.values())
    seen = {}
    for w, f in zip(s.words, s.expected.tolist()):
        assert f == (w in rs)
        seen.setdefault(w >> s.sb, set()).add(w)
    for p, b in s.buckets.items():
        assert b.prefix == p and len(b.elements) == b.length and b.kind == kind_of(b.length)
        assert b.elements == sorted(set(b.elements)) and b.candidates == sorted(seen[p])
        assert all(w >> s.sb == p and w in rs for w in b.elements) and set(b.elements) <= seen[p]
        misses = [w for w in b.candidates if w not in rs]
        assert misses and len(misses) + b.length == len(b.candidates)
        lo, hi, clo, chi = qs.border_words(b)
        if b.edges == "inner":
            assert clo < lo and chi > hi and clo not in rs and chi not in rs  # a key below the first, one above the last element
        else:
            assert clo == lo and clo in rs and (b.length == 1 or (chi == hi and chi in rs))
        if b.length >= 2:
            assert any(lo < w < hi for w in misses)  # and one between them
    assert s.expected.any() and not s.expected.all()
    return set(seen) - set(s.buckets)  # prefixes that are queried and have no bucket


@pytest.mark.parametrize("name", list(qs.EDGE_SHAPES))
def test_edge_shapes_deliver_every_named_length(name):
    spec = qs.EDGE_SHAPES[name]
    sb, wb, lengths, outer = EDGE_REACH[name]
    k, pb, canonical = spec[:3]
    P = pyref.params(k, pb)
    assert (P["SB"], P["WB"]) == (sb, wb)
    s = qs.shape(spec)
    assert (s.k, s.pb, s.canonical, s.sb) == (k, pb, canonical, sb)
    got = qs.delivered(s)
    assert tuple(sorted(got)) == lengths == tuple(sorted(spec[3]))
    assert all(("outer" if name.endswith("-b") else "inner") in got[n] for n in lengths)
    assert tuple(n for n in lengths if "outer" in got[n]) == outer
    unserved = _check_buckets(s, qs.batch_kind)
    assert unserved or name.startswith("31-3")  # queries that miss the directory (K = 31 at 3 prefix bits fills four prefixes, all taken)
    assert all(b.kind == (qs.VEC if b.length <= 1024 else qs.TRIE) for b in s.buckets.values())
    assert len(s.words) <= 200_000
    # the order CBL::iter must give: every resident word once, a Vec as inserted, a Trie ascending
    it = qs.iteration_order(s)
    assert sorted(it) == sorted(s.resident) and [w >> s.sb for w in it] == sorted(w >> s.sb for w in it)
    for b in s.buckets.values():
        mine = [w for w in it if w >> s.sb == b.prefix]
        assert sorted(mine) == b.elements and (b.kind == qs.VEC or mine == b.elements)
        assert mine == [w for w in s.resident if w >> s.sb == b.prefix] or b.kind == qs.TRIE
    assert any(b.kind == qs.VEC and b.length > 8 and b.elements != [w for w in it if w >> s.sb == b.prefix] for b in s.buckets.values())


def test_edge_shapes_reach_every_length_in_every_suffix_class():
    """Between their rounds the shapes with few populated prefixes reach what their class logic tells apart: 8 / 9 and 1024 / 1025
    (k_contains, Vec or Trie) and the table's capacity 4095 / 4096 everywhere; 2730 / 2731 where the `full` table is excluded by
    SB >= 64 only as lengths that must not matter."""
    reach = {}
    for name, (sb, _, lengths, _) in EDGE_REACH.items():
        reach.setdefault(sb, set()).update(lengths)
    assert reach[29] == reach[63] == reach[57] == reach[91] == set(ALL12)
    assert reach[64] >= {1, 8, 9, 1024, 1025, 2730, 2731, 4094, 4095, 4096, 4097}
    assert reach[65] == {8, 9, 1024, 1025, 4094, 4095, 4096, 4097}


def test_short_trie_shape_delivers_every_length():
    s = qs.shape(qs.SHORT_TRIE_SHAPE, ascending=True, kind_of=lambda n: qs.TRIE)
    got = qs.delivered(s)
    assert sorted(got) == list(range(1, 101)) + [728, 729, 730, 1023]
    assert all(sorted(v) == ["inner", "outer"] for v in got.values())
    assert s.resident == sorted(s.resident)  # ascending inserts leave every Vec ascending: installed as Tries
    assert _check_buckets(s, lambda n: qs.TRIE)
    assert sum(len(b.candidates) for b in s.buckets.values()) <= 200_000


@pytest.mark.parametrize("name", list(qs.MERGE_SHAPES))
def test_merge_shapes_split_into_shares_of_vec_size(name):
    spec = qs.MERGE_SHAPES[name]
    s = qs.shape(spec)
    assert pyref.params(*spec[:2])["SB"] == {"15-6": 29, "35-6": 71}[name]
    assert {n: sorted(v) for n, v in qs.delivered(s).items()} == {4500: ["inner", "outer"], 2500: ["inner", "outer"]}
    assert _check_buckets(s, qs.batch_kind)
    sh = qs.shares(s, qs.MERGE_SHARES)
    assert len(sh) == 5 and sorted(w for part in sh for w in part) == sorted(s.resident)
    for part in sh:
        per = {}
        for w in part:
            per[w >> s.sb] = per.get(w >> s.sb, 0) + 1
        assert set(per) == set(s.buckets) and max(per.values()) <= 1024  # every share's buckets are Vecs
    # `|=` appends what is new, ascending, behind self's sorted elements: the last share interleaves with the others
    for p, b in s.buckets.items():
        last = [w for w in sh[-1] if w >> s.sb == p]
        rest = [w for part in sh[:-1] for w in part if w >> s.sb == p]
        assert min(last) < max(rest)


@pytest.mark.parametrize("k,pb", qs.ONE_ABSENT)
def test_one_absent_sequences(k, pb):
    n = qs.ONE_ABSENT_KMERS
    assert n > 2 * 2048 and qs.ONE_ABSENT_AT == (0, n - 1, 2047, 2048, None)
    for absent in qs.ONE_ABSENT_AT:
        seq, words, resident = qs.all_but_one(k, pb, n, 1000 * k + pb, absent)
        assert len(seq) == n + k - 1 and len(resident) == n - (absent is not None)
        if absent is not None:
            assert words[absent] not in resident


def test_constants_mirror_the_kernels():
    def src(name):
        with open(os.path.join(ROOT, "cbl_amd", "csrc", name)) as f:
            return f.read()

    def const(text, name):
        return int(re.search(r"\b%s = (\d+)\b" % name, text).group(1))

    kb, kk, cm = src("kernels_bucket.hpp"), src("kernels_kmer.hpp"), src("common.hpp")
    assert const(kb, "QL") == qs.QL and qs.QL1 == qs.QL + 1 and "(QL + 1u)" in kb
    assert const(cm, "VEC_THRESHOLD") == qs.THRESHOLD
    assert const(kk, "JOIN_FULL_MAX") == qs.JOIN_FULL_MAX and const(kk, "JOIN_TAB_MAX") == qs.JOIN_TAB_MAX
    assert const(cm, "CHUNK_KMERS") == 2048
    assert qs.EDGE_LENGTHS == ALL12
    assert (const(kb, "KIND_VEC"), const(kb, "KIND_TRIE")) == (qs.VEC, qs.TRIE)
