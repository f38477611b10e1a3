"""CBL.at_least / CBL.occupancy on the GPU (cblx_set_at_least / cblx_occupancy_counts) against tests/threshold_model.py, byte for byte: the result AND
every operand after the operation. Operands are installed with `CBL.load(PyCBL(...).serialize())` from crafted bucket dicts, as
tests/test_gpu_setops_many.py does; tests/test_threshold_model.py shows on the CPU what the model is."""
import ctypes
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle.pyref import PyCBL, params  # noqa: E402

import setops_many_model as mm  # noqa: E402  (tests/)
import setops_model as sm  # noqa: E402  (tests/)
import threshold_model as tm  # noqa: E402  (tests/)

ROOT = Path(__file__).resolve().parent.parent
MANY_SMALL, MANY_LDS = tm.MANY_SMALL, tm.MANY_LDS  # kernels_setops.hpp (tests/test_threshold_model.py compares the values)
SORT_LDS = 4096  # kernels_setops.hpp SETOP_SORT_LDS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _gpu(m: PyCBL):
    g = cbl_amd.CBL(m.P["K"], m.P["PB"], canonical=m.canonical)
    g.load(m.serialize())
    return g


def _sb(k, pb):
    return params(k, pb)["SB"]


def _side(rng, kind, items):
    """kind: 'vec' = shuffled Vec, 'svec' = ascending Vec, 'trie'"""
    items = sorted(items)
    if kind == "vec":
        rng.shuffle(items)
    return ("trie" if kind == "trie" else "vec", items)


def _close(gs):
    for g in gs:
        g.close()


def _check(k, pb, canonical, bs, t, keep=False):
    """one at_least on crafted bucket dicts: result and every operand byte for byte, count, buckets, validate"""
    _need_gpu()
    ms = [sm.from_buckets(k, pb, canonical, b) for b in bs]
    gs = [_gpu(m) for m in ms]
    for g, m in zip(gs, ms):
        assert g.serialize() == m.serialize()  # as crafted, stored order included
    exp = tm.at_least(ms, t)
    d = cbl_amd.CBL.at_least(gs, t)
    assert d.count() == exp.count(), "t = %d" % t
    assert d.num_buckets() == len(exp.buckets)
    assert d.validate(False) == 0
    assert d.is_empty() == (exp.count() == 0)
    assert d.is_canonical() == canonical
    assert d.serialize() == exp.serialize(), "result, t = %d" % t
    for i, (g, m) in enumerate(zip(gs, ms)):
        assert g.serialize() == m.serialize(), "operand %d after at_least(t = %d)" % (i, t)
    if keep:
        return d, gs, exp, ms
    _close([d] + gs)


def _check_occupancy(k, pb, canonical, bs):
    """the histogram against the model, and every operand left as the model's merge leaves it"""
    _need_gpu()
    ms = [sm.from_buckets(k, pb, canonical, b) for b in bs]
    gs = [_gpu(m) for m in ms]
    want = tm.occupancy(ms)
    got = cbl_amd.CBL.occupancy(gs)
    assert got.dtype == np.uint64 and got.shape == (len(bs) + 1,)
    assert [int(v) for v in got] == want
    merged = [sm.from_buckets(k, pb, canonical, b) for b in bs]
    mm.merge(merged)
    for i, (g, m, mg) in enumerate(zip(gs, ms, merged)):
        assert g.serialize() == m.serialize() == mg.serialize(), "operand %d after occupancy" % i
        assert g.validate(False) == 0
    _close(gs)


def _thresholds(n):
    return sorted({1, 2, max(1, n - 1), n} & set(range(1, n + 1)))


# ---------------------------------------------------------------- 1: holder sets
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", [(31, 24), (59, 28)])
@pytest.mark.parametrize("n", [3, 5])
def test_holder_sets(n, k, pb, canonical):
    """one prefix per non-empty holder set and kind pattern, so prefixes with t - 1, t and t + 1 holders lie side by side: which are visited, which Vecs
    get sorted, clone-as-stored at t = 1"""
    sb, rng = _sb(k, pb), random.Random(k + pb + n)
    patterns = (("vec",) * n, ("svec",) * n, ("trie",) * n, tuple(("vec", "trie", "svec")[i % 3] for i in range(n)))
    bs, p = [dict() for _ in range(n)], 3
    for kinds in patterns:
        for holders in range(1, 1 << n):
            pool = sm.distinct(rng, 24, sb)
            for i in range(n):
                if (holders >> i) & 1:
                    bs[i][p] = _side(rng, kinds[i], rng.sample(pool, rng.randint(2, 14)))
            p += 5
    for t in _thresholds(n):
        _check(k, pb, canonical, bs, t)
    _check_occupancy(k, pb, canonical, bs)


# ---------------------------------------------------------------- 2: multiplicity edges
@pytest.mark.parametrize("t", [2, 3, 4])
def test_multiplicity_edges(t):
    k, pb, n = 31, 24, 4
    sb, rng = _sb(k, pb), random.Random(t)
    ones = (1 << sb) - 1
    v = sm.distinct(rng, 40, sb)
    bs = [dict() for _ in range(n)]

    def put(p, runs, kinds=("vec", "trie", "svec", "vec")):
        for i, run in enumerate(runs):
            if run is not None:
                bs[i][p] = _side(rng, kinds[i], run)

    # values held by exactly t - 1 and exactly t holders, among them suffix 0 and the all-ones suffix
    exact = {0: t - 1, ones: t}
    for j in range(8):
        exact[v[j]] = t - 1 if j % 2 else t
    runs = [[] for _ in range(n)]
    for x, c in exact.items():
        for i in rng.sample(range(n), c):
            runs[i].append(x)
    for i in range(n):
        runs[i].append(v[20 + i])  # nobody is empty
    put(10, runs)
    # a lowest copy that is not in the first run: the first run holds none of the qualifying values
    put(11, [[v[9]], [v[10], v[11]], [v[10], v[11], v[12]], [v[10], v[11], v[12]]])
    # a bucket whose result is empty at every t >= 2: it is dropped
    put(12, [[v[13]], [v[14]], [v[15]], [v[16]]])
    # a bucket where every value qualifies at every t
    put(13, [v[17:20]] * 4, kinds=("vec", "vec", "trie", "svec"))
    # three holders: not visited at t = 4
    put(14, [[v[1], v[2]], None, [v[2], v[1]], [v[2], v[3]]])
    d, gs, exp, ms = _check(k, pb, False, bs, t, keep=True)
    assert 12 not in exp.buckets and exp.buckets[13] == ["vec", sorted(v[17:20])]
    assert (14 in exp.buckets) == (t <= 3)
    if t == 4:
        assert ms[0].buckets[14] == ["vec", bs[0][14][1]]  # as stored
    _close([d] + gs)
    _check_occupancy(k, pb, False, bs)


# ---------------------------------------------------------------- 3: route edges
def _runs_of(rng, lens, sb, pattern):
    """ascending duplicate-free runs of exactly these lengths: 'nested' — every run a sample of the longest; 'windows' — overlapping windows of one pool;
    'disjoint'"""
    m = len(lens)
    if pattern == "nested":
        big = sm.distinct(rng, max(lens), sb)
        return [sorted(rng.sample(big, n)) for n in lens]
    if pattern == "disjoint":
        pool, out, at = sm.distinct(rng, sum(lens), sb), [], 0
        for n in lens:
            out.append(sorted(pool[at:at + n]))
            at += n
        return out
    pool = sm.distinct(rng, max(lens) + max(lens) // 2 + m, sb) + [0, (1 << sb) - 1]
    pool = sorted(set(pool))
    out = []
    for i, n in enumerate(lens):
        start = (i * len(pool) // (2 * m)) % max(1, len(pool) - n)
        out.append(pool[start:start + n] if i % 2 else sorted(rng.sample(pool, n)))
    return out


_EDGE_CACHE = {}


def _edge_buckets(k, pb):
    if (k, pb) not in _EDGE_CACHE:
        sb, rng = _sb(k, pb), random.Random(k * 11 + pb)
        bs, p = [dict() for _ in range(5)], 1
        for total in (MANY_SMALL - 1, MANY_SMALL, MANY_SMALL + 1, MANY_LDS - 1, MANY_LDS, MANY_LDS + 1):
            for holders in ((1, 3), (0, 2, 4), (0, 1, 2, 3, 4)):
                m = len(holders)
                for shape, pattern in (("even", "nested"), ("ones", "windows"), ("even", "windows"), ("ones", "disjoint")):
                    lens = [total // m] * m if shape == "even" else [1] * (m - 1) + [total - (m - 1)]
                    lens[0] += total - sum(lens)
                    runs = _runs_of(rng, lens, sb, pattern)
                    assert sum(map(len, runs)) == total
                    for i, run in zip(holders, runs):
                        bs[i][p] = _side(rng, rng.choice(["vec", "svec", "trie"]), run)
                    p += 3
        _EDGE_CACHE[(k, pb)] = bs
    return _EDGE_CACHE[(k, pb)]


@pytest.mark.parametrize("t", [1, 2, 3, 5, "occupancy"])
@pytest.mark.parametrize("k,pb", [(31, 24), (59, 28)])
def test_route_edges(k, pb, t):
    """words of all holders on either side of both thresholds, held by 2, 3 and 5 of five operands (t = 3 leaves the two-holder buckets unvisited)"""
    bs = _edge_buckets(k, pb)
    if t == "occupancy":
        _check_occupancy(k, pb, False, bs)
    else:
        _check(k, pb, False, bs, t)


# ---------------------------------------------------------------- 4: the long route
@pytest.mark.parametrize("k,pb", [(15, 6), (31, 3)])  # SUFFIX_BITS 24 and 65 (wide)
def test_long_route(k, pb):
    sb, rng = _sb(k, pb), random.Random(k)
    pool = sm.distinct(rng, 9000, sb)
    bs = [dict() for _ in range(5)]
    # prefix 1: every operand holds it, 10 700 words, one Vec side above SETOP_SORT_LDS (the huge sort), a run of one word
    for i, items in enumerate((pool[:5000], pool[2000:4500], pool[4000:4001], pool[3000:5200], pool[1000:4000])):
        bs[i][1] = _side(rng, ("vec", "trie", "vec", "svec", "vec")[i], items)
    assert len(bs[0][1][1]) > SORT_LDS
    # prefix 2: a long bucket two of the five hold — not visited at t = 3
    bs[1][2] = _side(rng, "vec", pool[:3000])
    bs[4][2] = _side(rng, "vec", pool[1500:4600])
    # prefix 3: three holders, a few thousand words, nothing shared by all three
    bs[0][3] = _side(rng, "trie", pool[:1500])
    bs[2][3] = _side(rng, "vec", pool[1000:2500])
    bs[3][3] = _side(rng, "vec", pool[2000:3500] + pool[:200])
    # prefix 4: short, beside the long ones
    for i in range(5):
        bs[i][4] = _side(rng, "vec", rng.sample(pool[:60], 30))
    for t in (2, 3, 5):
        d, gs, exp, ms = _check(k, pb, False, bs, t, keep=True)
        assert (2 in exp.buckets) == (t == 2)
        if t == 3:
            assert ms[1].buckets[2] == ["vec", bs[1][2][1]] and 3 not in exp.buckets  # as stored; and an empty long bucket is dropped
        _close([d] + gs)
    _check_occupancy(k, pb, False, bs)


@pytest.mark.parametrize("k,pb", [(15, 6), (31, 3)])  # SUFFIX_BITS 24 and 65 (wide)
def test_long_route_sixty_four_holders(k, pb):
    """2 560 words of 64 holders: a round stages 32 words of every run, and many rounds settle the bucket; one run of one word, one much longer"""
    sb, rng = _sb(k, pb), random.Random(pb)
    pool = sm.distinct(rng, 300, sb)
    bs = [{2: _side(rng, rng.choice(["vec", "trie"]), rng.sample(pool[:120], 40))} for _ in range(64)]
    bs[5][2] = _side(rng, "vec", pool[7:8])
    bs[40][2] = _side(rng, "trie", pool[60:300])
    assert sum(len(b[2][1]) for b in bs) > MANY_LDS
    for t in (2, 20, 64):
        _check(k, pb, False, bs, t)
    _check_occupancy(k, pb, False, bs)


# ---------------------------------------------------------------- 5: suffix widths and sentinel values
@pytest.mark.parametrize("k,pb", [(33, 10), (33, 9), (33, 8), (5, 8)])  # SUFFIX_BITS 63, 64, 65 and 6
def test_suffix_widths_and_sentinel_values(k, pb):
    sb = _sb(k, pb)
    assert sb == {(33, 10): 63, (33, 9): 64, (33, 8): 65, (5, 8): 6}[(k, pb)]
    ones, top = (1 << sb) - 1, 1 << (sb - 1)
    special = [0, 1, 2, 3, top - 1, top, top + 1, top | 2, ones - 1, ones] + ([1 << 63, (1 << 63) - 1, (1 << 64) - 1, 1 << 64] if sb > 64 else [])
    special = sorted(set(v for v in special if v <= ones))
    rng = random.Random(sb)
    bs, p = [{}, {}, {}, {}], 0
    for kinds in (("trie",) * 4, ("vec",) * 4, ("vec", "trie", "vec", "trie")):
        for sel in range(5):
            if sel == 0:
                runs = [list(special)] * 4
            elif sel == 1:
                runs = [special[::2], special[1::2], [0, ones], [ones]]
            elif sel == 2:
                runs = [[ones], [0, ones], [0, top, ones], [0, ones - 1, ones]]
            else:
                runs = [sorted(set(rng.sample(special, len(special) // 2 + 1)) | {0, ones}) for _ in range(4)]
            for i in range(4):
                bs[i][p] = (kinds[i], list(runs[i]) if kinds[i] == "trie" else list(runs[i])[::-1])
            p += 1
    top_p = (1 << pb) - 1
    for i in range(4):
        bs[i][top_p] = ("vec", [ones, 0]) if i % 2 else ("trie", [0, ones])
    for t in (2, 3, 4):
        _check(k, pb, False, bs, t)
    _check_occupancy(k, pb, False, bs)


# ---------------------------------------------------------------- 6: operand counts and empties
def _few(rng, sb, n, kind="vec"):
    items = sm.distinct(rng, n, sb)
    return (kind, sorted(items) if kind == "trie" else items)


def test_one_operand_is_a_clone():
    sb, rng = _sb(31, 24), random.Random(1)
    b = {3: _few(rng, sb, 5), 64: _few(rng, sb, 1), 65: _few(rng, sb, 30, "trie"), 1 << 20: _few(rng, sb, 1100)}
    d, gs, exp, ms = _check(31, 24, False, [b], 1, keep=True)
    assert d.serialize() == gs[0].serialize()  # as stored: unsorted Vecs, the Trie
    assert [int(v) for v in cbl_amd.CBL.occupancy(gs)] == [0, 1136] and gs[0].serialize() == ms[0].serialize()
    _close([d] + gs)


def test_two_operands():
    _need_gpu()
    import test_gpu_setops as t2  # the operands of its kind test: every pair of kinds and lengths on either side of the sort's limit

    ba, bb = t2._kind_buckets()
    for t in (1, 2):
        _check(31, 24, False, [ba, bb], t)
    _check_occupancy(31, 24, False, [ba, bb])


@pytest.mark.parametrize("t", [1, 32, 64])
def test_sixty_four_operands(t):
    sb, rng = _sb(31, 24), random.Random(64)
    pool = sm.distinct(rng, 40, sb)
    bs = []
    for i in range(64):
        b = {77: _side(rng, rng.choice(["vec", "trie"]), pool[:3] + rng.sample(pool[3:], rng.randint(1, 20)))}
        if i % 2:
            b[78] = _side(rng, "vec", rng.sample(pool, 3))  # 32 holders
        if i >= 33:
            b[79] = _side(rng, "vec", rng.sample(pool, 2))  # 31 holders
        bs.append(b)
    _check(31, 24, False, bs, t)
    if t == 32:
        _check_occupancy(31, 24, False, bs)


@pytest.mark.parametrize("shape", ["one_empty", "two_empty", "all_empty", "disjoint_prefixes"])
def test_empty_operands(shape):
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(sum(map(ord, shape)))
    some = {p: _few(rng, sb, n) for p, n in ((3, 5), (64, 1), (65, 30), (1 << 20, 1100))}
    back = {p: (kd, it[::-1]) for p, (kd, it) in some.items()}
    third = {p: _few(rng, sb, n) for p, n in ((3, 5), (67, 2), (1 << 22, 300))}
    bs = {"one_empty": [some, {}, back, third], "two_empty": [{}, some, {}, back], "all_empty": [{}, {}, {}],
          "disjoint_prefixes": [some, {p + 100: v for p, v in some.items()}, {p + 200: v for p, v in some.items()}]}[shape]
    live = sum(1 for b in bs if b)
    for t in range(1, len(bs) + 1):  # t on either side of the number of non-empty operands
        d, gs, exp, ms = _check(k, pb, False, bs, t, keep=True)
        if t > live or shape == "all_empty" or (shape == "disjoint_prefixes" and t >= 2):
            assert d.serialize() == bytes([0, 0]) and d.is_empty() and d.num_buckets() == 0
            assert [m.serialize() for m in ms] == [sm.from_buckets(k, pb, False, b).serialize() for b in bs]  # nothing was sorted
        _close([d] + gs)
    _check_occupancy(k, pb, False, bs)


# ---------------------------------------------------------------- 7: identities on the device
def test_identities_on_the_device():
    _need_gpu()
    bs = _edge_buckets(31, 24)
    n = len(bs)
    ms = [sm.from_buckets(31, 24, False, b) for b in bs]
    fresh = lambda: [_gpu(m) for m in ms]
    a, b = fresh(), fresh()
    x, y = cbl_amd.CBL.at_least(a, 1), cbl_amd.CBL.merge(b)
    assert x.serialize() == y.serialize() and [g.serialize() for g in a] == [g.serialize() for g in b]
    merged_operands = [g.serialize() for g in b]
    n_merge = y.count()
    _close([x, y] + a + b)
    a, b = fresh(), fresh()
    x, y = cbl_amd.CBL.at_least(a, n), cbl_amd.CBL.intersect(b)
    assert x.serialize() == y.serialize() and [g.serialize() for g in a] == [g.serialize() for g in b]
    n_inter = y.count()
    _close([x, y] + a + b)
    a = fresh()
    counts = [g.count() for g in a]
    pair = a[0].intersection_count(a[1])
    hist = [int(v) for v in cbl_amd.CBL.occupancy(a)]
    assert hist[0] == 0 and sum(j * h for j, h in enumerate(hist)) == sum(counts)
    assert sum(hist) == n_merge and hist[n] == n_inter
    assert [g.serialize() for g in a] == merged_operands  # left as a merge leaves them
    assert [int(v) for v in cbl_amd.CBL.occupancy(a[:2])][2] == pair
    for t in range(1, n + 1):
        d = cbl_amd.CBL.at_least(a, t)
        assert d.count() == sum(hist[t:])
        d.close()
    _close(a)


# ---------------------------------------------------------------- 8: errors
def test_errors_leave_every_context_alone():
    _need_gpu()
    rng = random.Random(1)
    sb = _sb(31, 24)
    mk = lambda canonical=False, k=31, pb=24: _gpu(sm.from_buckets(k, pb, canonical, {7: ("vec", sm.distinct(rng, 5, min(sb, _sb(k, pb))))}))
    a, b, c, d = mk(), mk(), mk(), mk()
    other_k, other_pb, canon = mk(k=33), mk(pb=20), mk(canonical=True)
    extra = [mk() for _ in range(65)]
    everything = [a, b, c, d, other_k, other_pb, canon] + extra
    before = [x.serialize() for x in everything]
    L = cbl_amd.lib()
    hist = (ctypes.c_uint64 * 70)()

    def refused(dst, srcs, t=1, n=None, msg=None, occupancy=True):
        arr = (ctypes.c_void_p * max(1, len(srcs)))(*[x._h if x is not None else None for x in srcs])
        rc = L.cblx_set_at_least(dst._h, arr, len(srcs) if n is None else n, t)
        assert rc == cbl_amd.EINVAL, rc
        if msg:
            assert msg in L.cblx_last_error(dst._h).decode()
        if occupancy:
            assert L.cblx_occupancy_counts(arr, len(srcs) if n is None else n, hist) == cbl_amd.EINVAL
        assert [g.serialize() for g in everything] == before

    refused(d, [])  # n == 0
    refused(d, extra)  # 65 valid contexts
    refused(d, [a, None, b])
    refused(d, [a, d, b], occupancy=False)  # dst among srcs
    refused(a, [a], occupancy=False)
    refused(d, [a, b, a])  # the same context twice
    for odd in (other_k, other_pb):
        refused(d, [a, odd, b])
        refused(odd, [a, b], occupancy=False)
    refused(d, [a, b, canon], msg="One of the index is canonical while the other isn't")
    refused(d, [canon, a], msg="One of the index is canonical while the other isn't")
    for t in (0, 4, 65, 1 << 31):  # the threshold out of range
        refused(d, [a, b, c], t=t, occupancy=False)
    assert L.cblx_occupancy_counts((ctypes.c_void_p * 2)(a._h, b._h), 2, None) == cbl_amd.EINVAL
    with pytest.raises(ValueError):
        cbl_amd.CBL.at_least([a, b], 3)
    with pytest.raises(cbl_amd.CblxError) as e:
        cbl_amd.CBL.at_least([a, canon], 1, out=d)
    assert e.value.code == cbl_amd.EINVAL and "canonical" in str(e.value)
    with pytest.raises(cbl_amd.CblxError):
        cbl_amd.CBL.occupancy([a, other_k])
    assert [g.serialize() for g in everything] == before
    out = cbl_amd.CBL.at_least([a, b, c], 1, out=d)  # `out` is overwritten
    assert out is d and d.count() == 15 and d.num_buckets() == 1
    out = cbl_amd.CBL.at_least(extra[:64], 2, out=d)
    assert out is d and d.is_empty()
    _close(everything)


# ---------------------------------------------------------------- 9: the result is a first-class index
@pytest.mark.parametrize("k,pb", [(15, 6), (31, 3)])  # SUFFIX_BITS 24 and 65 (wide)
def test_result_is_a_first_class_index(k, pb, tmp_path):
    import test_gpu_setops as t2

    G, words, ba, bb, shared = t2.first_class_operands(k, pb)
    rng = random.Random(pb)
    bc = {p: ("vec", rng.sample(it, len(it))) for p, (_, it) in ba.items()}  # a's sets as shuffled Vecs: a third operand
    d, gs, exp, ms = _check(k, pb, False, [ba, bb, bc], 2, keep=True)
    assert sm.words(exp) == sm.words(ms[0]) and all(v[0] == "vec" for v in exp.buckets.values())  # held by a and c, or by all three
    piece = bytes(G[100:400])
    d.insert_seq(piece)
    exp.insert_seq(piece)
    assert d.count() == exp.count() and d.serialize() == exp.serialize() and d.validate(False) == 0
    path = str(tmp_path / "at_least.cbl")
    d.save_to_file(path)
    again = cbl_amd.CBL.load_from_file(path, k, pb)
    assert again.serialize() == exp.serialize()
    u = cbl_amd.CBL.at_least([gs[1], again, gs[0]], 3)  # ... and as an operand
    mu = tm.at_least([ms[1], exp, ms[0]], 3)
    assert u.serialize() == mu.serialize() and again.serialize() == exp.serialize() and gs[1].serialize() == ms[1].serialize()
    _close([d, again, u] + gs)


# ---------------------------------------------------------------- 10: real k-mers
@pytest.mark.parametrize("k,pb,canonical", [(31, 24, False), (31, 24, True), (59, 28, False), (59, 28, True)])
def test_real_kmers(k, pb, canonical):
    _need_gpu()
    import test_gpu_setops as t2
    from collections import Counter

    seqs = t2._split_reads(78, 2000, 80)
    parts = [seqs[:1000], seqs[400:1400], seqs[800:1800], seqs[900:]]  # four overlapping read sets
    ms = [PyCBL(k, pb, canonical) for _ in parts]
    for m, ss in zip(ms, parts):
        for s in ss:
            m.insert_seq(s)
    sets = [sm.words(m) for m in ms]
    held = Counter(w for s in sets for w in s)
    blobs = [m.serialize() for m in ms]

    def fresh():
        out = []
        for blob in blobs:
            g = cbl_amd.CBL(k, pb, canonical=canonical)
            g.load(blob)
            out.append(g)
        return out

    for t in (2, 3):
        xs = [sm.from_buckets(k, pb, canonical, {p: (kd, it) for p, (kd, it) in m.buckets.items()}) for m in ms]
        gs = fresh()
        exp = tm.at_least(xs, t)
        d = cbl_amd.CBL.at_least(gs, t)
        want = {w for w, c in held.items() if c >= t}
        assert want and sm.words(exp) == want
        assert d.count() == len(want) and d.num_buckets() == len(exp.buckets) and d.validate(False) == 0
        assert d.serialize() == exp.serialize()
        for g, m in zip(gs, xs):
            assert g.serialize() == m.serialize()
        _close([d] + gs)
    gs = fresh()
    assert [int(v) for v in cbl_amd.CBL.occupancy(gs)] == [sum(1 for c in held.values() if c == j) for j in range(5)]
    _close(gs)


# ---------------------------------------------------------------- 11: seeded sweep
@pytest.mark.parametrize("seed", range(12))
def test_seeded_sweep(seed):
    rng = random.Random(seed)
    k, pb = rng.choice([11, 31, 33, 59]), rng.choice([6, 12, 16])
    sb, canonical = _sb(k, pb), rng.random() < 0.5
    n = rng.randint(2, 7)
    bs = [dict() for _ in range(n)]
    for p in rng.sample(range(1 << pb), rng.randint(1, min(12, 1 << pb))):
        holders = [i for i in range(n) if rng.random() < 0.7] or [rng.randrange(n)]
        share = rng.choice([0.0, 0.3, 1.0])
        common = sm.distinct(rng, min(rng.choice([1, 3, 40, 300]), (1 << sb) // 4), sb)
        for i in holders:
            own = min(rng.choice([0, 1, 3, 40, 400, 1500]), (1 << sb) // 4)
            items = set(rng.sample(common, max(1, int(share * len(common))))) | set(sm.distinct(rng, own, sb))
            bs[i][p] = _side(rng, rng.choice(["vec", "svec", "trie"]), items)
    _check(k, pb, canonical, bs, rng.randint(2, n))
    _check_occupancy(k, pb, canonical, bs)


# ---------------------------------------------------------------- 12: the CLI
def test_cli(tmp_path):
    _need_gpu()
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(11)
    pool = sm.distinct(rng, 60, sb)
    bs = [{p: _side(rng, kind, rng.sample(pool, 20)) for p in ps} for ps, kind in (((1, 2, 3), "vec"), ((2, 3, 4), "trie"), ((2, 3, 5), "vec"))]
    ms = [sm.from_buckets(k, pb, False, b) for b in bs]
    paths = []
    for i, m in enumerate(ms):
        paths.append(str(tmp_path / ("in%d.cbl" % i)))
        Path(paths[-1]).write_bytes(m.serialize())
    out = str(tmp_path / "out.cbl")
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    base = [sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb)]
    run = lambda args: subprocess.run(base + args, cwd=str(ROOT), env=env, capture_output=True, text=True, timeout=300)
    r = run(["at-least", "-t", "2"] + paths + ["-o", out])
    assert r.returncode == 0, r.stderr
    assert "Writing the index to " + out in r.stderr
    exp = tm.at_least([sm.from_buckets(k, pb, False, b) for b in bs], 2)
    assert Path(out).read_bytes() == exp.serialize() and ("%d 31-mers are held by at least 2 of the 3 indexes" % exp.count()) in r.stderr
    r = run(["occupancy"] + paths)
    assert r.returncode == 0, r.stderr
    hist = tm.occupancy(ms)
    assert r.stdout.splitlines() == ["%d\t%d" % (j, hist[j]) for j in (1, 2, 3)]
    r = run(["at-least", "-t", "4"] + paths)
    assert r.returncode != 0 and "threshold" in r.stderr
    r = run(["occupancy", paths[0]])
    assert r.returncode != 0 and "two or more" in r.stderr
