"""CBL.merge / CBL.intersect of many indexes on the GPU (cblx_set_op_many) against tests/setops_many_model.py, byte for byte: the result AND every
operand after the operation (merge sorts the Vec buckets of the holders of a prefix two or more hold, intersect those of every operand on the prefixes
all hold). Operands are installed with `CBL.load(PyCBL(...).serialize())` from crafted bucket dicts, as tests/test_gpu_setops.py does;
tests/test_setops_many_model.py shows on the CPU what the model is and that it is no fold of the binary operation."""
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
from cbl_amd import synth  # noqa: E402
from oracle import Oracle  # noqa: E402
from oracle.pyref import PyCBL, params  # noqa: E402

import setops_many_model as mm  # noqa: E402  (tests/)
import setops_model as sm  # noqa: E402  (tests/)

ROOT = Path(__file__).resolve().parent.parent
OPS = ("or", "and")
MANY_SMALL, MANY_LDS = mm.MANY_SMALL, mm.MANY_LDS  # kernels_setops.hpp (tests/test_setops_many_model.py compares the values)
SORT_LDS = 4096  # kernels_setops.hpp SETOP_SORT_LDS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _gpu(m: PyCBL):
    g = cbl_amd.CBL(m.P["K"], m.P["PB"], canonical=m.canonical)
    g.load(m.serialize())
    return g


def _run(op, gs, out=None):
    return cbl_amd.CBL.merge(gs, out=out) if op == "or" else cbl_amd.CBL.intersect(gs, out=out)


def _check(k, pb, canonical, bs, op, keep=False):
    """one operation on crafted bucket dicts: result and every operand byte for byte, count, buckets, validate"""
    _need_gpu()
    ms = [sm.from_buckets(k, pb, canonical, b) for b in bs]
    gs = [_gpu(m) for m in ms]
    for g, m in zip(gs, ms):
        assert g.serialize() == m.serialize()  # as crafted, stored order included
    exp = mm.MANY[op](ms)
    d = _run(op, gs)
    assert d.count() == exp.count()
    assert d.num_buckets() == len(exp.buckets)
    assert d.validate(False) == 0
    assert d.is_empty() == (exp.count() == 0)
    assert d.is_canonical() == canonical
    assert d.serialize() == exp.serialize(), "result"
    for i, (g, m) in enumerate(zip(gs, ms)):
        assert g.serialize() == m.serialize(), "operand %d after the operation" % i
    if keep:
        return d, gs, exp, ms
    for g in [d] + gs:
        g.close()


def _sb(k, pb):
    return params(k, pb)["SB"]


def _side(rng, kind, items):
    """kind: 'vec' = shuffled Vec, 'svec' = ascending Vec, 'trie'"""
    items = sorted(items)
    if kind == "vec":
        rng.shuffle(items)
    return ("trie" if kind == "trie" else "vec", items)


# ---------------------------------------------------------------- 1: holder sets
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", [(31, 24), (59, 28)])
def test_holder_sets(op, k, pb, canonical):
    """three operands, one prefix per non-empty holder set and kind pattern: clone-as-stored (Trie kept, unsorted Vec kept), which Vecs get sorted"""
    sb, rng = _sb(k, pb), random.Random(k + pb)
    bs, p = [{}, {}, {}], 3
    for kinds in (("vec",) * 3, ("svec",) * 3, ("trie",) * 3, ("vec", "trie", "svec"), ("trie", "vec", "vec")):
        for holders in range(1, 8):
            pool = sm.distinct(rng, 30, sb)
            for i in range(3):
                if (holders >> i) & 1:
                    bs[i][p] = _side(rng, kinds[i], rng.sample(pool, rng.randint(2, 14)))
            p += 5
    _check(k, pb, canonical, bs, op)


# ---------------------------------------------------------------- 2: n = 2 is cblx_set_op
@pytest.mark.parametrize("op", OPS)
def test_two_operands_equal_set_op(op):
    _need_gpu()
    import test_gpu_setops as t2  # the operands of its kind test: every pair of kinds and lengths on either side of the sort's limit

    ba, bb = t2._kind_buckets()
    ms = [sm.from_buckets(31, 24, False, b) for b in (ba, bb)]
    g_many, g_two = [_gpu(m) for m in ms], [_gpu(m) for m in ms]
    d_many, d_two = _run(op, g_many), cbl_amd.CBL.set_op(g_two[0], g_two[1], op)
    exp = mm.MANY[op](ms)
    assert d_many.serialize() == d_two.serialize() == exp.serialize()
    for a, b, m in zip(g_many, g_two, ms):
        assert a.serialize() == b.serialize() == m.serialize()
    for g in [d_many, d_two] + g_many + g_two:
        g.close()


# ---------------------------------------------------------------- 3: short-route edges
def _split(total, m, shape, rng):
    """m run lengths that sum to `total`"""
    if shape == "even":
        lens = [total // m] * m
        lens[0] += total - sum(lens)
    elif shape == "ones":  # runs of one word, one run with nearly everything
        lens = [1] * (m - 1) + [total - (m - 1)]
    else:  # the big run first, a run of one last
        lens = [total - 2 * (m - 1) + 1] + [2] * (m - 2) + [1]
    assert sum(lens) == total and all(x >= 1 for x in lens), (total, m, shape, lens)
    return lens


def _runs_with_pattern(rng, lens, pattern, sb):
    """ascending duplicate-free runs of the given lengths"""
    m, mn = len(lens), min(lens)
    if pattern == "all_shared":  # every run is a prefix-free sample of the longest: the shortest is inside all others only when nested
        big = sorted(sm.distinct(rng, max(lens), sb))
        order = sorted(range(m), key=lambda i: -lens[i])
        runs, cur = [None] * m, big
        for i in order:
            cur = sorted(rng.sample(cur, lens[i]))
            runs[i] = cur
        return runs
    pool = sm.distinct(rng, sum(lens), sb)
    runs, at = [], 0
    for n in lens:
        runs.append(pool[at:at + n])
        at += n
    if pattern == "none_shared":
        return [sorted(r) for r in runs]
    if pattern == "multiplicities":  # value j of the shortest run is held by 1 + j % m runs, a rotating window of holders; {0, 2} only when m >= 3
        for j in range(mn):
            v = runs[0][j]
            for t in range(1, 1 + j % m):
                runs[(j + t) % m][j % len(runs[(j + t) % m])] = v
        if m >= 3 and len(runs[2]) >= 1:
            runs[2][-1] = runs[0][0] if lens[0] > 1 else runs[2][-1]
        return [sorted(set(r)) for r in runs]
    assert pattern == "ends"  # equal values at the first and last position of every run
    lo, hi = 0, (1 << sb) - 1
    out = []
    for r in runs:
        r = sorted(set(r) - {lo, hi})
        out.append(sorted(set([lo] + r[1:-1] + [hi])) if len(r) >= 2 else [lo])
    return out


_EDGE_CACHE = {}


def _edge_buckets(k, pb):
    if (k, pb) not in _EDGE_CACHE:
        sb, rng = _sb(k, pb), random.Random(k * 7 + pb)
        bs, p = [dict() for _ in range(8)], 1
        for total in (MANY_SMALL - 1, MANY_SMALL, MANY_SMALL + 1, MANY_LDS - 1, MANY_LDS, MANY_LDS + 1):
            for m in (2, 3, 8):
                for shape in ("even", "ones", "tail"):
                    for pattern in ("all_shared", "none_shared", "multiplicities", "ends"):
                        lens = _split(total, m, shape, rng)
                        runs = _runs_with_pattern(rng, lens, pattern, sb)
                        # sets may have shrunk a run: top the first run up so that the words of all holders are `total` again
                        have = set().union(*map(set, runs))
                        while sum(map(len, runs)) < total:
                            v = rng.getrandbits(sb)
                            if v not in have:
                                have.add(v)
                                j = max(range(m), key=lambda i: len(runs[i]))
                                runs[j] = sorted(runs[j] + [v])
                        assert sum(map(len, runs)) == total
                        holders = {2: (1, 6), 3: (0, 3, 7), 8: tuple(range(8))}[m]  # which of the eight operands hold the bucket
                        for i, run in zip(sorted(holders), runs):
                            bs[i][p] = _side(rng, rng.choice(["vec", "svec", "trie"]), run)
                        p += 3
        _EDGE_CACHE[(k, pb)] = bs
    return _EDGE_CACHE[(k, pb)]


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k,pb", [(31, 24), (59, 28)])
def test_short_route_edges(op, k, pb):
    """words of all holders on either side of both thresholds, m in {2, 3, 8} holders out of eight operands: merge runs them in one call; intersect visits a
    prefix only when ALL operands hold it, so it runs one call per holder set with exactly those operands"""
    bs = _edge_buckets(k, pb)
    if op == "or":
        _check(k, pb, False, bs, op)
        return
    # intersect visits a prefix only when all operands hold it: group the buckets by holder set and run every group as one call
    groups = {}
    for p in sorted(set().union(*bs)):
        hs = tuple(i for i in range(8) if p in bs[i])
        groups.setdefault(hs, []).append(p)
    for hs, ps in groups.items():
        _check(k, pb, False, [{p: bs[i][p] for p in ps} for i in hs], op)


# ---------------------------------------------------------------- 4: the long route
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k,pb", [(15, 6), (31, 3)])  # SUFFIX_BITS 24 and 65 (wide)
def test_long_route(op, k, pb):
    sb, rng = _sb(k, pb), random.Random(k)
    pool = sm.distinct(rng, 9000, sb)
    shared = pool[:3000]
    b0 = {1: _side(rng, "trie", shared + pool[3000:5000]), 2: _side(rng, "vec", pool[:5000]), 3: _side(rng, "trie", pool[:4000])}  # 5000 words
    b1 = {1: _side(rng, "vec", [shared[7]]), 2: _side(rng, "svec", pool[2600:2601]), 3: _side(rng, "vec", pool[4000:4001])}  # 1 word
    b2 = {1: _side(rng, "vec", shared + pool[5000:8500]), 2: _side(rng, "trie", pool[2500:9000]), 3: _side(rng, "vec", pool[4000:9000])}  # 6500 words
    assert [len(b[1][1]) for b in (b0, b1, b2)] == [5000, 1, 6500] and SORT_LDS < 5000
    d, gs, exp, ms = _check(k, pb, False, [b0, b1, b2], op, keep=True)
    if op == "and":
        assert sorted(exp.buckets) == [1, 2] and 3 not in exp.buckets  # prefix 3: a long bucket whose intersection is empty
    for g in [d] + gs:
        g.close()
    # five operands, the middle one lacks the long bucket (merge: a fold step skips it; intersect: the prefix is not visited at all)
    five = [{1: _side(rng, rng.choice(["vec", "trie"]), rng.sample(pool, n)), 5: _side(rng, "vec", rng.sample(pool, 40))} for n in (900, 700, 1, 1200, 800)]
    del five[2][1]
    _check(k, pb, False, five, op)
    if op == "and":  # ... and with all five holding it
        five[2][1] = _side(rng, "vec", rng.sample(pool, 3000))
        _check(k, pb, False, five, op)


# ---------------------------------------------------------------- 5: suffix widths and sentinels
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k,pb", [(33, 10), (33, 9), (33, 8), (5, 8)])  # SUFFIX_BITS 63, 64, 65 and 6
def test_suffix_widths_and_sentinel_values(op, k, pb):
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
    _check(k, pb, False, bs, op)


# ---------------------------------------------------------------- 6: whole-index shapes
def _few(rng, sb, n, kind="vec"):
    items = sm.distinct(rng, n, sb)
    return (kind, sorted(items) if kind == "trie" else items)


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("shape", ["one_empty", "all_empty", "disjoint_prefixes", "identical", "empty_everywhere", "first_and_last_prefix", "one_operand"])
def test_whole_index_shapes(op, shape):
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(sum(map(ord, shape)))
    some = {p: _few(rng, sb, n) for p, n in ((3, 5), (64, 1), (65, 30), (1 << 20, 1100))}
    other = {p: _few(rng, sb, n, "trie") for p, n in ((4, 5), (66, 2), (1 << 21, 1200))}
    third = {p: _few(rng, sb, n) for p, n in ((5, 5), (67, 2), (1 << 22, 300))}
    if shape == "one_empty":
        bs = [some, {}, {p: (kd, it[::-1]) for p, (kd, it) in some.items()}]
    elif shape == "all_empty":
        bs = [{}, {}, {}]
    elif shape == "disjoint_prefixes":
        bs = [some, other, third]
    elif shape == "identical":
        bs = [some] * 4
    elif shape == "empty_everywhere":  # shared prefixes, disjoint buckets: the intersection is empty in every bucket (merge keeps all)
        bs = [{p: _few(rng, sb, 9) for p in (1, 2, 700)} for _ in range(3)]
    elif shape == "first_and_last_prefix":
        last = (1 << pb) - 1
        a = {0: _few(rng, sb, 7), last: _few(rng, sb, 7), 9: _few(rng, sb, 3)}
        bs = [a, {0: ("vec", a[0][1][:3] + sm.distinct(rng, 3, sb)), last: ("trie", sorted(a[last][1][2:])), 10: _few(rng, sb, 3)},
              {0: ("trie", sorted(a[0][1][1:4])), last: ("vec", a[last][1][3:][::-1])}]
    else:
        bs = [{**some, **other}]  # n = 1: merge is a clone, intersect turns every bucket into an ascending Vec
    d, gs, exp, ms = _check(k, pb, False, bs, op, keep=True)
    if shape == "all_empty" or (op == "and" and shape in ("one_empty", "disjoint_prefixes", "empty_everywhere")):
        assert d.serialize() == bytes([0, 0]) and d.is_empty() and d.num_buckets() == 0
    if shape == "one_operand" and op == "and":
        assert all(v[0] == "vec" and v[1] == sorted(v[1]) for v in exp.buckets.values()) and len(exp.buckets) == len(bs[0])
    for g in [d] + gs:
        g.close()


# ---------------------------------------------------------------- 7: limits and errors
@pytest.mark.parametrize("op", OPS)
def test_sixty_four_operands(op):
    sb, rng = _sb(31, 24), random.Random(64)
    pool = sm.distinct(rng, 200, sb)
    bs = [{77: _side(rng, rng.choice(["vec", "trie"]), pool[:5] + rng.sample(pool[5:], rng.randint(1, 20)))} for _ in range(64)]
    _check(31, 24, False, bs, op)


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

    def refused(dst, srcs, op=0, n=None, msg=None):
        arr = (ctypes.c_void_p * max(1, len(srcs)))(*[x._h if x is not None else None for x in srcs])
        rc = L.cblx_set_op_many(dst._h, arr, len(srcs) if n is None else n, op)
        assert rc == cbl_amd.EINVAL, rc
        if msg:
            assert msg in L.cblx_last_error(dst._h).decode()
        assert [g.serialize() for g in everything] == before

    for op in (0, 1):
        refused(d, [], op)  # n == 0
        refused(d, extra, op)  # 65 valid contexts
        refused(d, [a, None, b], op)
        refused(d, [a, d, b], op)  # dst among srcs
        refused(a, [a], op)
        refused(d, [a, b, a], op)  # the same context twice
        for odd in (other_k, other_pb):
            refused(d, [a, odd, b], op)
            refused(odd, [a, b], op)
        refused(d, [a, b, canon], op, msg="One of the index is canonical while the other isn't")
        refused(d, [canon, a], op, msg="One of the index is canonical while the other isn't")
    for op in (2, 3, 4):  # SUB, XOR: the reference has no n-ary form; 4: unknown
        refused(d, [a, b, c], op)
    with pytest.raises(ValueError):
        cbl_amd.CBL.merge([])
    with pytest.raises(ValueError):
        cbl_amd.CBL.intersect([a, b, a])
    with pytest.raises(cbl_amd.CblxError) as e:
        cbl_amd.CBL.merge([a, canon], out=d)
    assert e.value.code == cbl_amd.EINVAL and "canonical" in str(e.value)
    assert [g.serialize() for g in everything] == before
    out = cbl_amd.CBL.merge([a, b, c], out=d)  # `out` is overwritten
    assert out is d and d.count() == 15 and d.num_buckets() == 1
    out = cbl_amd.CBL.intersect(extra[:64], out=d)
    assert out is d and d.is_empty()


# ---------------------------------------------------------------- 8: the result is a first-class index
@pytest.mark.parametrize("k,pb", [(15, 6), (31, 3)])  # SUFFIX_BITS 24 and 65 (wide)
def test_result_is_a_first_class_index(k, pb):
    import test_gpu_setops as t2

    G, words, ba, bb, shared = t2.first_class_operands(k, pb)
    o = Oracle(k, pb, False)
    rng = random.Random(pb)
    bc = {p: ("vec", rng.sample(it, len(it))) for p, (_, it) in ba.items()}  # a's sets as shuffled Vecs: a third operand
    d, gs, exp, ms = _check(k, pb, False, [ba, bb, bc], "and", keep=True)
    assert sm.words(exp) == shared and all(v[0] == "vec" for v in exp.buckets.values())
    universe = sm.words(ms[0]) | sm.words(ms[1])
    t2._membership_agrees(d, exp, o, G, words, universe)  # contains_seqs, contains_kmers, kmers_np, iter
    path = os.path.join(os.environ.get("TMPDIR", "/tmp"), "setops_many_%d_%d_%d.cbl" % (os.getpid(), k, pb))
    try:
        d.save_to_file(path)
        again = cbl_amd.CBL.load_from_file(path, k, pb)
    finally:
        if os.path.exists(path):
            os.unlink(path)
    assert again.serialize() == exp.serialize()
    # a further merge with the result as an operand
    u = cbl_amd.CBL.merge([gs[1], d, gs[0]])
    mu = mm.merge([ms[1], exp, ms[0]])
    assert u.serialize() == mu.serialize() and d.serialize() == exp.serialize() and gs[0].serialize() == ms[0].serialize() and gs[1].serialize() == ms[1].serialize()
    t2._membership_agrees(u, mu, o, G, words, universe | {w for w in words if w not in universe and w % 7 == 0})
    # `|=` into it, and insert_seq into it
    d |= gs[1]
    exp.merge(ms[1])
    assert d.serialize() == exp.serialize() and gs[1].serialize() == ms[1].serialize() and d.validate(False) == 0
    piece = bytes(G[100:400])
    u.insert_seq(piece)
    mu.insert_seq(piece)
    assert u.count() == mu.count() and u.serialize() == mu.serialize() and u.validate(False) == 0


# ---------------------------------------------------------------- 9: real k-mers
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("k,pb,canonical", [(31, 24, False), (31, 24, True), (59, 28, False), (59, 28, True)])
def test_real_kmers(op, k, pb, canonical):
    _need_gpu()
    import test_gpu_setops as t2

    seqs = t2._split_reads(77, 24, 150)
    parts = [seqs[:12], seqs[4:16], seqs[8:20], seqs[10:]]  # four overlapping read sets
    gs = [cbl_amd.CBL(k, pb, canonical=canonical) for _ in parts]
    ms = [PyCBL(k, pb, canonical) for _ in parts]
    for g, m, ss in zip(gs, ms, parts):
        for i in range(0, len(ss), 4):  # several flushes: the Vec order is the insertion order
            g.insert_seqs(*t2._batch(ss[i:i + 4]))
            g.count()
            for s in ss[i:i + 4]:
                m.insert_seq(s)
    for g, m in zip(gs, ms):
        assert g.serialize() == m.serialize()
    sets = [sm.words(m) for m in ms]
    exp = mm.MANY[op](ms)
    d = _run(op, gs)
    assert d.serialize() == exp.serialize()
    for g, m in zip(gs, ms):
        assert g.serialize() == m.serialize()
    kept = set().union(*sets) if op == "or" else set.intersection(*sets)
    assert kept and sm.words(exp) == kept
    assert d.count() == len(kept) and d.num_buckets() == len(exp.buckets) and d.validate(False) == 0
    o = Oracle(k, pb, canonical)
    o.load(d.serialize())
    got = list(o.iter_words())
    assert set(got) == kept and len(got) == len(kept)
    assert d.contains_kmers([o.kmer_of_word(w) for w in sorted(kept)]).all()
    dropped = sorted(set().union(*sets) - kept)[:500]
    if dropped:
        assert not d.contains_kmers([o.kmer_of_word(w) for w in dropped]).any()
    assert list(d.iter()) == [o.kmer_of_word(w) for w in got]
    for g in [d] + gs:
        g.close()


# ---------------------------------------------------------------- 10: seeded sweep
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("seed", range(40))
def test_seeded_sweep(op, seed):
    rng = random.Random(seed)
    k, pb = rng.choice([11, 31, 33, 59]), rng.choice([6, 12, 16])
    sb, canonical = _sb(k, pb), rng.random() < 0.5
    n = rng.randint(1, 6)
    bs = [dict() for _ in range(n)]
    for p in rng.sample(range(1 << pb), rng.randint(1, min(12, 1 << pb))):
        holders = [i for i in range(n) if rng.random() < 0.6] or [rng.randrange(n)]
        if op == "and" and rng.random() < 0.6:
            holders = list(range(n))
        share = rng.choice([0.0, 0.3, 1.0])
        common = sm.distinct(rng, min(rng.choice([1, 3, 40, 300]), (1 << sb) // 4), sb)
        for i in holders:
            own = min(rng.choice([0, 1, 3, 40, 400]), (1 << sb) // 4)
            items = set(rng.sample(common, max(1, int(share * len(common))))) | set(sm.distinct(rng, own, sb))
            kind = rng.choice(["vec", "svec", "trie"])
            bs[i][p] = _side(rng, kind, items)
    _check(k, pb, canonical, bs, op)


# ---------------------------------------------------------------- 11: the CLI
@pytest.mark.parametrize("cmd,op", [("merge-all", "or"), ("inter-all", "and")])
def test_cli(cmd, op, tmp_path):
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
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb), cmd] + paths + ["-o", out], cwd=str(ROOT), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert "Writing the index to " + out in r.stderr
    assert Path(out).read_bytes() == mm.MANY[op](ms).serialize()
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb), cmd, paths[0]], cwd=str(ROOT), env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode != 0 and "two or more" in r.stderr
