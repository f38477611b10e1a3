"""`a &= b`, `a -= b`, `a ^= b` on the GPU (cblx_set_op_assign, CBL.set_op_assign, `python -m cbl_amd inter | diff | sym-diff`) against
tests/setops_assign_model.py, byte for byte: BOTH operands after the operation. Operands are installed with `CBL.load(PyCBL(...).serialize())` from
crafted bucket dicts, so kind, stored order and length are the test's own; tests/test_setops_assign_model.py shows on the CPU that the model's Vec
layout is remove_sorted_iter's literal replay and that its sets are the set algebra."""
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

import setops_assign_model as am  # noqa: E402  (tests/)
import setops_model as sm  # noqa: E402  (tests/)

ROOT = Path(__file__).resolve().parent.parent
T = 512  # kernels_setops.hpp UNI_TILE: outputs of one round of k_bucket_setop (a's side a Trie)
SORT_LDS = 4096  # kernels_setops.hpp SETOP_SORT_LDS: the longest Vec side one workgroup sorts in LDS
SA_LDS = 1024  # kernels_setops.hpp SA_LDS: the longest Vec whose fix-up tables sit in LDS
LENGTHS = (1, 2, 3, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 1024, 1025, 4096, 4097, 5000)
CONFIGS = [(31, 24), (59, 28)]  # SUFFIX_BITS 43 (one word) and 97 (two words)
assert SA_LDS in LENGTHS and SA_LDS + 1 in LENGTHS and SORT_LDS in LENGTHS and SORT_LDS + 1 in LENGTHS


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _gpu(m: PyCBL):
    g = cbl_amd.CBL(m.P["K"], m.P["PB"], canonical=m.canonical)
    g.load(m.serialize())
    return g


def _sb(k, pb):
    return params(k, pb)["SB"]


def _agrees(ga, gb, ma, mb, what=""):
    assert ga.serialize() == ma.serialize(), "left operand " + what
    assert gb.serialize() == mb.serialize(), "right operand " + what
    assert ga.count() == ma.count() and ga.num_buckets() == len(ma.buckets)
    assert ga.validate(False) == 0
    assert ga.is_empty() == (ma.count() == 0)


def _check(k, pb, canonical, ba, bb, op, keep=False):
    """one assigning operation on two crafted bucket dicts: the bytes of both operands, count, buckets, validate"""
    _need_gpu()
    ma, mb = sm.from_buckets(k, pb, canonical, ba), sm.from_buckets(k, pb, canonical, bb)
    ga, gb = _gpu(ma), _gpu(mb)
    assert ga.serialize() == ma.serialize() and gb.serialize() == mb.serialize()  # as crafted, stored order included
    am.set_op_assign(ma, mb, op)
    assert ga.set_op_assign(gb, op) is ga
    _agrees(ga, gb, ma, mb, "after %s" % op)
    assert ga.is_canonical() == canonical
    if keep:
        return ga, gb, ma, mb
    ga.close()
    gb.close()


# ---------------------------------------------------------------- 1: the swap_remove layout
_SHAPE_CACHE = {}


def _shape_buckets(k, pb, op, ins_mode):
    """One both-sided bucket per (length, named deletion set): a is a shuffled Vec of n words, b is built so that exactly the indices of the set are
    deleted from sorted a. `&=`: b holds what stays; `-=` and `^=`: b holds what goes. Words only b holds: `&=` / `-=` a few (they change nothing);
    `^=` 0, 3 or more than the deletions (ins_mode 0 / 1 / 2) — they are pushed at the end of a."""
    key = (k, pb, op, ins_mode)
    if key not in _SHAPE_CACHE:
        sb, rng = _sb(k, pb), random.Random(k * 1000 + pb * 10 + ins_mode + 7 * len(op) + ord(op[0]))
        ba, bb, p = {}, {}, 3
        for n in LENGTHS:
            for name, D in sorted(am.named_shapes(n).items()):
                extra = {0: 0, 1: 3, 2: len(D) + 5}[ins_mode] if op == "xor" else 4
                pool = sorted(sm.distinct(rng, n + extra, sb))
                own = set(rng.sample(range(n + extra), extra))  # b's own words lie between a's
                A = [v for i, v in enumerate(pool) if i not in own]
                inD = set(D)
                B = [v for i, v in enumerate(pool) if i in own]
                B += [A[i] for i in range(n) if (i in inD) != (op == "and")]
                if not B:
                    continue  # (`^=` without any word of b: not a both-sided bucket)
                stored = list(A)
                rng.shuffle(stored)
                ba[p] = ("vec", stored)
                if p % 2:
                    rng.shuffle(B)
                    bb[p] = ("vec", B)
                else:
                    bb[p] = ("trie", sorted(B))
                p += 5
        _SHAPE_CACHE[key] = (ba, bb)
    return _SHAPE_CACHE[key]


@pytest.mark.parametrize("op", ["and", "sub"])
@pytest.mark.parametrize("k,pb", CONFIGS)
def test_fixup_shapes(op, k, pb):
    ba, bb = _shape_buckets(k, pb, op, 0)
    _check(k, pb, False, ba, bb, op)


@pytest.mark.parametrize("ins_mode", [0, 1, 2])
@pytest.mark.parametrize("k,pb", CONFIGS)
def test_fixup_shapes_xor(ins_mode, k, pb):
    ba, bb = _shape_buckets(k, pb, "xor", ins_mode)
    ga, gb, ma, mb = _check(k, pb, False, ba, bb, "xor", keep=True)
    if ins_mode:
        assert any(kd == "vec" and len(it) > 1024 for kd, it in ma.buckets.values()), "a `^=` result crosses 1024 words and stays a Vec"
    ga.close()
    gb.close()


# ---------------------------------------------------------------- 2: kinds
_KIND_CACHE = {}


def _kind_buckets():
    if not _KIND_CACHE:
        sb, rng = _sb(31, 24), random.Random(777)

        def side(kind, n, pool):
            items = rng.sample(pool, n)
            return (kind, sorted(items) if kind == "trie" else items)

        sides = [("vec", 17), ("vec", 5000), ("trie", 1025), ("trie", 5000)]
        ba, bb, p = {}, {}, 5
        for sa in sides:
            for sb_ in sides:
                pool = sm.distinct(rng, max(sa[1], sb_[1]) + min(sa[1], sb_[1]) // 2 + 1, sb)  # both sides draw from it: they overlap
                ba[p], bb[p] = side(*sa, pool), side(*sb_, pool)
                p += 7
        for i, s in enumerate(sides):  # one-sided buckets of every kind on both sides
            pool = sm.distinct(rng, s[1] * 2, sb)
            ba[p + 2 * i] = side(*s, pool)
            bb[p + 2 * i + 1] = side(*s, pool)
        p += 2 * len(sides) + 3
        x = sorted(sm.distinct(rng, 1025 + 40, sb))
        big, rest = x[:1025], x[1025:]
        # results of exactly one word in a Trie, whatever the op: AND (b holds one of a's), SUB and XOR (b holds all but one)
        ba[p], bb[p] = ("trie", big), ("vec", [big[500]] + rest[:3])
        ba[p + 1], bb[p + 1] = ("trie", big), ("trie", big[:77] + big[78:])
        # results that come out empty, from a Vec and from a Trie: disjoint (AND), equal (SUB, XOR)
        ba[p + 2], bb[p + 2] = ("vec", rest[:20]), ("vec", rest[20:])
        ba[p + 3], bb[p + 3] = ("trie", big), ("trie", sorted(sm.distinct(rng, 1030, sb - 1)))
        e = list(rest)
        rng.shuffle(e)
        ba[p + 4], bb[p + 4] = ("vec", list(rest)), ("vec", e)
        ba[p + 5], bb[p + 5] = ("trie", big), ("vec", big[::-1])
        p += 8
        # a shared value on every round boundary of k_bucket_setop (a's side a Trie), and the same lists with a's side a Vec
        for na, nb in ((T, T), (T - 1, T + 1), (2 * T + 1, 2 * T + 1), (1, 2 * T + 1), (T + 1, T - 1)):
            A, B = sm.straddling_lists(na, nb, T, rng, bits=sb)
            ba[p], bb[p] = ("trie", A), ("trie", B)
            ba[p + 1], bb[p + 1] = ("vec", A[::-1]), ("trie", B)
            p += 2
        _KIND_CACHE["b"] = (ba, bb)
    return _KIND_CACHE["b"]


@pytest.mark.parametrize("op", am.OPS)
@pytest.mark.parametrize("canonical", [False, True])
def test_kinds(op, canonical):
    ba, bb = _kind_buckets()
    ga, gb, ma, mb = _check(31, 24, canonical, ba, bb, op, keep=True)
    tries = [len(it) for kd, it in ma.buckets.values() if kd == "trie"]
    assert 1 in tries, "a Trie of one word"
    assert len(ma.buckets) < len(set(ba) | set(bb)), "emptied buckets left the directory"
    ga.close()
    gb.close()


@pytest.mark.parametrize("op", am.OPS)
def test_kinds_with_wide_suffixes(op):
    k, pb = 59, 28
    sb, rng = _sb(k, pb), random.Random(59)
    ba, bb, p = {}, {}, 11
    for ka, na in (("vec", 40), ("vec", 4500), ("trie", 1025)):
        for kb, nb in (("vec", 40), ("vec", 4500), ("trie", 1025)):
            pool = sm.distinct(rng, max(na, nb) + min(na, nb) // 2 + 1, sb)
            A, B = rng.sample(pool, na), rng.sample(pool, nb)
            ba[p], bb[p] = (ka, sorted(A) if ka == "trie" else A), (kb, sorted(B) if kb == "trie" else B)
            p += 3
    ba[p], bb[p + 1] = ("vec", sm.distinct(rng, 9, sb)), ("trie", sorted(sm.distinct(rng, 1030, sb)))
    ones = (1 << sb) - 1
    ba[p + 2], bb[p + 2] = ("vec", [ones, 0, 1 << 64, (1 << 64) - 1, 5]), ("vec", [1 << 64, ones, 7, 1 << 63])
    _check(k, pb, True, ba, bb, op)


# ---------------------------------------------------------------- 3: empty operands
@pytest.mark.parametrize("op", am.OPS)
@pytest.mark.parametrize("shape", ["empty_a", "empty_b", "both_empty", "no_shared_prefix"])
def test_empty_operands(op, shape):
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(len(shape))
    some = {3: ("vec", sm.distinct(rng, 5, sb)), 64: ("vec", sm.distinct(rng, 1, sb)), 1 << 20: ("trie", sorted(sm.distinct(rng, 1100, sb)))}
    other = {4: ("vec", sm.distinct(rng, 6, sb)), 1 << 21: ("trie", sorted(sm.distinct(rng, 1200, sb)))}
    ba, bb = {"empty_a": ({}, some), "empty_b": (some, {}), "both_empty": ({}, {}), "no_shared_prefix": (some, other)}[shape]
    ga, gb, ma, mb = _check(k, pb, False, ba, bb, op, keep=True)
    want_empty = shape == "both_empty" or (shape == "empty_a" and op != "xor") or (shape in ("empty_b", "no_shared_prefix") and op == "and")
    assert ga.is_empty() == want_empty
    if want_empty:
        assert ga.serialize() == bytes([0, 0])  # the flag byte and varint(0)
    if shape == "empty_a" and op == "xor":
        assert ga.serialize() == gb.serialize()  # a clone of b as stored
    ga.close()
    gb.close()


# ---------------------------------------------------------------- 4: refusals
def test_refusals_leave_both_operands_alone():
    _need_gpu()
    rng = random.Random(1)
    mk = lambda canonical=False, k=31, pb=24: _gpu(sm.from_buckets(k, pb, canonical, {7: ("vec", sm.distinct(rng, 5, min(_sb(31, 24), _sb(k, pb))))}))
    a, b, other_k, other_pb, canon = mk(), mk(), mk(k=33), mk(pb=20), mk(canonical=True)
    everyone = (a, b, other_k, other_pb, canon)
    before = [x.serialize() for x in everyone]
    L = cbl_amd.lib()

    def refused(x, y, op, msg=None):
        rc = L.cblx_set_op_assign(x._h, y._h, op)
        assert rc == cbl_amd.EINVAL, rc
        if msg:
            assert msg in L.cblx_last_error(x._h).decode()
        assert [g.serialize() for g in everyone] == before

    for op in (0, 1, 2, 3):
        refused(a, a, op)
        for odd in (other_k, other_pb):
            refused(a, odd, op)
            refused(odd, b, op)
        refused(a, canon, op, "One of the index is canonical while the other isn't")
        refused(canon, b, op, "One of the index is canonical while the other isn't")
    refused(a, b, 4)
    with pytest.raises(cbl_amd.CblxError) as e:
        a.set_op_assign(canon, "and")
    assert e.value.code == cbl_amd.EINVAL and "canonical" in str(e.value)
    assert [g.serialize() for g in everyone] == before
    for g in everyone:
        g.close()


# ---------------------------------------------------------------- 5: the Python surface
def test_python_surface():
    _need_gpu()
    rng = random.Random(2)
    sb = _sb(31, 24)
    x = sm.distinct(rng, 30, sb)
    ba, bb = {1: ("vec", x[:20]), 2: ("vec", x[:3])}, {1: ("vec", x[10:]), 9: ("vec", x[:2])}
    a, b, a2, b2 = (_gpu(sm.from_buckets(31, 24, False, d)) for d in (ba, bb, ba, bb))
    assert a.set_op_assign(b, "or") is a
    a2 |= b2
    assert a.serialize() == a2.serialize() and b.serialize() == b2.serialize()
    with pytest.raises(ValueError):
        a.set_op_assign(b, "nand")
    for stmt in ("a &= b", "a -= b", "a ^= b"):
        with pytest.raises(NotImplementedError, match="set_op_assign"):
            exec(stmt, {"a": a, "b": b})
    assert a.serialize() == a2.serialize()
    for g in (a, b, a2, b2):
        g.close()


# ---------------------------------------------------------------- 6: the result is a first-class index
_REAL = {}


def _reads(seed, n, length):
    bases, offsets = synth.reads(seed, n, length)
    raw, off = bytes(np.asarray(bases, dtype=np.uint8)), [int(x) for x in np.asarray(offsets)]
    return [raw[off[i]:off[i + 1]] for i in range(n)]


def _batch(seqs):
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)


def _model_of(g, k, pb):
    """the index as the GPU holds it (built from reads: compared with the oracle in tests/test_gpu_parity.py), as a model index"""
    return sm.from_buckets(k, pb, False, {p: ("trie" if kd else "vec", items) for p, kd, items in g.buckets()})


def _real_operands(k, pb):
    """two indexes of real k-mers that share about half of their reads, in three insert calls each (Vec order = insertion order); the buckets
    they hold and the words of every read, computed once"""
    if (k, pb) not in _REAL:
        _need_gpu()
        seqs = _reads(11, 3000, 100)
        sa, sb_ = seqs[:2000], seqs[1000:]
        o = Oracle(k, pb, False)
        words = [w for s in seqs for w in o.seq_words(s)]
        buckets = []
        for ss in (sa, sb_):
            g = cbl_amd.CBL(k, pb)
            for i in range(0, len(ss), 700):
                g.insert_seqs(*_batch(ss[i:i + 700]))
                g.count()
            buckets.append({p: (kd, list(it)) for p, (kd, it) in _model_of(g, k, pb).buckets.items()})
            g.close()
        _REAL[(k, pb)] = (seqs, words, buckets[0], buckets[1])
    return _REAL[(k, pb)]


def _answers_as_the_model(g, m: PyCBL, o: Oracle, seqs, words):
    inside = sm.words(m)
    flags, total, positive = g.contains_seqs(*_batch(seqs))
    want = np.fromiter((w in inside for w in words), dtype=bool, count=len(words))
    assert total == len(words) and positive == int(want.sum())
    assert np.array_equal(np.asarray(flags).astype(bool), want)
    sb = m.P["SB"]
    expect = [o.kmer_of_word((p << sb) | s) for p in sorted(m.buckets) for s in m.buckets[p][1]]  # CBL::iter: prefixes ascending, stored order
    lo, hi = g.kmers_np()
    got = [int(x) for x in lo] if hi is None else [int(x) | (int(y) << 64) for x, y in zip(lo, hi)]
    assert got == expect


@pytest.mark.parametrize("op", am.OPS)
@pytest.mark.parametrize("k,pb", [(31, 12), (59, 14)])  # SUFFIX_BITS 55 and 111 (wide)
def test_result_is_a_first_class_index(op, k, pb):
    seqs, words, ba, bb = _real_operands(k, pb)
    o = Oracle(k, pb, False)
    ga, gb, ma, mb = _check(k, pb, False, ba, bb, op, keep=True)
    assert any(kd == "vec" and len(it) > 1 for kd, it in ma.buckets.values()) and ma.count() > 1000
    _answers_as_the_model(ga, ma, o, seqs, words)  # reads of both operands
    again = cbl_amd.CBL(k, pb)
    again.load(ga.serialize())
    assert again.serialize() == ma.serialize()
    again.close()
    # a further `|=` and a further assigning operation
    ga |= gb
    ma.merge(mb)
    _agrees(ga, gb, ma, mb, "after a further |=")
    nxt = {"and": "sub", "sub": "xor", "xor": "and"}[op]
    mc = sm.from_buckets(k, pb, False, ba)
    gc = _gpu(mc)
    ga.set_op_assign(gc, nxt)
    am.set_op_assign(ma, mc, nxt)
    _agrees(ga, gc, ma, mc, "after a further %s" % nxt)
    if ma.count():
        _answers_as_the_model(ga, ma, o, seqs, words)
    for g in (ga, gb, gc):
        g.close()


# ---------------------------------------------------------------- 7: seeded sweep
@pytest.mark.parametrize("op", am.OPS)
@pytest.mark.parametrize("seed", range(40))
def test_seeded_sweep(op, seed):
    rng = random.Random(seed)
    k, pb = rng.choice([11, 31, 33, 59]), rng.choice([6, 12, 16])
    sb, canonical = _sb(k, pb), rng.random() < 0.5
    ba, bb = {}, {}
    for p in rng.sample(range(1 << pb), rng.randint(1, min(12, 1 << pb))):
        na, nb = (min(rng.choice([0, 1, 3, 40, 600, 1024, 1025, 3000]), (1 << sb) // 2) for _ in range(2))
        if na == 0 and nb == 0:
            na = 1
        share = rng.choice([0.0, 0.3, 1.0])
        pool = sm.distinct(rng, na + nb, sb)
        A = pool[:na]
        nshared = int(share * min(na, nb))
        B = A[:nshared] + pool[na:na + nb - nshared]
        rng.shuffle(B)
        for side, items in ((ba, A), (bb, B)):
            if items:
                kind = rng.choice(["vec", "trie"])
                side[p] = (kind, sorted(items) if kind == "trie" or rng.random() < 0.2 else items)
    _check(k, pb, canonical, ba, bb, op)


# ---------------------------------------------------------------- 8: the command line
@pytest.mark.parametrize("cmd,op", [("inter", "and"), ("diff", "sub"), ("sym-diff", "xor")])
def test_cli(tmp_path, cmd, op):
    _need_gpu()
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(8)
    x = sm.distinct(rng, 60, sb)
    ma = sm.from_buckets(k, pb, False, {1: ("vec", x[:30]), 2: ("vec", x[:4]), 70000: ("trie", sorted(x))})
    mb = sm.from_buckets(k, pb, False, {1: ("vec", x[45:14:-1]), 5: ("vec", x[:2]), 70000: ("vec", x[50:])})
    fa, fb, out = tmp_path / "a.cbl", tmp_path / "b.cbl", tmp_path / "out.cbl"
    fa.write_bytes(ma.serialize())
    fb.write_bytes(mb.serialize())
    am.set_op_assign(ma, mb, op)
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb), cmd, str(fa), str(fb), "-o", str(out)], cwd=str(ROOT),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == ma.serialize()
