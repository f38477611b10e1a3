"""`a | b`, `a & b`, `a - b`, `a ^ b` into a new index on the GPU (cblx_set_op) against tests/setops_model.py, byte for byte: the result AND both
operands after the operation (the reference's iter_sorted leaves their Vec buckets sorted on the prefixes both hold). Operands are installed with
`CBL.load(PyCBL(...).serialize())` from crafted bucket dicts, so kind, stored order and length are the test's own; tests/test_setops_model.py shows
on the CPU that the model agrees with the oracle and that the list builders put a pair on every round boundary."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd import synth  # noqa: E402
from oracle import Oracle  # noqa: E402
from oracle.pyref import PyCBL, params  # noqa: E402

import query_shapes as qs  # noqa: E402  (tests/)
import setops_model as sm  # noqa: E402  (tests/)

T = 512  # kernels_setops.hpp UNI_TILE = UNI_THREADS * UNI_ITEMS = 128 * 4: outputs of one round of k_bucket_setop
SORT_LDS = 4096  # kernels_setops.hpp SETOP_SORT_LDS: the longest Vec side one workgroup sorts in LDS; longer ones take the general kernel


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _gpu(m: PyCBL):
    g = cbl_amd.CBL(m.P["K"], m.P["PB"], canonical=m.canonical)
    g.load(m.serialize())
    return g


def _check(k, pb, canonical, ba, bb, op, keep=False):
    """one operation on two crafted bucket dicts: the three byte equalities, count, buckets, validate"""
    _need_gpu()
    ma, mb = sm.from_buckets(k, pb, canonical, ba), sm.from_buckets(k, pb, canonical, bb)
    ga, gb = _gpu(ma), _gpu(mb)
    assert ga.serialize() == ma.serialize() and gb.serialize() == mb.serialize()  # as crafted, stored order included
    exp = sm.set_op(ma, mb, op)
    d = cbl_amd.CBL.set_op(ga, gb, op)
    assert d.count() == exp.count()
    assert d.num_buckets() == len(exp.buckets)
    assert d.validate(False) == 0
    assert d.is_empty() == (exp.count() == 0)
    assert d.is_canonical() == canonical
    assert d.serialize() == exp.serialize(), "result"
    assert ga.serialize() == ma.serialize(), "left operand after the operation"
    assert gb.serialize() == mb.serialize(), "right operand after the operation"
    if keep:
        return d, ga, gb, exp, ma, mb
    for g in (d, ga, gb):
        g.close()


def _sb(k, pb):
    return params(k, pb)["SB"]


# ---------------------------------------------------------------- 4a: round edges
_ROUND_CACHE = {}


def _round_edge_buckets(k, pb):
    """both sides Tries; every pair of lengths from {1, T-1, T, T+1, 2T+1} with a pair straddling each round boundary, all shared, none shared"""
    if (k, pb) not in _ROUND_CACHE:
        sb, rng = _sb(k, pb), random.Random(k * 1000 + pb)
        ba, bb, p = {}, {}, 1
        lens = (1, T - 1, T, T + 1, 2 * T + 1)
        for na in lens:
            for nb in lens:
                cases = [sm.straddling_lists(na, nb, T, rng, bits=sb), sm.random_lists(rng, na, nb, 0, bits=sb)]
                big = sorted(sm.distinct(rng, max(na, nb), sb))
                small = sorted(rng.sample(big, min(na, nb)))  # every value of the shorter side is shared
                cases.append((big, small) if na >= nb else (small, big))
                for A, B in cases:
                    assert len(A) == na and len(B) == nb
                    ba[p], bb[p] = ("trie", A), ("trie", B)
                    p += 3
        _ROUND_CACHE[(k, pb)] = (ba, bb)
    return _ROUND_CACHE[(k, pb)]


@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("k,pb", [(31, 24), (59, 28)])
def test_round_edges(op, k, pb):
    ba, bb = _round_edge_buckets(k, pb)
    _check(k, pb, False, ba, bb, op)


# ---------------------------------------------------------------- 4b: kinds and order
_KIND_CACHE = {}


def _kind_buckets():
    if not _KIND_CACHE:
        sb, rng = _sb(31, 24), random.Random(4242)

        def side(kind, n, shuffled, pool):
            items = sorted(rng.sample(pool, n))
            if shuffled:
                rng.shuffle(items)
            return (kind, items)

        # (kind, length, shuffled): unsorted Vecs, long Vecs (one ascending, one shuffled, on either side of the LDS sort's limit), Tries
        sides = [("vec", 1, True), ("vec", 17, True), ("vec", 1024, True), ("vec", 1025, False), ("vec", 5000, True), ("trie", 1025, False), ("trie", 5000, False)]
        assert 1025 <= SORT_LDS < 5000
        ba, bb, p = {}, {}, 5
        for sa in sides:
            for sb_ in sides:
                pool = sm.distinct(rng, max(sa[1], sb_[1]) + min(sa[1], sb_[1]) // 2 + 1, sb)  # both sides draw from it: they overlap
                ba[p], bb[p] = side(*sa, pool), side(*sb_, pool)
                p += 7
        for i, s in enumerate(sides):  # one-sided buckets of every kind on both sides: bytes come through unchanged
            pool = sm.distinct(rng, s[1] * 2, sb)
            ba[p + 2 * i] = side(*s, pool)
            bb[p + 2 * i + 1] = side(*s, pool)
        p += 2 * len(sides) + 3
        x, y = sm.distinct(rng, 40, sb), sm.distinct(rng, 900, sb)
        ba[p], bb[p] = ("vec", x[:20]), ("vec", x[20:])  # disjoint: AND is empty
        e1, e2 = list(y), list(y)
        rng.shuffle(e2)
        ba[p + 1], bb[p + 1] = ("vec", e1), ("vec", e2)  # equal sets in two orders: SUB and XOR are empty
        ba[p + 2], bb[p + 2] = ("trie", sorted(x)), ("vec", list(x))
        _KIND_CACHE["b"] = (ba, bb)
    return _KIND_CACHE["b"]


@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("canonical", [False, True])
def test_kinds_and_stored_order(op, canonical):
    ba, bb = _kind_buckets()
    _check(31, 24, canonical, ba, bb, op)


# ---------------------------------------------------------------- 4c: suffix widths
@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("k,pb", [(33, 10), (33, 9), (33, 8), (5, 8)])  # SUFFIX_BITS 63, 64, 65 and 6
def test_suffix_widths_and_sentinel_values(op, k, pb):
    sb = _sb(k, pb)
    assert sb == {(33, 10): 63, (33, 9): 64, (33, 8): 65, (5, 8): 6}[(k, pb)]
    ones, top = (1 << sb) - 1, 1 << (sb - 1)
    special = [0, 1, 2, 3, top - 1, top, top + 1, top | 2, ones - 1, ones] + ([1 << 63, (1 << 63) - 1, (1 << 64) - 1, 1 << 64] if sb > 64 else [])
    special = sorted(set(v for v in special if v <= ones))
    rng = random.Random(sb)
    ba, bb, p = {}, {}, 0
    for ka in ("trie", "vec"):
        for kb in ("trie", "vec"):
            for sel in range(6):
                if sel == 0:
                    A, B = list(special), list(special)
                elif sel == 1:
                    A, B = special[::2], special[1::2]
                elif sel == 2:
                    A, B = [ones], [0, ones]
                elif sel == 3:
                    A, B = [0, top, ones], [top - 1, ones - 1]
                else:
                    A, B = (sorted(rng.sample(special, len(special) // 2 + 1)) for _ in range(2))
                if ka == "vec":
                    A = A[::-1]
                if kb == "vec":
                    B = B[::-1]
                ba[p], bb[p] = (ka, list(A)), (kb, list(B))
                p += 1
    if sb > 8:  # long lists around the special values: several rounds
        fill = sm.distinct(rng, 3 * T, sb)
        ba[p], bb[p] = ("trie", sorted(set(fill[:2 * T] + special))), ("trie", sorted(set(fill[T:] + special[::2])))
    top_p = (1 << pb) - 1
    ba[top_p], bb[top_p] = ("vec", [ones, 0]), ("trie", [0, ones])
    _check(k, pb, False, ba, bb, op)


# ---------------------------------------------------------------- 4d: whole-index shapes
def _few(rng, sb, n, kind="vec"):
    items = sm.distinct(rng, n, sb)
    return (kind, sorted(items) if kind == "trie" else items)


@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("shape", ["empty_a", "empty_b", "both_empty", "disjoint_prefixes", "identical", "all_empty_result", "first_and_last_prefix"])
def test_whole_index_shapes(op, shape):
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(sum(map(ord, shape)))
    some = {p: _few(rng, sb, n) for p, n in ((3, 5), (64, 1), (65, 30), (1 << 20, 1100))}
    other = {p: _few(rng, sb, n, "trie") for p, n in ((4, 5), (66, 2), (1 << 21, 1200))}
    if shape == "empty_a":
        ba, bb = {}, some
    elif shape == "empty_b":
        ba, bb = some, {}
    elif shape == "both_empty":
        ba, bb = {}, {}
    elif shape == "disjoint_prefixes":
        ba, bb = some, other
    elif shape == "identical":
        ba, bb = some, {p: (kd, list(it)) for p, (kd, it) in some.items()}
    elif shape == "all_empty_result":  # whatever the op: AND of disjoint buckets on shared prefixes; SUB / XOR / OR see the same sets
        if op == "and":
            ba, bb = {p: _few(rng, sb, 9) for p in (1, 2, 700)}, {p: _few(rng, sb, 9) for p in (1, 2, 700)}
        elif op == "or":
            ba, bb = {}, {}
        else:
            ba = {p: _few(rng, sb, 9) for p in (1, 2, 700)}
            bb = {p: (kd, it[::-1]) for p, (kd, it) in ba.items()}
    else:
        last = (1 << pb) - 1
        ba = {0: _few(rng, sb, 7), last: _few(rng, sb, 7), 9: _few(rng, sb, 3)}
        bb = {0: ("vec", ba[0][1][:3] + sm.distinct(rng, 3, sb)), last: ("trie", sorted(ba[last][1][2:])), 10: _few(rng, sb, 3)}
    r = _check(k, pb, False, ba, bb, op, keep=True)
    if shape in ("both_empty", "all_empty_result"):
        assert r[0].serialize() == bytes([0, 0]) and r[0].is_empty() and r[0].num_buckets() == 0  # the flag byte and varint(0)
    for g in r[:3]:
        g.close()


@pytest.mark.parametrize("op", sm.OPS)
def test_three_thousand_buckets_of_mixed_fate(op):
    """PREFIX_BITS = 16: runs of 64 * j prefixes whose buckets all vanish (bitvector words that become zero), runs that stay, and mixed words"""
    k, pb = 31, 16
    sb, rng = _sb(k, pb), random.Random(16)
    ba, bb = {}, {}
    for p in range(0, 1 << pb, 21):
        word = p >> 6
        fate = "same" if word % 5 == 0 else "disjoint" if word % 5 == 1 else rng.choice(["same", "disjoint", "overlap", "a_only", "b_only"])
        n = rng.choice([1, 2, 5, 40])
        x = sm.distinct(rng, 2 * n, sb)
        if fate == "same":
            ba[p], bb[p] = ("vec", x[:n]), ("vec", x[:n][::-1])
        elif fate == "disjoint":
            ba[p], bb[p] = ("vec", x[:n]), ("vec", x[n:])
        elif fate == "overlap":
            ba[p], bb[p] = ("vec", x[:n + 1]), ("vec", x[n:])
        elif fate == "a_only":
            ba[p] = ("vec", x)
        else:
            bb[p] = ("vec", x)
    assert 3000 <= len(set(ba) | set(bb)) <= 3300
    _check(k, pb, False, ba, bb, op)


# ---------------------------------------------------------------- 4e: real k-mers
def _split_reads(seed, n, length):
    bases, offsets = synth.reads(seed, n, length)
    bases, offsets = np.asarray(bases, dtype=np.uint8), np.asarray(offsets, dtype=np.uint64)
    raw = bytes(bases)
    return [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(n)]


def _batch(seqs):
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)


@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("k,pb,canonical", [(31, 24, False), (31, 24, True), (59, 28, False), (59, 28, True)])
def test_real_kmers(op, k, pb, canonical):
    _need_gpu()
    seqs = _split_reads(77, 24, 150)
    sa, sb_ = seqs[:16], seqs[8:]
    ga, gb = cbl_amd.CBL(k, pb, canonical=canonical), cbl_amd.CBL(k, pb, canonical=canonical)
    ma, mb = PyCBL(k, pb, canonical), PyCBL(k, pb, canonical)
    for g, m, ss in ((ga, ma, sa), (gb, mb, sb_)):
        for i in range(0, len(ss), 4):  # several flushes: the Vec order is the insertion order
            g.insert_seqs(*_batch(ss[i:i + 4]))
            g.count()
            for s in ss[i:i + 4]:
                m.insert_seq(s)
    assert ga.serialize() == ma.serialize() and gb.serialize() == mb.serialize()
    oa, ob = Oracle(k, pb, canonical), Oracle(k, pb, canonical)
    oa.load(ma.serialize())
    ob.load(mb.serialize())
    wa, wb = set(oa.iter_words()), set(ob.iter_words())
    exp = sm.set_op(ma, mb, op)
    d = cbl_amd.CBL.set_op(ga, gb, op)
    assert d.serialize() == exp.serialize() and ga.serialize() == ma.serialize() and gb.serialize() == mb.serialize()
    assert d.count() == exp.count() and d.num_buckets() == len(exp.buckets) and d.validate(False) == 0
    o = Oracle(k, pb, canonical)
    o.load(d.serialize())
    got = list(o.iter_words())
    kept = set(sm.algebra(op, wa, wb))
    assert set(got) == kept and len(got) == len(kept)
    dropped = sorted((wa | wb) - kept)[:500]
    if kept:
        assert d.contains_kmers([o.kmer_of_word(w) for w in sorted(kept)]).all()
    if dropped:
        assert not d.contains_kmers([o.kmer_of_word(w) for w in dropped]).any()
    assert list(d.iter()) == [o.kmer_of_word(w) for w in got]
    for g in (d, ga, gb):
        g.close()


# ---------------------------------------------------------------- 4f: the result is a first-class index
_FIRST_CLASS = {}
FIRST_CLASS_LENGTHS = (1, 1024, 1025, 5000)


def first_class_operands(k, pb):
    """Operands of REAL k-mers whose AND holds Vec buckets of 1, 1024, 1025 and 5000 words: the words of a seeded genome (query_shapes.genome:
    segments that steer where the necklaces start, so a small PREFIX_BITS fills several prefixes) grouped by prefix; the four most crowded prefixes
    give, for every length n, n shared words, a's own extras (a: a Trie) and b's own extras (b: a shuffled Vec). -> (genome, its words in k-mer
    order, a's buckets, b's buckets, the shared words)"""
    if (k, pb) not in _FIRST_CLASS:
        rng = random.Random(k * 100 + pb)
        sb, o = _sb(k, pb), Oracle(k, pb, False)
        G = qs.genome(21, 14000)
        words = o.seq_words(G)
        by = qs.candidates_by_prefix(words, sb)
        crowded = sorted(by, key=lambda p: (-len(by[p]), p))[:len(FIRST_CLASS_LENGTHS)]
        ba, bb, shared = {}, {}, set()
        mask = (1 << sb) - 1
        for p, n in zip(crowded, sorted(FIRST_CLASS_LENGTHS, reverse=True)):
            extra = min(1500, (len(by[p]) - n) // 2)
            assert extra >= 1, (k, pb, p, len(by[p]), n)
            pick = rng.sample(by[p], n + 2 * extra)
            both, xa, xb = pick[:n], pick[n:n + extra], pick[n + extra:]
            shared |= set(both)
            vb = [w & mask for w in both + xb]
            rng.shuffle(vb)
            ba[p], bb[p] = ("trie", sorted(w & mask for w in both + xa)), ("vec", vb)
        _FIRST_CLASS[(k, pb)] = (G, words, ba, bb, shared)
    return _FIRST_CLASS[(k, pb)]


def _kmers_as_stored(m: PyCBL, o: Oracle):
    """CBL::iter over a model index: prefixes ascending, every bucket in stored order"""
    sb = m.P["SB"]
    return [o.kmer_of_word((p << sb) | s) for p in sorted(m.buckets) for s in m.buckets[p][1]]


def _membership_agrees(g, m: PyCBL, o: Oracle, G, words, universe):
    """contains_seqs over the genome, contains_kmers on every word of `universe`, and kmers_np / iter against the model index `m`"""
    inside = sm.words(m)
    flags, total, positive = g.contains_seqs(np.frombuffer(G, dtype=np.uint8), np.array([0, len(G)], dtype=np.uint64))
    want = np.fromiter((w in inside for w in words), dtype=bool, count=len(words))
    assert total == len(words) and positive == int(want.sum())
    assert np.array_equal(np.asarray(flags).astype(bool)[:len(words)], want)
    kept, dropped = sorted(inside), sorted(universe - inside)
    assert kept and dropped
    assert g.contains_kmers([o.kmer_of_word(w) for w in kept]).all()  # every k-mer the algebra keeps
    assert not g.contains_kmers([o.kmer_of_word(w) for w in dropped]).any()  # ... and none it drops
    expect = _kmers_as_stored(m, o)
    assert len(set(expect)) == len(expect) == m.count()
    lo, hi = g.kmers_np()
    got = [int(x) for x in lo] if hi is None else [int(x) | (int(y) << 64) for x, y in zip(lo, hi)]
    assert got == expect
    assert list(g.iter()) == expect


@pytest.mark.parametrize("k,pb", [(15, 6), (31, 3)])  # SUFFIX_BITS 29 and 65 (wide)
def test_result_is_a_first_class_index(k, pb):
    G, words, ba, bb, shared = first_class_operands(k, pb)
    o = Oracle(k, pb, False)
    d, ga, gb, exp, ma, mb = _check(k, pb, False, ba, bb, "and", keep=True)
    assert sorted(len(v[1]) for v in exp.buckets.values()) == sorted(FIRST_CLASS_LENGTHS) and all(v[0] == "vec" for v in exp.buckets.values())
    assert sm.words(exp) == shared
    universe = sm.words(ma) | sm.words(mb)
    again = cbl_amd.CBL(k, pb)
    again.load(d.serialize())
    assert again.serialize() == exp.serialize()
    assert [(p_, kd, list(it)) for p_, kd, it in d.buckets()] == [(p_, 0, exp.buckets[p_][1]) for p_ in sorted(exp.buckets)]
    _membership_agrees(d, exp, o, G, words, universe)  # Vec buckets of 1, 1024, 1025 and 5000 words
    # an operator result works as an operand
    chain = cbl_amd.CBL.set_op(d, ga, "or")
    exp_chain = sm.set_op(exp, ma, "or")
    assert chain.serialize() == exp_chain.serialize() and d.serialize() == exp.serialize() and ga.serialize() == ma.serialize()
    assert (d | ga).serialize() == exp_chain.serialize()
    _membership_agrees(chain, exp_chain, o, G, words, universe)  # Vec buckets of up to 6500 words
    # ... and as the right side of the existing `|=`
    x = ga ^ gb
    mx = sm.set_op(ma, mb, "xor")
    assert x.serialize() == mx.serialize()
    _membership_agrees(x, mx, o, G, words, universe)
    ga |= x
    ma.merge(mx)
    assert ga.serialize() == ma.serialize() and x.serialize() == mx.serialize()
    assert ga.validate(False) == 0
    _membership_agrees(ga, ma, o, G, words, universe | {w for w in words if w not in universe and w % 7 == 0})


# ---------------------------------------------------------------- 4g: errors
def test_errors_leave_the_three_contexts_alone():
    _need_gpu()
    rng = random.Random(1)
    sb = _sb(31, 24)
    mk = lambda canonical=False, k=31, pb=24: _gpu(sm.from_buckets(k, pb, canonical, {7: ("vec", sm.distinct(rng, 5, min(sb, _sb(k, pb))))}))
    a, b, d = mk(), mk(), mk()
    before = [x.serialize() for x in (a, b, d)]
    L = cbl_amd.lib()

    def refused(dst, x, y, op=1, msg=None):
        rc = L.cblx_set_op(dst._h, x._h, y._h, op)
        assert rc == cbl_amd.EINVAL, rc
        if msg:
            assert msg in L.cblx_last_error(dst._h).decode()
        assert [g.serialize() for g in (a, b, d)] == before

    refused(a, a, b)
    refused(a, b, a)
    refused(d, a, a)
    refused(d, a, b, op=4)
    other_k, other_pb, canon = mk(k=33), mk(pb=20), mk(canonical=True)
    others = [x.serialize() for x in (other_k, other_pb, canon)]
    for odd in (other_k, other_pb):
        refused(d, a, odd)
        refused(d, odd, b)
        refused(odd, a, b)
    refused(d, a, canon, msg="One of the index is canonical while the other isn't")
    refused(d, canon, b, msg="One of the index is canonical while the other isn't")
    assert [x.serialize() for x in (other_k, other_pb, canon)] == others
    with pytest.raises(cbl_amd.CblxError) as e:
        cbl_amd.CBL.set_op(a, canon, "and", out=d)
    assert e.value.code == cbl_amd.EINVAL and "canonical" in str(e.value)
    with pytest.raises(ValueError):
        cbl_amd.CBL.set_op(a, b, "nand")
    for stmt in ("a &= b", "a -= b", "a ^= b"):
        with pytest.raises(NotImplementedError):
            exec(stmt, {"a": a, "b": b})
    assert [g.serialize() for g in (a, b, d)] == before
    out = cbl_amd.CBL.set_op(a, b, "or", out=d)  # `out` is overwritten
    assert out is d and d.count() == 10 and d.num_buckets() == 1


# ---------------------------------------------------------------- 4h: seeded sweep
@pytest.mark.parametrize("op", sm.OPS)
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
