"""CPU checks of the n-ary set operations CBL.merge / CBL.intersect (cblx_set_op_many):
(a) tests/setops_many_model.py — the expected bytes of every GPU test — as sets, against tests/setops_model.py at n = 2, and where it differs from a
    FOLD of the binary operation (the reason the n-ary form is no fold);
(b) the short route of `k_bucket_setop_many` (cbl_amd/csrc/kernels_setops.hpp) restated thread by thread: the merged position by binary searches with the
    `<=` / `<` tie rule, the kept flags, the ordered compaction; the search over the shortest run for intersect;
(c) the ABI: header, ctypes signatures, the Rust crates, and the thresholds the GPU tests mirror."""
import itertools
import random
import re
from pathlib import Path

import numpy as np
import pytest

import setops_many_model as mm
import setops_model as sm
from cbl_amd import synth
from oracle.pyref import PyCBL

ROOT = Path(__file__).resolve().parent.parent


def _reads(seed, n=12, length=120):
    bases, offsets = synth.reads(seed, n, length)
    b = bytes(np.asarray(bases, dtype=np.uint8))
    off = [int(x) for x in offsets]
    return [b[off[i]:off[i + 1]] for i in range(len(off) - 1)]


def _py(k, pb, canonical, seqs):
    c = PyCBL(k, pb, canonical)
    for s in seqs:
        c.insert_seq(s)
    return c


def _copy(c: PyCBL) -> PyCBL:
    return sm.from_buckets(c.P["K"], c.P["PB"], c.canonical, {p: (kd, it) for p, (kd, it) in c.buckets.items()})


# ---------------------------------------------------------------- (a) the model
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("k,pb,canonical", [(11, 8, False), (15, 6, True), (31, 12, False), (33, 8, True)])
def test_model_is_the_set_algebra(n, k, pb, canonical):
    seqs = _reads(n * 10 + k, 6 + 4 * n)
    ops = [_py(k, pb, canonical, seqs[4 * i:4 * i + 10]) for i in range(n)]
    sets = [sm.words(x) for x in ops]
    u, i_ = mm.merge(ops), mm.intersect(ops)
    assert sm.words(u) == set().union(*sets) and u.count() == len(set().union(*sets))
    assert sm.words(i_) == set.intersection(*sets) and i_.count() == len(set.intersection(*sets))
    assert [sm.words(x) for x in ops] == sets  # the operands keep their sets
    assert all(v[1] for v in i_.buckets.values())  # no empty bucket stays


@pytest.mark.parametrize("op", ["or", "and"])
@pytest.mark.parametrize("k,pb,canonical,seed", [(11, 8, False, 1), (15, 6, True, 2), (31, 12, True, 3), (33, 10, False, 4)])
def test_model_at_two_operands_is_the_binary_model(op, k, pb, canonical, seed):
    seqs = _reads(seed, 16)
    a, b = _py(k, pb, canonical, seqs[:10]), _py(k, pb, canonical, seqs[6:])
    a2, b2 = _copy(a), _copy(b)
    many, two = mm.MANY[op]([a, b]), sm.set_op(a2, b2, op)
    assert many.serialize() == two.serialize()
    assert a.serialize() == a2.serialize() and b.serialize() == b2.serialize()


def _three(b0, b1, b2):
    return [sm.from_buckets(31, 24, False, b) for b in (b0, b1, b2)]


def test_merge_is_not_a_fold():
    """prefix 5 is held by operands 0 and 2 only, operand 0's Vec unsorted: the n-ary merge sorts operand 0's Vec (two holders), the fold
    ((a | b) | c) clones it into the temporary first and never sorts a's own Vec"""
    mk = lambda: _three({5: ("vec", [9, 3, 7])}, {6: ("vec", [2, 1])}, {5: ("vec", [8, 3])})
    ops = mk()
    res = mm.merge(ops)
    assert ops[0].buckets[5] == ["vec", [3, 7, 9]] and ops[2].buckets[5] == ["vec", [3, 8]] and ops[1].buckets[6] == ["vec", [2, 1]]
    assert res.buckets == {5: ["vec", [3, 7, 8, 9]], 6: ["vec", [2, 1]]}
    f = mk()
    folded = sm.set_op(sm.set_op(f[0], f[1], "or"), f[2], "or")
    assert f[0].buckets[5] == ["vec", [9, 3, 7]]  # the fold leaves a's Vec as stored
    assert f[0].serialize() != ops[0].serialize()
    assert sm.words(folded) == sm.words(res) and folded.serialize() == res.serialize()  # (here the results agree; the operands do not)
    assert f[2].serialize() == ops[2].serialize()


def test_intersect_is_not_a_fold():
    """prefix 5 is held by operands 0 and 1 but not 2: the n-ary intersect never visits it, the fold (a & b) & c sorts a's and b's Vecs there"""
    mk = lambda: _three({5: ("vec", [9, 3, 7]), 6: ("vec", [4, 1])}, {5: ("vec", [7, 2]), 6: ("vec", [1, 0])}, {6: ("vec", [5, 1])})
    ops = mk()
    res = mm.intersect(ops)
    assert ops[0].buckets[5] == ["vec", [9, 3, 7]] and ops[1].buckets[5] == ["vec", [7, 2]]  # not visited
    assert [x.buckets[6] for x in ops] == [["vec", [1, 4]], ["vec", [0, 1]], ["vec", [1, 5]]]
    assert res.buckets == {6: ["vec", [1]]}
    f = mk()
    folded = sm.set_op(sm.set_op(f[0], f[1], "and"), f[2], "and")
    assert f[0].buckets[5] == ["vec", [3, 7, 9]] and f[1].buckets[5] == ["vec", [2, 7]]  # the fold sorted them
    assert f[0].serialize() != ops[0].serialize() and f[1].serialize() != ops[1].serialize()
    assert folded.serialize() == res.serialize() and f[2].serialize() == ops[2].serialize()


def test_one_operand():
    b = {1: ("vec", [5, 2, 9]), 2: ("trie", [1, 4, 6]), 3: ("vec", [7])}
    a = sm.from_buckets(31, 24, False, b)
    before = a.serialize()
    m = mm.merge([a])
    assert m.serialize() == before == a.serialize() and m is not a  # the identity: every bucket has one holder
    i_ = mm.intersect([a])
    assert i_.buckets == {1: ["vec", [2, 5, 9]], 2: ["vec", [1, 4, 6]], 3: ["vec", [7]]}  # Tries become Vecs
    assert a.buckets == {1: ["vec", [2, 5, 9]], 2: ["trie", [1, 4, 6]], 3: ["vec", [7]]}  # ... and a's Vecs are sorted


def test_empty_operands():
    a = sm.from_buckets(31, 24, False, {1: ("vec", [5, 2]), 2: ("vec", [3, 1])})
    b = sm.from_buckets(31, 24, False, {1: ("vec", [9, 5])})
    e = PyCBL(31, 24, False)
    before = [a.serialize(), b.serialize()]
    assert mm.intersect([a, e, b]).buckets == {} and [a.serialize(), b.serialize()] == before  # nothing is visited
    a2, b2 = _copy(a), _copy(b)
    assert mm.merge([a, e, b]).serialize() == mm.merge([a2, b2]).serialize() and a.serialize() == a2.serialize() and b.serialize() == b2.serialize()
    assert mm.merge([e]).buckets == {} and mm.intersect([e]).buckets == {}


# ---------------------------------------------------------------- (b) the kernel's short route
def _check_runs(runs):
    want_or = sorted(set(v for r in runs for v in r))
    want_and = sorted(set.intersection(*(set(r) for r in runs)))
    assert mm.or_short_route(runs) == want_or, runs
    assert mm.and_short_route(runs) == want_and, runs
    # the copy that is kept is the LOWEST holder's
    for k, row in enumerate(mm.or_positions(runs)):
        for j, (_, kept) in enumerate(row):
            assert kept == all(runs[k][j] not in runs[kk] for kk in range(k))


@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_short_route_on_every_multiset_of_multiplicities(m):
    """up to 6 values, every value held by 1 .. m of the m runs, every tuple of multiplicities: with EVERY choice of holder sets while those are at most
    50 000 ((2^m - 1)^values), beyond that with the lowest holders, the highest holders and two seeded choices per tuple. Runs that stay empty are skipped."""
    masks = range(1, 1 << m)
    by_mult = {c: [x for x in masks if bin(x).count("1") == c] for c in range(1, m + 1)}
    rng = random.Random(m)
    seen = 0

    def run_case(assign):
        runs = [[10 * v for v in range(len(assign)) if (assign[v] >> k) & 1] for k in range(m)]
        if all(runs):
            _check_runs(runs)
            return 1
        return 0

    for nv in range(1, 7):
        if (len(masks)) ** nv <= 50000:
            for assign in itertools.product(masks, repeat=nv):
                seen += run_case(assign)
        else:
            for mult in itertools.product(range(1, m + 1), repeat=nv):
                seen += run_case([by_mult[c][0] for c in mult]) + run_case([by_mult[c][-1] for c in mult])
                for _ in range(2):
                    seen += run_case([rng.choice(by_mult[c]) for c in mult])
    assert seen > 0


def test_short_route_on_random_runs():
    rng = random.Random(5)
    for _ in range(300):
        m = rng.randint(1, 8)
        bits = rng.choice([3, 6, 64])
        pool = sm.distinct(rng, min(40, 1 << bits), bits) + [0, (1 << bits) - 1]
        runs = [sorted(set(rng.sample(pool, rng.randint(1, min(len(pool), 30))))) for _ in range(m)]
        _check_runs(runs)


# ---------------------------------------------------------------- (c) the ABI
def test_set_op_many_is_declared_everywhere():
    import cbl_amd

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cblx.h").read_text(), flags=re.S)
    rs = (ROOT / "rust" / "cblx-sys" / "src" / "lib.rs").read_text()
    assert re.search(r"int cblx_set_op_many\(cblx_ctx\* dst, cblx_ctx\* const\* srcs, uint32_t n, uint32_t op\);", header)
    assert re.search(r"#define CBLX_SETOP_MAX_OPERANDS 64\b", header)
    assert re.search(r"pub const CBLX_SETOP_MAX_OPERANDS: u32 = 64;", rs)
    assert mm.MAX_OPERANDS == 64
    assert "cblx_set_op_many" in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES["cblx_set_op_many"][1]) == 4
    assert hasattr(cbl_amd.lib(), "cblx_set_op_many")
    assert re.search(r"pub fn cblx_set_op_many\(", rs)
    assert re.search(r"#define CBLX_ABI_VERSION 3\b", header)
    assert "cblx_set_op_many" in (ROOT / "include" / "cblx.h").read_text().split("#define CBLX_ABI_VERSION")[0]  # the "Added under 3" note
    facade = (ROOT / "rust" / "cbl-gpu" / "src" / "lib.rs").read_text()
    assert re.search(r"pub fn merge\(cbls: Vec<&mut Self>\) -> Self", facade) and re.search(r"pub fn intersect\(cbls: Vec<&mut Self>\) -> Self", facade)
    assert callable(cbl_amd.CBL.merge) and callable(cbl_amd.CBL.intersect)


def test_python_refuses_before_the_call():
    import cbl_amd

    with pytest.raises(ValueError):
        cbl_amd.CBL.merge([])
    with pytest.raises(ValueError):
        cbl_amd.CBL.intersect([])
    x = object()
    with pytest.raises(ValueError):
        cbl_amd.CBL.merge([x, x])
    with pytest.raises(ValueError):
        cbl_amd.CBL.intersect([x, x])


def test_thresholds_the_gpu_tests_mirror():
    src = (ROOT / "cbl_amd" / "csrc" / "kernels_setops.hpp").read_text()
    m = re.search(r"static const u32 MANY_SMALL = (\d+), MANY_LDS = (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (mm.MANY_SMALL, mm.MANY_LDS)
    assert re.search(r"static const u32 MANY_MAX = 64;", src)
