"""CPU checks of `CBL.at_least` / `CBL.occupancy` (cblx_set_at_least / cblx_occupancy_counts):
(a) tests/threshold_model.py — the expected bytes of every GPU test — against tests/setops_many_model.py at both ends (t = 1 is merge, t = n is
    intersect), against a brute-force collections.Counter, and where it differs from any fold of binary operations;
(b) the occupancy identities;
(c) the kernels restated thread by thread: the short route's (position, kept, holders), the long route's rounds, the vertical counter;
(d) the Python-level argument errors, raised without a GPU, and the ABI: header, ctypes signatures, the Rust declarations."""
import itertools
import random
import re
from collections import Counter
from pathlib import Path

import numpy as np
import pytest

import cbl_amd
import setops_many_model as mm
import setops_model as sm
import threshold_model as tm
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


def _operands(n, k, pb, canonical):
    seqs = _reads(n * 10 + k, 6 + 4 * n)
    return [_py(k, pb, canonical, seqs[4 * i:4 * i + 10]) for i in range(n)]


# ---------------------------------------------------------------- (a) the model
@pytest.mark.parametrize("n", [1, 2, 3, 5])
@pytest.mark.parametrize("k,pb,canonical", [(11, 8, False), (15, 6, True), (31, 12, False), (33, 8, True)])
def test_both_ends_are_merge_and_intersect(n, k, pb, canonical):
    ops = _operands(n, k, pb, canonical)
    a, b = [_copy(x) for x in ops], [_copy(x) for x in ops]
    assert tm.at_least(a, 1).serialize() == mm.merge(b).serialize()
    assert [x.serialize() for x in a] == [x.serialize() for x in b]
    if n >= 2:
        a, b = [_copy(x) for x in ops], [_copy(x) for x in ops]
        assert tm.at_least(a, n).serialize() == mm.intersect(b).serialize()
        assert [x.serialize() for x in a] == [x.serialize() for x in b]


@pytest.mark.parametrize("n", [2, 3, 5])
@pytest.mark.parametrize("k,pb,canonical", [(11, 8, False), (15, 6, True), (31, 12, False), (33, 8, True)])
def test_every_threshold_is_the_counter(n, k, pb, canonical):
    ops = _operands(n, k, pb, canonical)
    sets = [sm.words(x) for x in ops]
    held = Counter(w for s in sets for w in s)
    for t in range(1, n + 1):
        xs = [_copy(x) for x in ops]
        res = tm.at_least(xs, t)
        want = {w for w, c in held.items() if c >= t}
        assert sm.words(res) == want and res.count() == len(want)
        assert [sm.words(x) for x in xs] == sets  # the operands keep their sets
        assert all(v[1] for v in res.buckets.values())  # no empty bucket stays
        if t >= 2:
            assert all(v[0] == "vec" and v[1] == sorted(v[1]) for v in res.buckets.values())
    xs = [_copy(x) for x in ops]
    hist = tm.occupancy(xs)
    assert hist == [sum(1 for c in held.values() if c == j) for j in range(n + 1)] and hist[0] == 0
    assert [sm.words(x) for x in xs] == sets
    m = [_copy(x) for x in ops]
    mm.merge(m)
    assert [x.serialize() for x in xs] == [x.serialize() for x in m]  # occupancy leaves the operands as merge does


def _four(*bs):
    return [sm.from_buckets(31, 24, False, b) for b in bs]


def test_rules_per_prefix():
    """prefix 5: three holders; prefix 6: two; prefix 7: one. At t = 2 prefix 7 is not visited (its Vec stays as stored), at t = 3 prefix 6 is not either."""
    mk = lambda: _four({5: ("vec", [9, 3, 7]), 6: ("vec", [4, 1]), 7: ("vec", [8, 2])}, {5: ("trie", [3, 7, 8]), 6: ("vec", [1, 0])}, {5: ("vec", [7, 3, 1])}, {})
    ops = mk()
    res = tm.at_least(ops, 2)
    assert res.buckets == {5: ["vec", [3, 7]], 6: ["vec", [1]]}
    assert ops[0].buckets == {5: ["vec", [3, 7, 9]], 6: ["vec", [1, 4]], 7: ["vec", [8, 2]]}
    assert ops[1].buckets == {5: ["trie", [3, 7, 8]], 6: ["vec", [0, 1]]} and ops[2].buckets == {5: ["vec", [1, 3, 7]]} and ops[3].buckets == {}
    ops = mk()
    res = tm.at_least(ops, 3)
    assert res.buckets == {5: ["vec", [3, 7]]}
    assert ops[0].buckets == {5: ["vec", [3, 7, 9]], 6: ["vec", [4, 1]], 7: ["vec", [8, 2]]} and ops[1].buckets[6] == ["vec", [1, 0]]
    ops = mk()
    assert tm.at_least(ops, 4).buckets == {} and [x.serialize() for x in ops] == [x.serialize() for x in mk()]  # four operands, three non-empty
    ops = mk()
    assert tm.occupancy(ops) == [0, 2 + 3 + 2, 1, 2, 0]  # prefix 7's two words from the directory; 5: {9, 8, 1} once, {3, 7} thrice; 6: {4, 0} once, {1} twice
    assert ops[0].buckets[7] == ["vec", [8, 2]] and ops[0].buckets[5] == ["vec", [3, 7, 9]] and ops[1].buckets[6] == ["vec", [0, 1]]


def test_it_is_not_a_fold():
    """A fold of binary operations forgets how many operands held a value. Every region of the Venn diagram holds one value: 1, 2, 3 one holder each,
    4 = a and b, 5 = a and c, 6 = b and c, 7 all. No bracketing of |, &, -, ^ over (a, b, c) in order gives {4, 5, 6, 7}."""
    a, b, c = {5: ("vec", [7, 1, 5, 4])}, {5: ("vec", [6, 2, 7, 4])}, {5: ("vec", [3, 7, 6, 5])}
    ops = _four(a, b, c)
    res = tm.at_least(ops, 2)
    assert res.buckets == {5: ["vec", [4, 5, 6, 7]]}
    sets = [sm.words(x) for x in _four(a, b, c)]
    want = sm.words(res)
    ALG = {"or": set.union, "and": set.intersection, "sub": set.difference, "xor": set.symmetric_difference}
    for o1, o2 in itertools.product(ALG, repeat=2):
        assert ALG[o2](ALG[o1](sets[0], sets[1]), sets[2]) != want
        assert ALG[o1](sets[0], ALG[o2](sets[1], sets[2])) != want
    # with the pairwise intersections merged ((a & b) | (a & c) | (b & c): not a fold of the operands) the SET agrees, the result's bytes need not
    f = _four(a, b, c)
    pairs = [sm.set_op(f[i], f[j], "and") for i, j in ((0, 1), (0, 2), (1, 2))]
    assert sm.words(mm.merge(pairs)) == want


# ---------------------------------------------------------------- (b) the identities
@pytest.mark.parametrize("n", [1, 2, 3, 4, 6])
def test_occupancy_identities(n):
    ops = _operands(n, 15, 6, n % 2 == 0)
    counts = [x.count() for x in ops]
    hist = tm.occupancy([_copy(x) for x in ops])
    assert len(hist) == n + 1 and hist[0] == 0
    assert sum(j * h for j, h in enumerate(hist)) == sum(counts)
    assert sum(hist) == mm.merge([_copy(x) for x in ops]).count()
    assert hist[n] == mm.intersect([_copy(x) for x in ops]).count()
    if n == 2:
        assert hist[2] == len(sm.words(ops[0]) & sm.words(ops[1]))
    for t in range(1, n + 1):
        assert tm.at_least([_copy(x) for x in ops], t).count() == sum(hist[t:])


def test_empty_operands_count_towards_n():
    a = sm.from_buckets(31, 24, False, {1: ("vec", [5, 2]), 2: ("vec", [3, 1])})
    b = sm.from_buckets(31, 24, False, {1: ("vec", [9, 5])})
    e = PyCBL(31, 24, False)
    before = [a.serialize(), b.serialize()]
    assert tm.at_least([a, e, b], 3).buckets == {} and [a.serialize(), b.serialize()] == before  # nothing is visited
    assert tm.at_least([a, e, b], 2).buckets == {1: ["vec", [5]]} and a.buckets[1] == ["vec", [2, 5]] and a.buckets[2] == ["vec", [3, 1]]
    assert tm.occupancy([a, e, b]) == [0, 4, 1, 0]
    assert tm.occupancy([e]) == [0, 0] and tm.at_least([e], 1).buckets == {}


# ---------------------------------------------------------------- (c) the kernels, thread by thread
def _check_runs(runs):
    held = Counter(v for r in runs for v in r)
    m = len(runs)
    for t in range(1, m + 1):
        want = sorted(v for v, c in held.items() if c >= t)
        assert tm.short_route(runs, t) == want, (runs, t)
        for cap in (m, m + 1, 2 * m + 1, 16, tm.MANY_LDS):
            if cap >= m:
                assert tm.long_route(runs, t, cap) == want, (runs, t, cap)
    assert tm.short_route(runs, 1) == mm.or_short_route(runs)
    assert tm.short_tally(runs) == tm.long_tally(runs, m) == tm.long_tally(runs, 7 * m) == [sum(1 for c in held.values() if c == j) for j in range(m + 1)]
    for k, row in enumerate(tm.short_elements(runs, 1)):
        for j, (pos, kept, h) in enumerate(row):
            assert h == held[runs[k][j]]
            assert kept == all(runs[k][j] not in runs[kk] for kk in range(k))  # the copy that counts is the LOWEST holder's
            assert pos == mm.or_positions(runs)[k][j][0]


def test_routes_exhaustive_small():
    """every choice of up to three runs over four values"""
    subsets = [sorted(s) for r in range(1, 5) for s in itertools.combinations(range(4), r)]
    for m in (1, 2, 3):
        for runs in itertools.product(subsets, repeat=m):
            _check_runs(list(runs))


@pytest.mark.parametrize("seed", range(12))
def test_routes_seeded(seed):
    rng = random.Random(seed)
    m = rng.randint(2, 9)
    pool = sm.distinct(rng, 60, rng.choice([6, 24, 64, 65]))
    runs = [sorted(rng.sample(pool, rng.randint(1, 40))) for _ in range(m)]
    runs[rng.randrange(m)] = sorted(pool[:1])  # a run of one word
    _check_runs(runs)


def test_long_rounds():
    """the windows, the limit and what a round settles: the run that sets the limit gives up its whole window, a value the limit excludes waits"""
    runs = [[1, 2, 3, 9], [2, 4, 5, 6, 7, 8], [9]]
    rounds = tm.long_rounds(runs, cap=6)  # two words of every run
    assert rounds[0] == ([[1, 2], [2, 4], [9]], [2, 1, 0])  # limit 2 (run 0 and run 1 go beyond their windows, run 2 does not)
    assert rounds[1] == ([[3, 9], [4, 5], [9]], [1, 2, 0])  # limit 5 (only run 1 goes beyond)
    assert rounds[2] == ([[9], [6, 7], [9]], [0, 2, 0])  # limit 7
    assert rounds[3] == ([[9], [8], [9]], [1, 1, 1]) and len(rounds) == 4  # nobody goes beyond: the last round takes everything
    assert tm.long_route(runs, 2, cap=6) == [2, 9] and tm.long_tally(runs, cap=6) == [0, 7, 2, 0]
    for windows, act in tm.long_rounds([list(range(0, 9000, 3)), list(range(0, 9000, 2)), [5, 6]]):
        assert sum(map(len, windows)) <= tm.MANY_LDS
    assert tm.long_route([list(range(0, 9000, 3)), list(range(0, 9000, 2)), [5, 6]], 2) == sorted(set(range(0, 9000, 6)) | {6})


def test_lowest_copy_not_in_the_first_run():
    runs = [[1, 5], [2, 5, 8], [2, 8, 9]]
    assert tm.short_route(runs, 2) == tm.long_route(runs, 2) == [2, 5, 8]
    assert tm.short_elements(runs, 2)[1][0][1:] == (True, 2) and tm.short_elements(runs, 2)[2][0][1:] == (False, 2)
    assert tm.short_route(runs, 3) == [] and tm.short_tally(runs) == [0, 2, 3, 0]


@pytest.mark.parametrize("n", [1, 2, 3, 7, 63, 64])
def test_vertical_counter(n):
    rng = random.Random(n)
    words = [rng.getrandbits(64) for _ in range(n)] if n < 63 else [rng.getrandbits(64) | rng.getrandbits(64) | (1 << 17) for _ in range(n)]
    for t in sorted({1, 2, max(1, n // 2), max(1, n - 1), n}):
        want = sum(1 << b for b in range(64) if sum((w >> b) & 1 for w in words) >= t)
        assert tm.candidates_word(words, t) == want, (n, t)


def test_capacity_rule():
    """every output consumes t staged words or more: sum // t bounds the kept elements"""
    rng = random.Random(5)
    for _ in range(200):
        m = rng.randint(2, 6)
        runs = [sorted(rng.sample(range(12), rng.randint(1, 12))) for _ in range(m)]
        for t in range(2, m + 1):
            assert len(tm.short_route(runs, t)) <= sum(map(len, runs)) // t


# ---------------------------------------------------------------- (d) errors without a GPU, and the ABI
def test_python_argument_errors():
    x, y = object(), object()  # refused before anything is asked of an operand
    for bad in ([], [x, x], [x, y, x]):
        with pytest.raises(ValueError):
            cbl_amd.CBL.at_least(bad, 1)
        with pytest.raises(ValueError):
            cbl_amd.CBL.occupancy(bad)
    for t in (0, 3, -1):
        with pytest.raises(ValueError):
            cbl_amd.CBL.at_least([x, y], t)


def test_occupancy_report_is_pure():
    from cbl_amd.__main__ import occupancy_report

    lines, human = occupancy_report(np.array([0, 8, 1, 2], dtype=np.uint64))
    assert lines == ["1\t8", "2\t1", "3\t2"]
    assert "11 distinct" in human[0] and human[1].startswith("2 are held by all")
    with pytest.raises(ValueError):
        occupancy_report([1, 2])


def test_abi_declares_the_entry_points():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cblx.h").read_text(), flags=re.S)
    assert re.search(r"int cblx_set_at_least\(cblx_ctx\* dst, cblx_ctx\* const\* srcs, uint32_t n, uint32_t t\);", header)
    assert re.search(r"int cblx_occupancy_counts\(cblx_ctx\* const\* srcs, uint32_t n, uint64_t\* hist\);", header)
    assert "#define CBLX_ABI_VERSION 3" in header
    assert len(cbl_amd.SIGNATURES["cblx_set_at_least"][1]) == 4 and len(cbl_amd.SIGNATURES["cblx_occupancy_counts"][1]) == 3
    rs = (ROOT / "rust" / "cblx-sys" / "src" / "lib.rs").read_text()
    assert "pub fn cblx_set_at_least(dst: *mut cblx_ctx, srcs: *const *mut cblx_ctx, n: u32, t: u32) -> c_int;" in rs
    assert "pub fn cblx_occupancy_counts(srcs: *const *mut cblx_ctx, n: u32, hist: *mut u64) -> c_int;" in rs
    assert cbl_amd.SETOPS == {"or": 0, "and": 1, "sub": 2, "xor": 3}
    src = (ROOT / "cbl_amd" / "csrc" / "kernels_setops.hpp").read_text()
    assert "static const u32 MANY_SMALL = %d, MANY_LDS = %d;" % (tm.MANY_SMALL, tm.MANY_LDS) in src
