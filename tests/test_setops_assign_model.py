"""CPU checks of the assigning set operations `a &= b`, `a -= b`, `a ^= b` (cblx_set_op_assign):
(a) the closed form of the Vec layout and the restatement the kernel computes — prefix counts of the deletion flags, next[] over the
    tail, pointer doubling — against remove_sorted_iter's literal replay (tests/setops_assign_model.py);
(b) the model: the set algebra, the count, which Vec buckets get sorted and which keep their order;
(c) the ABI: header, ctypes signatures, the Rust sys crate and facade name the new function."""
import itertools
import random
import re
from pathlib import Path

import pytest

import setops_assign_model as am
import setops_model as sm
from oracle.pyref import params

ROOT = Path(__file__).resolve().parent.parent
_ALGEBRA = {"and": set.__and__, "sub": set.__sub__, "xor": set.__xor__}


def _agree(v, D, cs):
    want = am.replay(v, D)
    assert am.swap_remove_closed_form(v, D) == want, (v, D)
    got, rounds = am.fixup_by_doubling(v, D, cs)
    assert got == want, (v, D, cs)
    return rounds


# ---------------------------------------------------------------- (a) the layout
def test_every_deletion_set_up_to_ten_words():
    for n in range(0, 11):
        v = list(range(100, 100 + n))
        for m in range(n + 1):
            for D in itertools.combinations(range(n), m):
                _agree(v, list(D), n)


def test_xor_shape_sorted_part_plus_pushed_part():
    """v = sorted a ++ ascending pushed words; deletions in the sorted part only"""
    for cs in range(0, 8):
        for ins in range(0, 5):
            v = list(range(100, 100 + cs)) + list(range(500, 500 + ins))
            for m in range(cs + 1):
                for D in itertools.combinations(range(cs), m):
                    _agree(v, list(D), cs)


@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 511, 512, 513, 1025, 1500])
def test_named_shapes(n):
    v = [7 * i + 1 for i in range(n)]
    for name, D in am.named_shapes(n).items():
        rounds = _agree(v, D, n)
        if name == "run_ending_at_n_minus_2" and n >= 63:
            assert rounds <= n.bit_length() + 1, "a chain of n - 2 hops settles in about log2 n rounds"
        for ins in (3, len(D) + 5):  # the `^=` shape on top
            _agree(v + [10 ** 6 + j for j in range(ins)], D, n)


def test_random_deletions():
    rng = random.Random(5)
    for _ in range(300):
        n = rng.choice([5, 40, 200, 1500])
        cs = rng.randint(0, n)
        frac = rng.choice([0.05, 0.5, 0.95, 1.0])
        D = [i for i in range(cs) if rng.random() < frac]
        _agree(list(range(n)), D, cs)


# ---------------------------------------------------------------- (b) the model
def _operands(rng, k=31, pb=8):
    bits = params(k, pb)["SB"]
    ba, bb = {}, {}
    for p in rng.sample(range(1 << pb), 40):
        na, nb = rng.choice([0, 1, 3, 40, 300]), rng.choice([0, 1, 3, 40, 300])
        if na == 0 and nb == 0:
            na = 2
        pool = sm.distinct(rng, na + nb, bits)
        A = pool[:na]
        share = int(rng.choice([0.0, 0.4, 1.0]) * min(na, nb))
        B = A[:share] + pool[na:na + nb - share]
        rng.shuffle(B)
        for side, items in ((ba, A), (bb, B)):
            if items:
                kind = rng.choice(["vec", "trie"])
                side[p] = (kind, sorted(items) if kind == "trie" else items)
    return sm.from_buckets(k, pb, False, ba), sm.from_buckets(k, pb, False, bb)


@pytest.mark.parametrize("op", am.OPS)
@pytest.mark.parametrize("seed", range(6))
def test_model_is_the_set_algebra_and_sorts_only_shared_vecs(op, seed):
    a, b = _operands(random.Random(seed))
    wa, wb = sm.words(a), sm.words(b)
    before_a = {p: (kd, list(it)) for p, (kd, it) in a.buckets.items()}
    before_b = {p: (kd, list(it)) for p, (kd, it) in b.buckets.items()}
    shared = set(before_a) & set(before_b)
    assert shared and set(before_a) - shared and set(before_b) - shared
    r = am.set_op_assign(a, b, op)
    assert r is a
    assert sm.words(a) == _ALGEBRA[op](wa, wb)
    assert a.count() == len(_ALGEBRA[op](wa, wb))
    assert sm.words(b) == wb and set(b.buckets) == set(before_b)
    assert all(items for _, items in a.buckets.values()), "an empty bucket leaves the index"
    for p, (kd, items) in b.buckets.items():
        assert kd == before_b[p][0]
        if p in shared and kd == "vec":
            assert items == sorted(before_b[p][1])  # iter_sorted, also where the result is empty
        else:
            assert items == before_b[p][1]
    for p, (kd, items) in a.buckets.items():
        if p in shared:
            assert kd == before_a[p][0]  # a's kind stays
            if kd == "trie":
                assert items == sorted(items)
        elif p in before_a:
            assert (kd, items) == before_a[p]  # untouched: not sorted
        else:
            assert op == "xor" and (kd, items) == before_b[p]  # cloned as stored


def test_model_bucket_rules():
    mk = lambda: (sm.from_buckets(31, 24, False, {1: ("vec", [9, 3, 5]), 2: ("vec", [7, 1]), 3: ("trie", [2, 4]), 5: ("vec", [8, 6, 1, 4])}),
                  sm.from_buckets(31, 24, False, {2: ("vec", [7, 1]), 3: ("vec", [4, 0]), 4: ("vec", [6, 5]), 5: ("trie", [1, 2])}))
    a, b = mk()
    am.set_op_assign(a, b, "xor")
    # 5: sorted [1, 4, 6, 8] ++ [2], then index 0 removed: the last word takes its place
    assert a.buckets == {1: ["vec", [9, 3, 5]], 3: ["trie", [0, 2]], 4: ["vec", [6, 5]], 5: ["vec", [2, 4, 6, 8]]}
    assert b.buckets[2] == ["vec", [1, 7]] and b.buckets[3] == ["vec", [0, 4]] and b.buckets[4] == ["vec", [6, 5]]
    a, b = mk()
    am.set_op_assign(a, b, "and")
    assert a.buckets == {2: ["vec", [1, 7]], 3: ["trie", [4]], 5: ["vec", [1]]}
    a, b = mk()
    am.set_op_assign(a, b, "sub")
    assert a.buckets == {1: ["vec", [9, 3, 5]], 3: ["trie", [2]], 5: ["vec", [8, 4, 6]]}


def test_assigning_and_operator_forms_hold_the_same_set():
    for op in am.OPS:
        a, b = _operands(random.Random(99))
        a2, b2 = _operands(random.Random(99))
        assert sm.words(am.set_op_assign(a, b, op)) == sm.words(sm.set_op(a2, b2, op))
        assert b.serialize() == b2.serialize()  # both forms leave b the same


# ---------------------------------------------------------------- (c) the ABI
def test_set_op_assign_is_declared_everywhere():
    import cbl_amd

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cblx.h").read_text(), flags=re.S)
    rs = (ROOT / "rust" / "cblx-sys" / "src" / "lib.rs").read_text()
    assert re.search(r"int cblx_set_op_assign\(cblx_ctx\* a, cblx_ctx\* b, uint32_t op\);", header)
    assert "cblx_set_op_assign" in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES["cblx_set_op_assign"][1]) == 3
    assert hasattr(cbl_amd.lib(), "cblx_set_op_assign")
    assert re.search(r"pub fn cblx_set_op_assign\(", rs)
    assert re.search(r"#define CBLX_ABI_VERSION 3\b", header)
    facade = (ROOT / "rust" / "cbl-gpu" / "src" / "lib.rs").read_text()
    for tr in ("BitAndAssign<&mut Self>", "SubAssign<&mut Self>", "BitXorAssign<&mut Self>"):
        assert "%s for CBL<K, T, PREFIX_BITS>" % tr in facade
    assert callable(getattr(cbl_amd.CBL, "set_op_assign"))
