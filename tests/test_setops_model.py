"""CPU checks of the set operations `a | b`, `a & b`, `a - b`, `a ^ b` (cblx_set_op):
(a) tests/setops_model.py — the expected bytes of every GPU test — against the C++ oracle where the two overlap;
(b) `k_bucket_setop`'s rounds (cbl_amd/csrc/kernels_setops.hpp) restated thread by thread, as tests/test_union_rounds_model.py does for the union: the
    two staging rings, the co-rank on the round's diagonal, the merge network, the origin of an output recovered from the candidates the thread
    still holds, the round's last output HELD BACK until its successor is known, the ordered compaction;
(c) the ABI: header, ctypes signatures and the Rust sys crate name the new function and its four constants."""
import random
import re
from pathlib import Path

import numpy as np
import pytest

import setops_model as sm
from cbl_amd import synth
from oracle import Oracle
from oracle.pyref import PyCBL

ROOT = Path(__file__).resolve().parent.parent
INF = (1 << 64) - 1
UNI_THREADS, UNI_ITEMS = 128, 4  # kernels_setops.hpp UNI_THREADS / UNI_ITEMS: the kernel's tile is their product


# ---------------------------------------------------------------- (a) the model against the oracle
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


@pytest.mark.parametrize("k,pb,canonical", [(11, 8, False), (15, 6, True), (31, 24, False)])
def test_model_or_into_an_empty_left_operand_is_the_merge(k, pb, canonical):
    seqs = _reads(3)
    b = _py(k, pb, canonical, seqs)
    via_model = sm.set_op(PyCBL(k, pb, canonical), b, "or")
    merged = PyCBL(k, pb, canonical)
    merged.merge(_py(k, pb, canonical, seqs))
    o, ob = Oracle(k, pb, canonical), Oracle(k, pb, canonical)
    for s in seqs:
        ob.insert_seq(s)
    o.merge(ob)
    assert sm.words(via_model) == sm.words(merged) == set(o.iter_words())
    assert via_model.serialize() == merged.serialize() == o.serialize()  # every bucket is cloned as stored


@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("k,pb,canonical,seed", [(11, 8, False, 1), (15, 6, True, 2), (31, 12, True, 3), (33, 10, False, 4)])
def test_model_results_load_into_the_oracle_as_the_set_algebra(op, k, pb, canonical, seed):
    seqs = _reads(seed, 16)
    a, b = _py(k, pb, canonical, seqs[:10]), _py(k, pb, canonical, seqs[6:])
    oa, ob = Oracle(k, pb, canonical), Oracle(k, pb, canonical)
    oa.load(a.serialize())
    ob.load(b.serialize())
    wa, wb = set(oa.iter_words()), set(ob.iter_words())
    assert wa & wb and wa - wb and wb - wa
    res = sm.set_op(a, b, op)
    o = Oracle(k, pb, canonical)
    o.load(res.serialize())
    got = list(o.iter_words())
    assert len(got) == len(set(got)) == res.count()
    assert set(got) == set(sm.algebra(op, wa, wb))
    # the operands keep their sets
    oa.load(a.serialize())
    ob.load(b.serialize())
    assert set(oa.iter_words()) == wa and set(ob.iter_words()) == wb


def test_model_bucket_rules():
    a = sm.from_buckets(31, 24, False, {1: ("vec", [9, 3, 5]), 2: ("vec", [7, 1]), 3: ("trie", [2, 4]), 5: ("vec", [8, 6])})
    b = sm.from_buckets(31, 24, False, {2: ("vec", [7, 1]), 3: ("vec", [4, 0]), 4: ("vec", [6, 5]), 5: ("trie", [1, 2])})
    r = sm.set_op(a, b, "xor")
    assert r.buckets == {1: ["vec", [9, 3, 5]], 3: ["vec", [0, 2]], 4: ["vec", [6, 5]], 5: ["vec", [1, 2, 6, 8]]}
    assert a.buckets[2] == ["vec", [1, 7]] and b.buckets[2] == ["vec", [1, 7]] and b.buckets[3] == ["vec", [0, 4]]  # sorted though the result is empty
    assert a.buckets[1] == ["vec", [9, 3, 5]] and b.buckets[4] == ["vec", [6, 5]]  # one-sided: untouched
    assert sm.set_op(a, b, "and").buckets == {2: ["vec", [1, 7]], 3: ["vec", [4]]}
    assert sm.set_op(a, b, "sub").buckets == {1: ["vec", [9, 3, 5]], 3: ["vec", [2]], 5: ["vec", [6, 8]]}
    assert sorted(sm.set_op(a, b, "or").buckets) == [1, 2, 3, 4, 5]


# ---------------------------------------------------------------- (b) the kernel's rounds
def pad(i):
    return i + (i >> 3)  # uni_pad


def keep_rule(op, eqp, eqn, from_a):
    return {"or": not eqp, "and": eqp, "xor": not eqp and not eqn, "sub": from_a and not eqp and not eqn}[op]


def setop_rounds(A, B, op, threads, items):
    T = threads * items
    assert T & (T - 1) == 0
    lds = [None] * (pad(2 * T) + 8)
    ra = lambda g: pad(g & (T - 1))
    rb = lambda g: pad(T + (g & (T - 1)))
    cs, co = len(A), len(B)
    ia = ib = ha = hb = 0
    out, loads = [], 0
    carry, have_carry, carry_eqp, carry_a = INF, False, False, False
    while ia < cs or ib < co:
        na, nb = min(cs - ia, T), min(co - ib, T)
        nout = min(na + nb, T)
        for g in range(ia + ha, ia + na):
            lds[ra(g)] = A[g]
            loads += 1
        for g in range(ib + hb, ib + nb):
            lds[rb(g)] = B[g]
            loads += 1
        i1 = []
        for tid in range(threads):
            d1 = min((tid + 1) * items, nout)
            lo, hi = max(d1 - nb, 0), min(d1, na)
            while lo < hi:
                mid = (lo + hi) >> 1
                if lds[ra(ia + mid)] <= lds[rb(ib + d1 - 1 - mid)]:
                    lo = mid + 1
                else:
                    hi = mid
            i1.append(lo)
        iend = i1[-1]
        outs, org = [None] * T, [0] * threads
        for tid in range(threads):
            d0 = min(tid * items, nout)
            i0 = i1[tid - 1] if tid else 0
            j0 = d0 - i0
            a = [lds[ra(ia + i0 + k)] if i0 + k < na else INF for k in range(items)]
            b = [lds[rb(ib + j0 + k)] if j0 + k < nb else INF for k in range(items)]
            o = [min(a[k], b[items - 1 - k]) for k in range(items)]
            st = items // 2
            while st >= 1:
                for k in range(items):
                    if (k & st) == 0 and o[k] > o[k + st]:
                        o[k], o[k + st] = o[k + st], o[k]
                st >>= 1
            from_a = i1[tid] - i0  # a[0 .. from_a) are the thread's outputs that came from A: an output equal to none of them came from B
            for k in range(items):
                outs[tid * items + k] = o[k]
                if any(j < from_a and o[k] == a[j] for j in range(items)):
                    org[tid] |= 1 << k
        oslot = lambda q: ra(ia + q) if q < iend else rb(ib + (q - iend))
        for q in range(nout):
            lds[oslot(q)] = outs[q]
        org_of = lambda q: bool((org[q // items] >> (q % items)) & 1)
        X = lambda q: lds[oslot(q)]
        # emit slot e holds output e - 1 (slot 0: the value held back), its successor is output e
        for e in range(nout):
            if e == 0 and not have_carry:
                continue
            v = X(e - 1) if e >= 1 else carry
            pred = X(e - 2) if e >= 2 else carry
            eqp = carry_eqp if e == 0 else ((e >= 2 or have_carry) and v == pred)
            from_a = carry_a if e == 0 else org_of(e - 1)
            if keep_rule(op, eqp, v == X(e), from_a):
                out.append(v)
        last = X(nout - 1)
        before = X(nout - 2) if nout >= 2 else carry
        carry_eqp = (nout >= 2 or have_carry) and last == before
        carry_a = org_of(nout - 1)
        carry, have_carry = last, True
        ha, hb = na - iend, nb - (nout - iend)
        ia += iend
        ib += nout - iend
    if have_carry and keep_rule(op, carry_eqp, False, carry_a):
        out.append(carry)
    return out, loads


def test_straddling_lists_put_a_pair_on_every_round_boundary():
    T = 16
    for na, nb in ((T, T), (T - 1, T + 1), (2 * T + 1, 2 * T + 1), (1, 2 * T + 1), (T + 1, T - 1)):
        A, B = sm.straddling_lists(na, nb, T)
        merged = sorted([(v, 0) for v in A] + [(v, 1) for v in B])
        for q in range(1, (na + nb) // T + 1):
            if q * T < na + nb and q <= min(na, nb):
                assert merged[q * T - 1][0] == merged[q * T][0] and merged[q * T - 1][1] == 0, (na, nb, q)
        assert len(set(A) & set(B)) == min(len([q for q in range(1, (na + nb) // T + 1) if q * T < na + nb]), na, nb)


@pytest.mark.parametrize("op", sm.OPS)
@pytest.mark.parametrize("threads,items", [(8, 4), (2, 4), (16, 2), (UNI_THREADS, UNI_ITEMS)])
def test_rounds_give_the_sorted_set_algebra(op, threads, items):
    rng = random.Random(threads * 100 + items)
    T = threads * items
    shapes = [(0, 5), (5, 0), (1, 1), (T, T), (T - 1, T + 1), (T - 1, 1), (1, T), (2 * T + 1, 2 * T + 1), (3 * T + 7, 2 * T - 3), (6 * T, 13), (13, 6 * T)]
    for na, nb in shapes:
        cases = [sm.random_lists(rng, na, nb, sh) for sh in (0, min(na, nb) // 3, min(na, nb))]  # none shared, some, as many as fit
        cases.append(sm.straddling_lists(na, nb, T, rng))
        if na == nb and na:
            A, _ = sm.random_lists(rng, na, 0, 0)
            cases.append((A, list(A)))  # every value shared
        for A, B in cases:
            got, loads = setop_rounds(A, B, op, threads, items)
            assert got == sm.algebra(op, A, B), (op, threads, items, na, nb)
            assert loads == len(A) + len(B), "every word is staged exactly once"


@pytest.mark.parametrize("op", sm.OPS)
def test_rounds_with_sentinel_valued_words(op):
    # all-ones pads the candidate fetch and is a legal suffix at SUFFIX_BITS = 64; 0 and the top / bottom bit neighbours ride along
    top = 1 << 63
    A = [0, 1, top - 1, top, INF - 1, INF]
    for B in ([INF], [0, INF], [1, top, INF - 1], [0, 1, top - 1, top, INF - 1, INF], [2, top + 1]):
        for threads in (2, 8):
            assert setop_rounds(A, B, op, threads, 4)[0] == sm.algebra(op, A, B)
            assert setop_rounds(B, A, op, threads, 4)[0] == sm.algebra(op, B, A)


# ---------------------------------------------------------------- (c) the ABI
def test_set_op_is_declared_everywhere():
    import cbl_amd

    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cblx.h").read_text(), flags=re.S)
    rs = (ROOT / "rust" / "cblx-sys" / "src" / "lib.rs").read_text()
    assert re.search(r"int cblx_set_op\(cblx_ctx\* dst, cblx_ctx\* a, cblx_ctx\* b, uint32_t op\);", header)
    assert "cblx_set_op" in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES["cblx_set_op"][1]) == 4
    assert hasattr(cbl_amd.lib(), "cblx_set_op")
    assert re.search(r"pub fn cblx_set_op\(", rs)
    for name, val in (("OR", 0), ("AND", 1), ("SUB", 2), ("XOR", 3)):
        assert re.search(r"#define CBLX_SETOP_%s %d\b" % (name, val), header)
        assert re.search(r"pub const CBLX_SETOP_%s: u32 = %d;" % (name, val), rs)
        assert cbl_amd.SETOPS[name.lower()] == val
    assert re.search(r"#define CBLX_ABI_VERSION 3\b", header)
    facade = (ROOT / "rust" / "cbl-gpu" / "src" / "lib.rs").read_text()
    for tr in ("BitAnd<Self>", "Sub<Self>", "BitXor<Self>", "BitOr<Self>"):
        assert "%s for &mut CBL<K, T, PREFIX_BITS>" % tr in facade
