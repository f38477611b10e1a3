"""The reference's operator forms `&mut a & &mut b`, `-`, `^`, `|` restated on `oracle.pyref.PyCBL.buckets` (prefix -> [kind, items]) — a helper, not a
test file. /root/reference/src/wordset/set_ops.rs:78-121, 159-190, 241-279, 319-364 walk the two prefix sets, src/trievec/set_ops.rs:5-41, 73-99,
131-161, 189-224 the buckets:
  * a bucket one side holds is CLONED as stored, kind and order kept: AND keeps none, SUB only the left operand's, XOR and OR both sides';
  * a bucket both sides hold goes through `iter_sorted` on either side, which sorts a Vec IN PLACE (the operands are `&mut`), and becomes
    `TrieOrVec::Vec(result)`: always a Vec, ascending, whatever its length — dropped when empty.
`set_op` returns a new PyCBL and mutates its operands the way the reference does; `PyCBL.serialize()` then gives the expected bytes of all three."""
import random

from oracle.pyref import PyCBL

OPS = ("or", "and", "sub", "xor")
_ALGEBRA = {"or": set.__or__, "and": set.__and__, "sub": set.__sub__, "xor": set.__xor__}


def algebra(op, a, b):
    """sorted(a OP b) of two iterables of distinct values"""
    return sorted(_ALGEBRA[op](set(a), set(b)))


def set_op(a: PyCBL, b: PyCBL, op: str) -> PyCBL:
    assert op in OPS
    assert a.canonical == b.canonical, "One of the index is canonical while the other isn't"
    assert (a.P["K"], a.P["PB"]) == (b.P["K"], b.P["PB"])
    res = PyCBL(a.P["K"], a.P["PB"], a.canonical)
    for p in sorted(set(a.buckets) | set(b.buckets)):
        in_a, in_b = p in a.buckets, p in b.buckets
        if in_a and in_b:
            for side in (a, b):
                if side.buckets[p][0] == "vec":
                    side.buckets[p][1].sort()
            items = algebra(op, a.buckets[p][1], b.buckets[p][1])
            if items:
                res.buckets[p] = ["vec", items]
        elif in_a and op != "and":
            res.buckets[p] = [a.buckets[p][0], list(a.buckets[p][1])]
        elif in_b and op in ("or", "xor"):
            res.buckets[p] = [b.buckets[p][0], list(b.buckets[p][1])]
    return res


def from_buckets(k, pb, canonical, buckets) -> PyCBL:
    """a PyCBL holding a copy of a crafted {prefix: (kind, items)} dict"""
    c = PyCBL(k, pb, canonical)
    c.buckets = {p: [kind, list(items)] for p, (kind, items) in buckets.items()}
    return c


def words(c: PyCBL):
    """every word of the set: prefix << SUFFIX_BITS | suffix"""
    sb = c.P["SB"]
    return {(p << sb) | s for p, (_, items) in c.buckets.items() for s in items}


# ---- ascending lists for the kernel's round model (tests/test_setops_model.py) and for crafted buckets (tests/test_gpu_setops.py)
def distinct(rng, n, bits):
    """n distinct values below 2^bits in random order (any width: range() cannot be sampled past 2^63)"""
    assert n <= 1 << bits
    if (1 << bits) <= 4 * n + 64:
        return rng.sample(range(1 << bits), n)
    seen = {}
    while len(seen) < n:
        seen.setdefault(rng.getrandbits(bits), None)
    return list(seen)


def random_lists(rng, na, nb, shared, bits=40):
    pool = distinct(rng, na + nb, bits)
    a, b = pool[:na], pool[na:]
    if na and shared:
        b = b[:max(0, nb - shared)] + rng.sample(a, min(shared, na, nb))
    return sorted(set(a)), sorted(set(b))


def straddling_lists(na, nb, T, rng=None, bits=40):
    """Two ascending lists of na and nb distinct values whose merged sequence (a's copy of a pair first) has a shared value at positions
    q*T - 1 | q*T for every round boundary q*T it reaches: a's copy is the last output of a round and b's copy the first of the next. Everything
    else is unshared. Built position by position: the merged sequence is na + nb slots, slot values ascend, each slot is dealt to a side."""
    rng = rng or random.Random(na * 100003 + nb)
    total = na + nb
    pairs = [q * T - 1 for q in range(1, total // T + 1) if q * T < total]  # merged positions of a's copy
    pairs = pairs[:min(na, nb)]
    ra_, rb_ = na - len(pairs), nb - len(pairs)  # unshared words still to deal
    vals = sorted(distinct(rng, total - len(pairs), bits))
    A, B, pos, vi = [], [], 0, 0
    pset = set(pairs)
    while pos < total:
        v = vals[vi]
        vi += 1
        if pos in pset:
            A.append(v)
            B.append(v)
            pos += 2
            continue
        take_a = ra_ > 0 and (rb_ == 0 or rng.random() * (ra_ + rb_) < ra_)
        if take_a:
            A.append(v)
            ra_ -= 1
        else:
            B.append(v)
            rb_ -= 1
        pos += 1
    assert len(A) == na and len(B) == nb, (na, nb, len(A), len(B))
    return A, B
