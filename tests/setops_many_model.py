"""The reference's `CBL::merge(Vec<&mut Self>)` and `CBL::intersect(Vec<&mut Self>)` (/root/reference/src/cbl.rs:106-124) restated on
`oracle.pyref.PyCBL.buckets` (prefix -> [kind, items]) — a helper, not a test file, in the style of tests/setops_model.py.
src/wordset/set_ops.rs:11-42 (merge) and :49-75 (intersect) walk the operands' prefix sets with `merge_iters_detailed_by` / `intersect_iters_detailed_by`:
per distinct prefix ascending, the (operand index, item) of every operand that holds it — all prefixes for merge, only those EVERY operand holds for
intersect. Per visited prefix:
  * merge, one holder: the bucket is CLONED as stored, kind and order kept;
  * merge, two or more holders: `iter_sorted` on every holder sorts a Vec IN PLACE (the operands are `&mut`); the result is
    `TrieVec::new().insert_sorted_iter(union)`, src/trievec/mod.rs:118-131 — a Vec, ascending, whatever its length;
  * intersect: `iter_sorted` on every operand; the result is Vec(ascending intersection), dropped when empty. Nothing else in any operand changes.
`merge` / `intersect` return a new PyCBL and mutate their operands the way the reference does; `PyCBL.serialize()` gives the expected bytes of all.
The second half restates the short route of k_bucket_setop_many (cbl_amd/csrc/kernels_setops.hpp) thread by thread."""
from bisect import bisect_left, bisect_right

from oracle.pyref import PyCBL

MANY_SMALL, MANY_LDS = 256, 2048  # kernels_setops.hpp: words of all holders one wave / one workgroup stages in LDS; longer buckets are folded
MAX_OPERANDS = 64  # include/cblx.h CBLX_SETOP_MAX_OPERANDS


def _new_like(ops):
    a = ops[0]
    assert len(ops) >= 1 and len(set(map(id, ops))) == len(ops), "the reference takes &mut of each operand"
    for x in ops:
        assert x.canonical == a.canonical, "One of the index is canonical while the other isn't"
        assert (x.P["K"], x.P["PB"]) == (a.P["K"], a.P["PB"])
    return PyCBL(a.P["K"], a.P["PB"], a.canonical)


def _sorted_side(x, p):
    """iter_sorted: a Vec is sorted in place, a Trie iterates ascending"""
    if x.buckets[p][0] == "vec":
        x.buckets[p][1].sort()
    return x.buckets[p][1]


def merge(ops) -> PyCBL:
    res = _new_like(ops)
    for p in sorted(set().union(*(x.buckets for x in ops))):
        holders = [x for x in ops if p in x.buckets]
        if len(holders) == 1:
            res.buckets[p] = [holders[0].buckets[p][0], list(holders[0].buckets[p][1])]
        else:
            res.buckets[p] = ["vec", sorted(set().union(*(_sorted_side(x, p) for x in holders)))]
    return res


def intersect(ops) -> PyCBL:
    res = _new_like(ops)
    for p in sorted(set.intersection(*(set(x.buckets) for x in ops))):
        items = sorted(set.intersection(*(set(_sorted_side(x, p)) for x in ops)))
        if items:
            res.buckets[p] = ["vec", items]
    return res


MANY = {"or": merge, "and": intersect}


# ---- k_bucket_setop_many's short route, one "thread" per element: m ascending duplicate-free runs staged back to back
def or_positions(runs):
    """-> [(merged position, kept)] per run and element. Position: own index + per other run one binary search — runs of LOWER index count their
    elements <= v, runs of HIGHER index those < v, so the lowest holder's copy of a value comes first. Kept: no lower run holds v (seen by the same
    search: the element just below the upper bound)."""
    out = []
    for k, run in enumerate(runs):
        row = []
        for j, v in enumerate(run):
            pos, dup = j, False
            for kk, other in enumerate(runs):
                if kk == k:
                    continue
                at = bisect_right(other, v) if kk < k else bisect_left(other, v)
                pos += at
                if kk < k and at > 0 and other[at - 1] == v:
                    dup = True
            row.append((pos, not dup))
        out.append(row)
    return out


def or_short_route(runs):
    """the flags go to the merged positions; the ordered compaction keeps the flagged ones"""
    total = sum(map(len, runs))
    slot = [None] * total
    for k, row in enumerate(or_positions(runs)):
        for j, (pos, kept) in enumerate(row):
            assert slot[pos] is None, "two elements at one merged position"
            slot[pos] = (runs[k][j], kept)
    assert all(s is not None for s in slot)
    assert [v for v, _ in slot] == sorted(v for r in runs for v in r)  # the merged multiset, ascending
    return [v for v, kept in slot if kept]


def and_short_route(runs):
    """the elements of the shortest run (the lowest one on ties) searched in every other run"""
    ks = min(range(len(runs)), key=lambda k: (len(runs[k]), k))
    out = []
    for v in runs[ks]:
        keep = True
        for kk, other in enumerate(runs):
            if kk != ks and keep:
                at = bisect_left(other, v)
                keep = at < len(other) and other[at] == v
        if keep:
            out.append(v)
    return out
