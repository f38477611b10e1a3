"""`CBL.at_least(cbls, t)` and `CBL.occupancy(cbls)` (cblx_set_at_least / cblx_occupancy_counts) restated on
`oracle.pyref.PyCBL.buckets` (prefix -> [kind, items]) — a helper, not a test file, in the style of tests/setops_many_model.py. The reference has no
such operation; the rules are the project's own:
  * t = 1 is `setops_many_model.merge`, byte for byte (the one-holder clone as stored included);
  * t >= 2, a prefix m < t operands hold: not visited — no result bucket, no operand changes there;
  * t >= 2, m >= t: every holder's Vec is sorted in place (iter_sorted), the result is Vec(ascending {v : t holders or more hold v}), dropped when empty;
  * empty operands count towards n and hold nothing.
`occupancy` visits what a merge visits and leaves the operands as a merge does: hist[j] = distinct k-mers exactly j operands hold.
The second half restates the kernels thread by thread: the short route's (position, kept, holders) per element and the long route's rounds."""
from bisect import bisect_left, bisect_right

import setops_many_model as mm
from oracle.pyref import PyCBL  # noqa: F401  (the operands' type)

MANY_SMALL, MANY_LDS, MAX_OPERANDS = mm.MANY_SMALL, mm.MANY_LDS, mm.MAX_OPERANDS


def at_least(ops, t) -> "PyCBL":
    n = len(ops)
    assert 1 <= n <= MAX_OPERANDS and 1 <= t <= n
    if t == 1:
        return mm.merge(ops)
    res = mm._new_like(ops)
    for p in sorted(set().union(*(x.buckets for x in ops))):
        holders = [x for x in ops if p in x.buckets]
        if len(holders) < t:
            continue
        held = {}
        for x in holders:
            for v in mm._sorted_side(x, p):
                held[v] = held.get(v, 0) + 1
        items = sorted(v for v, c in held.items() if c >= t)
        if items:
            res.buckets[p] = ["vec", items]
    return res


def occupancy(ops):
    """-> hist[0 .. n]; sorts the operands' Vecs on every prefix two or more hold, as merge does"""
    n = len(ops)
    assert 1 <= n <= MAX_OPERANDS
    mm._new_like(ops)
    hist = [0] * (n + 1)
    for p in sorted(set().union(*(x.buckets for x in ops))):
        holders = [x for x in ops if p in x.buckets]
        if len(holders) == 1:
            hist[1] += len(holders[0].buckets[p][1])  # from the directory alone
            continue
        held = {}
        for x in holders:
            for v in mm._sorted_side(x, p):
                held[v] = held.get(v, 0) + 1
        for c in held.values():
            hist[c] += 1
    return hist


# ---- k_bucket_atleast, one "thread" per element: m ascending duplicate-free runs staged back to back
def short_elements(runs, t):
    """-> [(merged position, kept, holders)] per run and element. Position as in mm.or_positions. Holders: 1 + the other runs that hold v — a LOWER run
    holds it when the element just below its upper bound equals v, a HIGHER run when the element at its lower bound does. Kept: no lower run holds v
    and holders >= t."""
    out = []
    for k, run in enumerate(runs):
        row = []
        for j, v in enumerate(run):
            pos, dup, h = j, False, 1
            for kk, other in enumerate(runs):
                if kk == k:
                    continue
                if kk < k:
                    at = bisect_right(other, v)
                    if at > 0 and other[at - 1] == v:
                        dup = True
                        h += 1
                else:
                    at = bisect_left(other, v)
                    if at < len(other) and other[at] == v:
                        h += 1
                pos += at
            row.append((pos, (not dup) and h >= t, h))
        out.append(row)
    return out


def short_route(runs, t):
    """the flags go to the merged positions; the ordered compaction keeps the flagged ones"""
    total = sum(map(len, runs))
    slot = [None] * total
    for k, row in enumerate(short_elements(runs, t)):
        for j, (pos, kept, _) in enumerate(row):
            assert slot[pos] is None, "two elements at one merged position"
            slot[pos] = (runs[k][j], kept)
    assert all(s is not None for s in slot)
    return [v for v, kept in slot if kept]


def short_tally(runs):
    """count-only mode: the holders of every lowest copy"""
    n = len(runs)
    hist = [0] * (n + 1)
    for k, row in enumerate(short_elements(runs, 1)):
        for j, (_, kept, h) in enumerate(row):
            if kept:
                hist[h] += 1
    return hist


# ---- k_bucket_atleast_long: rounds over the runs where they lie. A round stages the next cap // (runs with words left) words of every run; `limit` is
# the smallest last staged word among the runs that have words beyond their window; the elements <= limit (all, when no run goes beyond its window) are
# settled as on the short route, the others are staged again.
def long_rounds(runs, cap=MANY_LDS):
    """-> [(windows, act)] per round: the staged window of every run and how many of its elements the round settles"""
    m = len(runs)
    assert 1 <= m <= cap
    pos, out = [0] * m, []
    while True:
        rem = [len(r) - q for r, q in zip(runs, pos)]
        left = sum(1 for x in rem if x)
        if not left:
            return out
        per = cap // left
        take = [min(x, per) for x in rem]
        windows = [r[q:q + n] for r, q, n in zip(runs, pos, take)]
        beyond = [w[-1] for w, r, q in zip(windows, runs, pos) if w and q + len(w) < len(r)]
        act = [bisect_right(w, min(beyond)) for w in windows] if beyond else list(take)
        assert sum(act) > 0, "a round settles something"
        out.append((windows, act))
        pos = [q + a for q, a in zip(pos, act)]


def long_route(runs, t, cap=MANY_LDS):
    """every round: (position, kept) of the active elements among the staged windows, ordered compaction, appended to the rounds before"""
    out = []
    for windows, act in long_rounds(runs, cap):
        active = sum(act)
        slot = [None] * active
        for k, row in enumerate(short_elements(windows, t)):
            for j, (pos, kept, _) in enumerate(row):
                if j < act[k]:
                    assert pos < active and slot[pos] is None, "an active element outside the merged positions 0 .. active - 1"
                    slot[pos] = (windows[k][j], kept)
        assert all(x is not None for x in slot)
        out += [v for v, kept in slot if kept]
    return out


def long_tally(runs, cap=MANY_LDS):
    """count-only mode: the holders of every lowest copy, round by round"""
    hist = [0] * (len(runs) + 1)
    for windows, act in long_rounds(runs, cap):
        for k, row in enumerate(short_elements(windows, 1)):
            for j, (_, kept, h) in enumerate(row):
                if j < act[k] and kept:
                    hist[h] += 1
    return hist


# ---- the candidates: a vertical counter over the n bitvector words, seven bit planes, compared with t bit-sliced (k_thresh_bv)
def candidates_word(words, t):
    c = [0] * 7
    for x in words:
        carry = x
        for b in range(6):
            c[b], carry = c[b] ^ carry, c[b] & carry
        c[6] ^= carry
    ge = (1 << 64) - 1
    for b in range(7):
        ge = (c[b] & ge) if (t >> b) & 1 else (c[b] | ge)
    return ge
