"""Unitigs on the CPU: (i) the definition as a sequential walk over the k-mers of a non-canonical set in iteration order,
(ii) the route the device takes restated with numpy — links, pointer-jumping rounds with the stall rule, the cut of the pure cycles, numbering —
(iii) the text, and (iv) the crafted inputs of the GPU tests. Pure CPU; no expectation comes from the GPU path. A helper, not a test file.

    edge x -> y      y = append(x, c), both in the set; SIMPLE when x has one successor and y one predecessor in the set
    unitig           a path or a cycle of simple edges; every k-mer is in exactly one
    head             the k-mer of a path without a simple in-edge; of a cycle of simple edges only, its member with the smallest ordinal (circular)
    numbering        by ascending ordinal of the heads; offset = simple edges from the head

The ordinal of a k-mer is its index in the iteration order (neighbors_model.oracle_kmers)."""
from __future__ import annotations

import random

import numpy as np

import neighbors_model as nm
from neighbors_model import NUCS, _rand, append, oracle_kmers, pack, prepend, unpack  # noqa: F401  (re-exported for the tests)

NONE = 0xFFFFFFFF
RANK_ABSENT = (1 << 64) - 1


# ---- degrees and simple edges ------------------------------------------------------------------------------------------------------------------
def masks_of_set(kmers, k: int):
    """The neighbour masks of the k-mers of a non-canonical set against that set (Python set membership; tests check it against nm.masks_model)."""
    held = set(kmers)
    out = np.zeros(len(kmers), dtype=np.uint8)
    for i, x in enumerate(kmers):
        m = 0
        for j, y in enumerate(nm.neighbors(x, k)):
            if y in held:
                m |= 1 << j
        out[i] = m
    return out


def simple_links(kmers, masks, k: int):
    """(next, prev) as uint32 arrays of ordinals, NONE where a k-mer has no simple out- / in-edge."""
    ordinal = {x: i for i, x in enumerate(kmers)}
    assert len(ordinal) == len(kmers)
    n = len(kmers)
    nxt = np.full(n, NONE, dtype=np.uint32)
    prv = np.full(n, NONE, dtype=np.uint32)
    for i, x in enumerate(kmers):
        out = int(masks[i]) & 15
        if bin(out).count("1") != 1:
            continue
        r = ordinal[append(x, out.bit_length() - 1, k)]
        if bin(int(masks[r]) >> 4).count("1") == 1:
            nxt[i] = r
            assert prv[r] == NONE  # one writer
            prv[r] = i
    return nxt, prv


# ---- (i) the definition: a sequential walk ------------------------------------------------------------------------------------------------------
def _table(n, unitigs):
    """unitigs: [(head ordinal, [member ordinals in offset order], circular)] -> the table, numbered by ascending head."""
    unitigs = sorted(unitigs, key=lambda u: u[0])
    t = {"unitig": np.zeros(n, dtype=np.uint32), "offset": np.zeros(n, dtype=np.uint32),
         "head": np.array([u[0] for u in unitigs], dtype=np.uint32), "length": np.array([len(u[1]) for u in unitigs], dtype=np.uint32),
         "flags": np.array([1 if u[2] else 0 for u in unitigs], dtype=np.uint8), "n_circular": sum(1 for u in unitigs if u[2])}
    for number, (_, members, _) in enumerate(unitigs):
        for off, i in enumerate(members):
            t["unitig"][i] = number
            t["offset"][i] = off
    return t


def walk_model(kmers, k: int, masks=None):
    """The compaction table by following the simple edges one k-mer at a time: from every path head in turn, then — what is left lies on cycles of
    simple edges only — from the smallest ordinal not yet seen."""
    masks = masks_of_set(kmers, k) if masks is None else masks
    nxt, prv = simple_links(kmers, masks, k)
    n = len(kmers)
    seen = [False] * n
    unitigs = []

    def follow(h):
        members, i = [], h
        while i != NONE and not seen[i]:
            seen[i] = True
            members.append(i)
            i = int(nxt[i])
        return members, i

    for h in range(n):
        if prv[h] == NONE:
            members, end = follow(h)
            assert end == NONE  # a path ends at a k-mer without a simple out-edge
            unitigs.append((h, members, False))
    for h in range(n):
        if not seen[h]:
            members, end = follow(h)
            assert end == h  # back at the head: a cycle
            unitigs.append((h, members, True))
    t = _table(n, unitigs)
    t["n_simple"] = int((nxt != NONE).sum())
    return t


# ---- (ii) the device's route: jump rounds with the stall rule, the cycle cut, numbering ---------------------------------------------------------
def jump_model(nxt, prv):
    """List ranking by pointer jumping over prev, as kernels_unitig.hpp does it. State: anc[i], an ancestor of i along the simple in-edges, and dist[i],
    the edges between them; a head has anc = itself and dist = 0, every other k-mer dist >= 1, so `a is a head` reads dist[a] == 0. Each round writes
    fresh arrays and counts the k-mers that were unfinished (their ancestor no head) when it began. Unfinished k-mers of paths strictly decrease, so
    the loop ends when the count is 0 — or when it repeats: then the unfinished k-mers are exactly the members of the pure cycles. Min-doubling over
    next finds each cycle's smallest ordinal; the simple edge into it is cut, it is flagged circular, and its cycle is ranked again.
    Returns (anc, dist, next, prev, circular, rounds)."""
    nxt, prv = nxt.copy(), prv.copy()
    n = len(prv)
    idx = np.arange(n, dtype=np.uint32)
    head = prv == NONE
    anc = np.where(head, idx, prv).astype(np.uint32)
    dist = np.where(head, 0, 1).astype(np.uint64)
    circular = np.zeros(n, dtype=np.uint8)
    last, cut, rounds = None, False, 0
    while n:
        da = dist[anc]
        unfinished = da != 0
        anc, dist = np.where(unfinished, anc[anc], anc), np.minimum(np.where(unfinished, dist + da, dist), NONE)  # both from the old arrays
        rounds += 1
        count = int(unfinished.sum())
        if count == 0:
            break
        if count != last:
            last = count
            continue
        assert not cut, "stalled again after the cycle cut"
        cut, last = True, None
        member = dist[anc] != 0
        low = np.where(member, idx, NONE).astype(np.uint32)
        ptr = np.where(member, nxt, NONE).astype(np.uint32)
        span = 1
        while span < count:  # a cycle has at most `count` members
            live = ptr != NONE
            safe = np.where(live, ptr, 0)
            low, ptr = np.where(live, np.minimum(low, low[safe]), low), np.where(live, ptr[safe], ptr)
            span *= 2
        heads = np.flatnonzero(member & (low == idx))
        others = np.flatnonzero(member & (low != idx))
        nxt[prv[heads]] = NONE
        prv[heads] = NONE
        circular[heads] = 1
        anc[heads], dist[heads] = heads, 0
        anc[others], dist[others] = prv[others], 1
    return anc, dist.astype(np.uint32), nxt, prv, circular, rounds


def route_model(kmers, k: int, masks=None):
    """The compaction table by the device's route; also `rounds`, the number of jump rounds."""
    masks = masks_of_set(kmers, k) if masks is None else masks
    nxt0, prv0 = simple_links(kmers, masks, k)
    anc, dist, nxt, prv, circular, rounds = jump_model(nxt0, prv0)
    n = len(kmers)
    is_head = (prv == NONE).astype(np.int64)
    uid = np.cumsum(is_head) - is_head  # exclusive scan
    nu = int(is_head.sum())
    t = {"unitig": uid[anc].astype(np.uint32) if n else np.zeros(0, dtype=np.uint32), "offset": dist, "head": np.flatnonzero(is_head).astype(np.uint32),
         "length": np.zeros(nu, dtype=np.uint32), "flags": circular[np.flatnonzero(is_head)].astype(np.uint8), "n_circular": int(circular.sum()),
         "n_simple": int((nxt0 != NONE).sum()), "rounds": rounds}
    tails = np.flatnonzero(nxt == NONE)
    t["length"][t["unitig"][tails]] = dist[tails] + 1
    return t


def same_table(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("unitig", "offset", "head", "length", "flags")) and a["n_circular"] == b["n_circular"]


# ---- the identities of the definition ------------------------------------------------------------------------------------------------------------
def check_identities(t, n: int, n_simple=None):
    """Every ordinal occurs once as (unitig, offset); the lengths add up to n; U = n - simple edges + circular unitigs; heads ascend and sit at offset 0."""
    nu = len(t["head"])
    assert len(t["unitig"]) == n and len(t["offset"]) == n and len(t["length"]) == nu and len(t["flags"]) == nu
    assert int(t["length"].astype(np.int64).sum()) == n
    if n:
        assert int(t["unitig"].max()) < nu and (t["offset"] < t["length"][t["unitig"]]).all()
        start = np.concatenate([[0], np.cumsum(t["length"].astype(np.int64))[:-1]])
        slot = start[t["unitig"]] + t["offset"]
        assert np.array_equal(np.sort(slot), np.arange(n))  # a bijection onto 0 .. n - 1
        assert (np.diff(t["head"].astype(np.int64)) > 0).all() and (t["offset"][t["head"]] == 0).all()
        assert np.array_equal(t["unitig"][t["head"]], np.arange(nu))
    assert int((t["flags"] & 1).sum()) == t["n_circular"] and not (t["flags"] & 0xFE).any()
    n_simple = t.get("n_simple") if n_simple is None else n_simple
    if n_simple is not None:
        assert nu == n - n_simple + t["n_circular"]


# ---- (iii) the text ------------------------------------------------------------------------------------------------------------------------------
def text_model(kmers, t, k: int) -> bytes:
    """Line u = the K letters of its head, the last letter of every following k-mer in offset order, a newline: K + length bytes."""
    nu = len(t["head"])
    members = [[None] * int(ln) for ln in t["length"]]
    for i, (u, off) in enumerate(zip(t["unitig"].tolist(), t["offset"].tolist())):
        members[u][off] = i
    lines = []
    for u in range(nu):
        m = members[u]
        assert m[0] == int(t["head"][u])
        lines.append(unpack(kmers[m[0]], k) + "".join(NUCS[kmers[i] & 3] for i in m[1:]))
    text = "".join(ln + "\n" for ln in lines).encode()
    assert len(text) == len(kmers) + nu * k
    return text


def kmers_of_text(text: bytes, k: int):
    """The k-mers of the lines, in line order (a circular unitig is written open: the edge that closes it is not spelled)."""
    out = []
    for ln in text.decode().split("\n")[:-1]:
        assert len(ln) >= k
        out += [pack(ln[i: i + k]) for i in range(len(ln) - k + 1)]
    return out


def summary_model(length, flags, k: int):
    ls = [int(v) for v in length]
    bases = sorted((v + k - 1 for v in ls), reverse=True)
    total, acc, n50 = sum(bases), 0, 0
    for b in bases:
        acc += b
        if 2 * acc >= total:
            n50 = b
            break
    return {"unitigs": len(ls), "circular": sum(int(f) & 1 for f in flags), "kmers": sum(ls), "bases": total, "longest": max(ls, default=0), "n50": n50}


# ---- (iv) crafted inputs: lists of reads (bytes) -------------------------------------------------------------------------------------------------
PATH_LENGTHS = (1, 2, 3, 4, 5, 8, 9, 63, 64, 65, 1023, 1024, 1025, 4097)  # k-mers per path: the rounds end one path after the other
CYCLE_LENGTHS = (64, 65, 1000)


def path_edge_reads(k: int, seed: int = 5):
    """Random reads of PATH_LENGTHS k-mers, pure cycles of CYCLE_LENGTHS k-mers (reads s + s[:K - 1]), and a cycle of 200 with a read running into
    it, which is not pure and comes out linear: the stall rule is met while paths of every length are still running."""
    rng = random.Random(seed * 100 + k)
    reads = [_rand(rng, ln + k - 1) for ln in PATH_LENGTHS]
    for ln in CYCLE_LENGTHS:
        s = _rand(rng, ln)
        reads.append(s + s[: k - 1])
    s = _rand(rng, 200)
    reads += [s + s[: k - 1], _rand(rng, 40) + s[:k]]
    return [r.encode() for r in reads]


def long_path_reads(k: int = 31, n_kmers: int = 70000, seed: int = 9):
    return [_rand(random.Random(seed), n_kmers + k - 1).encode()]


def dense_reads(seed: int = 13, n_reads: int = 300, length: int = 150):
    """For K = 9, PREFIX_BITS = 4: 4^9 = 262 144 possible k-mers, a branching graph with Tries in every bucket."""
    rng = random.Random(seed)
    return [_rand(rng, length).encode() for _ in range(n_reads)]


def branch_reads(k: int, seed: int = 17):
    """(first, second): a path, then a read that leaves it in the middle — inserted in a second flush it splits the unitig in three."""
    rng = random.Random(seed + k)
    main = _rand(rng, 300 + k - 1)
    mid = main[150: 150 + k]
    other = NUCS[(nm.CODE[main[150 + k]] + 1) % 4]
    return [main.encode()], [(mid + other + _rand(rng, 20)).encode()]


def kmers_of_reads(reads, k: int):
    """Distinct k-mers of the reads, in first-occurrence order (NOT the iteration order: for the CPU tests that need a set only)."""
    seen, out = set(), []
    for r in reads:
        r = r.decode()
        for i in range(len(r) - k + 1):
            x = pack(r[i: i + k])
            if x not in seen:
                seen.add(x)
                out.append(x)
    return out
