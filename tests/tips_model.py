"""Tip clipping on the CPU: the degrees at the two ends of every unitig, the marks, and clip_tips as rounds of compaction, marking and
one WordSet::remove_batch on an oracle.pyref.PyCBL; and the crafted read sets of the CPU and the GPU tests. Pure CPU; no expectation comes from the GPU
path. A helper, not a test file.

    table, masks    gfa_model.walk_model / masks_of_set of the k-mers in iteration order: the plain table of a non-canonical set (section 6k), the
                    bidirected one of a canonical set (section 6l); bit c of a mask = successor by base c held, bit 4 + c = predecessor by base c held
    right(u)        the out-degree of the tail of the kept image: popcount(mask & 15) of its stored k-mer, popcount(mask >> 4) where that is reversed
    left(u)         the in-degree of the head of the kept image: popcount(mask >> 4), popcount(mask & 15) where that is reversed
    kind[u]         with length[u] <= max_kmers: 1 (tip) when exactly one of left, right is 0, 2 (isolated) when both are; otherwise 0
    a round         the k-mers of the marked unitigs (tips; isolated ones too when asked) in iteration order, as words, removed by one remove_batch"""
from __future__ import annotations

import random

import numpy as np

from oracle.pyref import THRESHOLD, PyCBL, necklace_pos

import gfa_model as gm
import removal_model as rm
from neighbors_model import NUCS, _primitive, _rand, revcomp_str

STATS = ("rounds", "tips", "tip_kmers", "isolated", "isolated_kmers", "kmers_left", "fixpoint")


# ---- words and k-mers ------------------------------------------------------------------------------------------------------------------------------
def kmer_of_word(w: int, P) -> int:
    """The k-mer a word stands for: the necklace rotated back by its position (the stored form in a canonical set)."""
    kb, pos_bits = P["KB"], P["POS"]
    n, p = w >> pos_bits, w & ((1 << pos_bits) - 1)
    return ((n >> p) | (n << (kb - p))) & ((1 << kb) - 1)


def word_of_kmer(x: int, P) -> int:
    n, p = necklace_pos(x, P["KB"])
    return (n << P["POS"]) | p


def iteration_words(m: PyCBL):
    """CBL::iter order: ascending prefixes, every bucket as stored."""
    sb = m.P["SB"]
    return [(p << sb) | s for p in sorted(m.buckets) for s in m.buckets[p][1]]


def model_of_words(k: int, pb: int, canonical: bool, words) -> PyCBL:
    """A PyCBL holding `words` (the iteration order of an index that only ever took inserts: a bucket is a Trie exactly when it outgrew THRESHOLD)."""
    m = PyCBL(k, pb, canonical)
    sb = m.P["SB"]
    for w in words:
        m.buckets.setdefault(w >> sb, ["vec", []])[1].append(w & ((1 << sb) - 1))
    for b in m.buckets.values():
        if len(b[1]) > THRESHOLD:
            b[0] = "trie"
            assert b[1] == sorted(b[1])
    return m


# ---- ends and kinds --------------------------------------------------------------------------------------------------------------------------------
def _pc(x: int) -> int:
    return bin(x).count("1")


def ends_model(kmers, k: int, canonical: bool, table, masks):
    """(left, right): uint8 arrays over the unitigs of `table`."""
    nu = len(table["head"])
    left, right = np.full(nu, 0xFF, dtype=np.uint8), np.full(nu, 0xFF, dtype=np.uint8)
    for i in range(len(kmers)):
        u, off, s, m = int(table["unitig"][i]), int(table["offset"][i]), int(table["reversed"][i]), int(masks[i])
        assert canonical or s == 0
        if off == 0:
            assert left[u] == 0xFF  # one writer
            left[u] = _pc(m & 15) if s else _pc(m >> 4)
        if off + 1 == int(table["length"][u]):
            assert right[u] == 0xFF
            right[u] = _pc(m >> 4) if s else _pc(m & 15)
    assert nu == 0 or (int(left.max()) <= 4 and int(right.max()) <= 4)  # every element written
    return left, right


def kinds_model(table, left, right, max_kmers: int):
    """(kind, counts): kind uint8 per unitig; counts = (tips, their k-mers, isolated unitigs, their k-mers)."""
    assert max_kmers >= 1
    kind = np.zeros(len(table["head"]), dtype=np.uint8)
    counts = [0, 0, 0, 0]
    for u, ln in enumerate(table["length"].tolist()):
        dead = (int(left[u]) == 0) + (int(right[u]) == 0)
        if ln <= max_kmers and dead:
            kind[u] = dead
            counts[2 * (dead - 1)] += 1
            counts[2 * (dead - 1) + 1] += ln
    return kind, tuple(counts)


def marks_of_set(kmers, k: int, canonical: bool, max_kmers: int):
    """Everything a round looks at: the dict of table, masks, left, right, kind and counts."""
    t = gm.walk_model(kmers, k, canonical)
    masks = gm.masks_of_set(kmers, k, canonical)
    left, right = ends_model(kmers, k, canonical, t, masks)
    kind, counts = kinds_model(t, left, right, max_kmers)
    return {"table": t, "masks": masks, "left": left, "right": right, "kind": kind, "counts": counts}


def selected(marks, isolated: bool):
    """Per k-mer, in iteration order: whether its unitig is removed."""
    kd = marks["kind"][marks["table"]["unitig"].astype(np.int64)] if len(marks["kind"]) else np.zeros(0, dtype=np.uint8)
    return (kd == 1) | ((kd == 2) & bool(isolated))


# ---- clip_tips -------------------------------------------------------------------------------------------------------------------------------------
def clip_model(m: PyCBL, max_kmers: int, isolated: bool, rounds: int, trace=None):
    """cblx_clip_tips on m, in place; returns the stats. trace (a list) takes, per round, (k-mers of the round in iteration order, selection, marks)."""
    k, canonical = m.P["K"], m.canonical
    st = dict.fromkeys(STATS, 0)
    r = 0
    while True:
        words = iteration_words(m)
        kmers = [kmer_of_word(w, m.P) for w in words]
        marks = marks_of_set(kmers, k, canonical, max_kmers)
        sel = selected(marks, isolated)
        st["rounds"] += 1
        if trace is not None:
            trace.append((kmers, sel, marks))
        if not sel.any():
            st["fixpoint"] = 1
            break
        c = marks["counts"]
        st["tips"] += c[0]
        st["tip_kmers"] += c[1]
        if isolated:
            st["isolated"] += c[2]
            st["isolated_kmers"] += c[3]
        rm.remove_batch(m, [w for w, f in zip(words, sel.tolist()) if f])  # the words of the selected k-mers are the stored words themselves
        r += 1
        if r == rounds:
            break
    st["kmers_left"] = m.count()
    return st


# ---- crafted read sets: lists of reads (bytes), usable in both forms -------------------------------------------------------------------------------
def _other(rng, c: str) -> str:
    return rng.choice([x for x in NUCS if x != c])


def _leaving(rng, trunk: str, p: int, k: int, n: int) -> str:
    """A read that shares the K - 1 letters from p with the trunk and goes on with n letters of its own: n k-mers that leave the trunk behind k-mer p - 1."""
    return trunk[p: p + k - 1] + _other(rng, trunk[p + k - 1]) + _rand(rng, n - 1)


def _entering(rng, trunk: str, q: int, k: int, n: int) -> str:
    """n letters of its own, then the K - 1 letters from q: n k-mers that enter the trunk in front of k-mer q."""
    return _rand(rng, n - 1) + _other(rng, trunk[q - 1]) + trunk[q: q + k - 1]


def edge_reads(k: int, max_kmers: int, seed: int = 41):
    """A trunk of 6 K k-mers with four dead-end branches: one that leaves it and one that enters it of exactly max_kmers k-mers, and one each of
    max_kmers + 1. The end pieces of the trunk are longer than max_kmers (they are dead ends too)."""
    assert max_kmers <= k
    rng = random.Random(seed + k)
    trunk = _rand(rng, 7 * k - 1)
    reads = [trunk, _leaving(rng, trunk, 2 * k, k, max_kmers), _leaving(rng, trunk, 3 * k, k, max_kmers + 1),
             _entering(rng, trunk, 4 * k, k, max_kmers), _entering(rng, trunk, 5 * k - 3, k, max_kmers + 1)]
    return [r.encode() for r in reads]


def cascade_reads(k: int, seed: int = 43, branch: int = 4, arms=(3, 6)):
    """A trunk with a branch of `branch` k-mers that ends in a fork of two dead ends: round 1 takes the arms, round 2 the branch, round 3 finds nothing."""
    rng = random.Random(seed + k)
    trunk = _rand(rng, 5 * k)
    stem = _leaving(rng, trunk, 2 * k, k, branch)
    a1 = _rand(rng, arms[0])
    a2 = _other(rng, a1[0]) + _rand(rng, arms[1] - 1)
    return [r.encode() for r in (trunk, stem + a1, stem[-(k - 1):] + a2)]


def fork_reads(k: int, seed: int = 47, stem: int = 5, arms=(2, 4)):
    """A stem and two arms and nothing else: three tips in one round."""
    rng = random.Random(seed + k)
    s = _rand(rng, k - 1 + stem)
    a1 = _rand(rng, arms[0])
    a2 = _other(rng, a1[0]) + _rand(rng, arms[1] - 1)
    return [r.encode() for r in (s + a1, s[-(k - 1):] + a2)]


def island_reads(k: int, max_kmers: int, seed: int = 53, cycle: int = 7):
    """An isolated path of max_kmers k-mers and one of max_kmers + 1; a pure cycle of `cycle` k-mers; poly-A; and u + rc(u) with |u| = K, whose K + 1 k-mers
    are (K + 1) / 2 mirror pairs: in the canonical form a unitig whose one end is linked to nothing and whose other end only to itself."""
    rng = random.Random(seed + k)
    s = _rand(rng, cycle)
    while not _primitive(s):
        s = _rand(rng, cycle)
    u = _rand(rng, k)
    reads = [_rand(rng, k - 1 + max_kmers), _rand(rng, k + max_kmers), (s * (k // cycle + 2))[: cycle + k - 1], "A" * k, u + revcomp_str(u)]
    return [r.encode() for r in reads]


def deep_reads(k: int = 15, seed: int = 59, branches: int = 28):
    """Many k-mers per bucket at a small PREFIX_BITS: a trunk with a branch every 20 k-mers, leaving and entering by turns, of 1 .. K - 1 k-mers; and an
    isolated path over the letters C and G alone, whose words (both strands) have prefixes the rest does not reach."""
    rng = random.Random(seed + k)
    trunk = _rand(rng, 20 * (branches + 2) + k)
    reads = [trunk]
    for j in range(branches):
        n = 1 + (5 * j) % (k - 1)
        reads.append(_leaving(rng, trunk, 20 * (j + 1), k, n) if j % 2 == 0 else _entering(rng, trunk, 20 * (j + 1), k, n))
    reads.append("".join(rng.choice("CG") for _ in range(k - 1 + 6)))
    reads = reads[1:] + reads[:1]  # the trunk last: the words of the tips stand in front of it in the Vecs, so their swap_remove shows
    return [r.encode() for r in reads]


PB = {15: 6, 31: 24, 33: 16, 59: 28}  # the PREFIX_BITS of the other crafted graph cases
CRAFTED = ["edge", "edge15", "edge33", "edge59", "cascade", "fork", "islands", "deep"]


def crafted(name):
    """(k, pb, flushes, max_kmers) of a crafted case: the CPU and the GPU tests insert the same flushes, into an index of either form."""
    if name.startswith("edge"):
        k = int(name[4:] or 31)
        mk = {15: 5, 31: k - 1, 33: k, 59: 12}[k]  # the default, below it, and K itself
        return k, PB[k], [edge_reads(k, mk)], mk
    if name == "cascade":
        return 31, 24, [cascade_reads(31)], 6
    if name == "fork":
        return 31, 24, [fork_reads(31)], 5
    if name == "islands":
        return 31, 24, [island_reads(31, 30)], 30
    assert name == "deep"
    return 15, 6, [deep_reads(15)], 14


def features(kmers, marks, canonical: bool):
    """What a case exercises, from the marks of its first round."""
    t, left, right, kind = marks["table"], marks["left"], marks["right"], marks["kind"]
    tips = np.flatnonzero(kind == 1)
    ends_rev = set()
    for i in range(len(kmers)):
        u, off = int(t["unitig"][i]), int(t["offset"][i])
        if int(t["reversed"][i]) and (off == 0 or off + 1 == int(t["length"][u])):
            ends_rev.add(u)
    return {"left_dead": bool(((left[tips] == 0)).any()), "right_dead": bool((right[tips] == 0).any()),
            "reversed_end": any(u in ends_rev for u in tips.tolist()), "isolated": bool((kind == 2).any()),
            "lengths": sorted(set(t["length"][tips].tolist()))}
