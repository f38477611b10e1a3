"""Bubble popping on the CPU: the qualified arms and their groups on the link table of gfa_model.definition_model, the order in
Python integers, the kinds and counts, pop_bubbles as rounds of compaction, marking and one WordSet::remove_batch on an oracle.pyref.PyCBL, the carry of
the counts through those removals; and the crafted read sets of the CPU and the GPU tests. Pure CPU; no expectation comes from the GPU path. A helper, not
a test file.

    out(x), in(x)   of image slot x: the links that leave slot x, and the links of the whole table that enter slot x (counted, in both forms)
    qualified arm   image x of unitig p from source slot a to target slot T: a -> x is a link, in(x) == out(x) == 1, the link of x enters T,
                    length[p] <= max_kmers, p is neither the unitig of a nor that of T
    group           the unitigs of the qualified arms that share (a, T); bidirected: (a, T) and (T ^ 1, a ^ 1) are one group
    order           u above v: kc[u] length[v] > kc[v] length[u]; then the longer; then the lower number. Without counts: from the second clause
    kind[u]         2 (kept): in a group of >= 2 unitigs and above all others; 1 (popped): another member is above it; else 0
    a round         the k-mers of the popped unitigs in iteration order, as words, removed by one remove_batch; the counts follow their k-mers"""
from __future__ import annotations

import random

import numpy as np

from oracle.pyref import PyCBL

import abundance_model as am
import gfa_model as gm
import removal_model as rm
import tips_model as tm
from neighbors_model import NUCS, _rand, revcomp_str

STATS = ("rounds", "bubbles", "popped", "popped_kmers", "kmers_left", "fixpoint")
COUNTS = ("bubbles", "popped", "popped_kmers")
MAX = (1 << 32) - 1


# ---- arms, groups, kinds -------------------------------------------------------------------------------------------------------------------------------
def arms_model(lt, length, max_kmers: int):
    """[(a, x, T)] of every qualified arm, in table order of the link a -> x."""
    pairs = gm.slot_pairs(lt)
    outs, indeg = {}, {}
    for a, b in pairs:
        outs.setdefault(a, []).append(b)
        indeg[b] = indeg.get(b, 0) + 1
    arms = []
    for a, x in pairs:
        p = x >> 1
        if indeg[x] != 1 or len(outs.get(x, [])) != 1 or int(length[p]) > max_kmers:
            continue
        t = outs[x][0]
        if p == a >> 1 or p == t >> 1:
            continue
        arms.append((a, x, t))
    return arms


def groups_model(arms, canonical: bool):
    """{key: set of unitigs}; key = the frozenset of the views of the group: {(a, T)} and, bidirected, its mirror (T ^ 1, a ^ 1)."""
    groups = {}
    for a, x, t in arms:
        key = frozenset({(a, t), (t ^ 1, a ^ 1)}) if canonical else frozenset({(a, t)})
        groups.setdefault(key, set()).add(x >> 1)
    return groups


def above(u: int, v: int, length, kc) -> bool:
    if kc is not None:
        lhs, rhs = int(kc[u]) * int(length[v]), int(kc[v]) * int(length[u])  # Python integers: exact
        if lhs != rhs:
            return lhs > rhs
    if int(length[u]) != int(length[v]):
        return int(length[u]) > int(length[v])
    return u < v


def kinds_model(groups, length, kc):
    """(kind, counts): kind uint8 per unitig; counts = (kept arms, popped arms, the k-mers of the popped arms)."""
    kind = np.zeros(len(length), dtype=np.uint8)
    for members in groups.values():
        if len(members) < 2:
            continue
        ranked = sorted(members)
        best = [u for u in ranked if all(above(u, v, length, kc) for v in ranked if v != u)]
        assert len(best) == 1  # the order is total on a group
        for u in ranked:
            assert kind[u] == 0  # an arm is in one group
            kind[u] = 2 if u == best[0] else 1
    counts = (int((kind == 2).sum()), int((kind == 1).sum()), int(np.asarray(length)[kind == 1].sum()))
    return kind, counts


def marks_of_set(kmers, k: int, canonical: bool, max_kmers: int, counts=None):
    """Everything a round looks at: the dict of table, links, kc, arms, groups, kind and counts."""
    assert max_kmers >= 1
    t = gm.walk_model(kmers, k, canonical)
    lt = gm.definition_model(kmers, k, canonical, t)
    kc = None if counts is None else am.kc_model(t, counts)
    arms = arms_model(lt, t["length"], max_kmers)
    groups = groups_model(arms, canonical)
    kind, c = kinds_model(groups, t["length"], kc)
    return {"table": t, "links": lt, "kc": kc, "arms": arms, "groups": groups, "kind": kind, "counts": c}


def selected(marks):
    """Per k-mer, in iteration order: whether its unitig is popped."""
    kd = marks["kind"][marks["table"]["unitig"].astype(np.int64)] if len(marks["kind"]) else np.zeros(0, dtype=np.uint8)
    return kd == 1


# ---- pop_bubbles ---------------------------------------------------------------------------------------------------------------------------------------
def pop_model(m: PyCBL, max_kmers: int, counts, rounds: int, trace=None):
    """cblx_pop_bubbles on m, in place; returns (stats, counts after or None). counts: None (the length rule) or a uint32 array by ordinal; the array that
    comes back has the length of the one given: the survivors' counts by their new ordinals, then zeros. A call that removes nothing returns the array as
    it was. trace (a list) takes, per round, (k-mers of the round in iteration order, selection, marks, counts of the round)."""
    k, canonical = m.P["K"], m.canonical
    st = dict.fromkeys(STATS, 0)
    given = None if counts is None else len(counts)
    cur = None if counts is None else np.asarray(counts, dtype=np.uint32).copy()
    assert counts is None or given == m.count()
    r = 0
    while True:
        words = tm.iteration_words(m)
        kmers = [tm.kmer_of_word(w, m.P) for w in words]
        now = None if cur is None else cur[: len(words)]
        marks = marks_of_set(kmers, k, canonical, max_kmers, now)
        sel = selected(marks)
        st["rounds"] += 1
        if trace is not None:
            trace.append((kmers, sel, marks, None if now is None else now.copy()))
        if not sel.any():
            st["fixpoint"] = 1
            break
        c = marks["counts"]
        st["bubbles"] += c[0]
        st["popped"] += c[1]
        st["popped_kmers"] += c[2]
        held = None if cur is None else {w: int(v) for w, v in zip(words, now.tolist())}  # the carry: the count goes with the word
        rm.remove_batch(m, [w for w, f in zip(words, sel.tolist()) if f])
        if cur is not None:
            after = tm.iteration_words(m)
            cur = np.array([held[w] for w in after] + [0] * (given - len(after)), dtype=np.uint32)
        r += 1
        if r == rounds:
            break
    st["kmers_left"] = m.count()
    return st, cur


# ---- crafted read sets: lists of reads (bytes), usable in both forms -------------------------------------------------------------------------------------
def _distinct(rng, n: int, avoid=""):
    """n different letters, none of them in `avoid`."""
    return rng.sample([c for c in NUCS if c not in avoid], n)


def bubble_strings(rng, k: int, mids, flank: int = None, left=None, right=None):
    """len(mids) strings A + M + B that leave A by different letters and enter B by different letters: arms of len(M) + K - 1 k-mers each between the last
    k-mer of A and the first of B. mids: lengths (0: the arm of K - 1 k-mers, A + B itself). Returns (strings, A, B)."""
    flank = k + 6 if flank is None else flank
    a = _rand(rng, flank) if left is None else left
    b = _rand(rng, flank) if right is None else right
    n = len(mids)
    assert n <= 4 and mids.count(0) <= 1
    while True:  # the letter behind A and the letter in front of B, per string: pairwise different; an empty M has B[0] and A[-1], a single letter is both
        firsts = [b[0] if ln == 0 else rng.choice(NUCS) for ln in mids]
        lasts = [a[-1] if ln == 0 else f if ln == 1 else rng.choice(NUCS) for ln, f in zip(mids, firsts)]
        if len(set(firsts)) == n and len(set(lasts)) == n:
            break
    out = []
    for ln, f, la in zip(mids, firsts, lasts):
        out.append(a + ("" if ln == 0 else f if ln == 1 else f + _rand(rng, ln - 2) + la) + b)
    return out, a, b


def snp_reads(k: int, seed: int = 71, variants: int = 2):
    """A read and its copies with another letter at one middle position: arms of exactly K k-mers."""
    rng = random.Random(seed + k)
    base = _rand(rng, 2 * (k + 6) + 1)
    p = k + 6
    letters = [base[p]] + _distinct(rng, variants - 1, base[p])
    return [(base[:p] + c + base[p + 1:]).encode() for c in letters]


def indel_reads(k: int, seed: int = 73):
    """A read and its copy without one middle letter: arms of K and K - 1 k-mers."""
    rng = random.Random(seed + k)
    s, _, _ = bubble_strings(rng, k, [1, 0])
    return [x.encode() for x in s]


def chain_reads(k: int, seed: int = 79, mids=((1, 1), (1, 1)), gap: int = None):
    """Bubbles one behind the other on one trunk, `gap` letters apart (more than K): reads[0] is the trunk through the first arm of every bubble, the others
    are windows around the other arms."""
    rng = random.Random(seed + k)
    gap = k + 7 if gap is None else gap
    trunk, others = _rand(rng, gap), []
    for md in mids:
        s, a, b = bubble_strings(rng, k, list(md), flank=gap, left=trunk[-gap:])
        others += [x[gap - k: len(x) - gap + k] for x in s[1:]]  # K letters of the flanks: the arm and one k-mer of the source and of the target
        trunk += s[0][gap:]
    return [trunk.encode()] + [x.encode() for x in others]


def split_reads(k: int, seed: int = 83):
    """Two arms of K k-mers from one source to different targets, each target entered by a read of its own as well."""
    rng = random.Random(seed + k)
    a = _rand(rng, k + 6)
    x, y = _distinct(rng, 2)
    r1, r2 = a + x + _rand(rng, 2 * k), a + y + _rand(rng, 2 * k)
    q = len(a) + 1
    return [r.encode() for r in (r1, r2, tm._entering(rng, r1, q, k, 4), tm._entering(rng, r2, q, k, 4))]


def shared_reads(k: int, seed: int = 89):
    """Two SNP bubbles on two reads: an arm of the first has a second way in at its head, an arm of the second a second way out at its tail."""
    rng = random.Random(seed + k)
    out = []
    for which in (0, 1):
        base = _rand(rng, 2 * (k + 6) + 1)
        p = k + 6
        var = base[:p] + tm._other(rng, base[p]) + base[p + 1:]
        extra = tm._entering(rng, base, p - k + 1, k, 5) if which == 0 else tm._leaving(rng, base, p + 1, k, 5)
        out += [base, var, extra]
    return [r.encode() for r in out]


def loop_reads(k: int, seed: int = 97):
    """U + M + U for two M: the arms lead from the tail of U to its own head."""
    rng = random.Random(seed + k)
    u = _rand(rng, k + 8)
    s, _, _ = bubble_strings(rng, k, [1, 1], left=u, right=u)
    return [x.encode() for x in s]


def mirror_reads(k: int, arms: int, seed: int = 101):
    """U + M + rc(U): in the bidirected form the arm leads from the tail of U to the head of U's mirror, a = T ^ 1, and rc(read) = U + rc(M) + rc(U) is the
    arm's other image in the same group. One arm: never popped. Two arms: one popped."""
    rng = random.Random(seed + k + arms)
    u = _rand(rng, k + 8)
    ru = revcomp_str(u)
    while True:  # the four letters at the ends of M and rc(M) differ, so four links leave the source
        mids = [_rand(rng, 5) for _ in range(arms)]
        firsts = [m[0] for m in mids] + [revcomp_str(m)[0] for m in mids]
        if len(set(firsts)) == 2 * arms:
            break
    return [(u + m + ru).encode() for m in mids]


def nested_reads(k: int, seed: int = 103):
    """An outer bubble A + M1 + B / A + M2 + B whose long arm M1 holds a SNP bubble: round 1 pops the inner arm, round 2 the outer one, round 3 nothing."""
    rng = random.Random(seed + k)
    s, a, b = bubble_strings(rng, k, [3 * k, 1])
    long_arm = s[0]
    p = len(a) + (3 * k) // 2
    inner = long_arm[:p] + tm._other(rng, long_arm[p]) + long_arm[p + 1:]
    return [long_arm.encode(), s[1].encode(), inner[p - k: p + k + 1].encode()]


def tipped_reads(k: int, seed: int = 107):
    """A SNP bubble whose first arm carries a tip of 4 k-mers in its middle: no bubble until the tip is clipped."""
    rng = random.Random(seed + k)
    base, var = (r.decode() for r in snp_reads(k, seed))
    p = k + 6
    return [base.encode(), var.encode(), tm._leaving(rng, base, p - k // 2 + 1, k, 4).encode()]


def homopolymer_reads(k: int, m: int, seed: int = 109):
    """P + c^r + S and P + c^(r + 1) + S with r = K - 1 - m: arms of m and m + 1 k-mers (an indel in a homopolymer run)."""
    rng = random.Random(seed + k + m)
    c = "C"
    pre = _rand(rng, k + 4) + tm._other(rng, c)
    suf = tm._other(rng, c) + _rand(rng, k + 4)
    r = k - 1 - m
    return [(pre + c * r + suf).encode(), (pre + c * (r + 1) + suf).encode()]


def long_pair_reads(k: int, seed: int = 113, lengths=(300, 299)):
    """Arms of 300 and 299 k-mers."""
    rng = random.Random(seed + k)
    s, _, _ = bubble_strings(rng, k, [ln - k + 1 for ln in lengths])
    return [x.encode() for x in s]


def deep_reads(k: int = 15, seed: int = 59, bubbles: int = 8):
    """tips_model.deep_reads (many k-mers per bucket at PREFIX_BITS = 6, a bucket of its own for the C / G path) with SNP bubbles on the trunk between its
    branches, the variants in front of the trunk: the words of the popped arms stand in front of survivors in the Vecs, so their swap_remove moves ordinals."""
    reads = tm.deep_reads(k, seed)
    trunk = reads[-1].decode()
    rng = random.Random(seed + k + 1)
    variants = []
    for j in range(bubbles):
        p = 20 * (j + 2) + 17  # k-mers p - K + 1 .. p lie between the branches at 20 (j + 2) and 20 (j + 3)
        variants.append((trunk[p - k: p] + tm._other(rng, trunk[p]) + trunk[p + 1: p + k + 1]).encode())
    cg = "".join(rng.choice("CG") for _ in range(2 * k + 1))  # a bubble over C and G alone: its popped arm empties nothing, its bucket shrinks
    cg_var = cg[:k] + ("G" if cg[k] == "C" else "C") + cg[k + 1:]
    return variants + [cg_var.encode(), cg.encode()] + reads


def sized_reads(k: int, unitigs: int, seed: int = 127, bubbles: int = 8):
    """Exactly `unitigs` unitigs in either form: a chain of `bubbles` SNP bubbles (3 per bubble and 1) and isolated reads of one k-mer."""
    rng = random.Random(seed + unitigs)
    reads = chain_reads(k, seed + unitigs, mids=((1, 1),) * bubbles)
    return reads + [_rand(rng, k).encode() for _ in range(unitigs - (3 * bubbles + 1))]


PB = tm.PB
SIZES = (63, 64, 65, 255, 256, 257)
CRAFTED = (["snp15", "snp31", "snp33", "snp59", "snp31-short", "indel", "triple", "quad", "split", "shared", "edge", "ties", "cross", "long-pair", "nested", "chain",
            "loop", "mirror1", "mirror2", "strands", "tipped", "deep"] + [f"sized{n}" for n in SIZES])


def crafted(name):
    """(k, pb, flushes, max_kmers, tally) of a crafted case: the CPU and the GPU tests insert the same flushes, into an index of either form. tally: the
    batch of reads whose occurrences are the counts (the first read three times, the others once), or a function (kmers, table, k) -> uint32 array."""
    def reads_case(k, reads, mk, pb=None, tally=None):
        return k, (PB[k] if pb is None else pb), [reads], mk, ([reads[0]] * 3 + reads[1:] if tally is None else tally)

    if name.startswith("snp"):
        k = int(name[3:5])
        return reads_case(k, snp_reads(k), k - 1 if name.endswith("short") else k)
    if name == "indel":
        return reads_case(31, indel_reads(31), 31)
    if name == "triple":
        return reads_case(31, snp_reads(31, variants=3), 40)
    if name == "quad":
        return reads_case(31, snp_reads(31, variants=4), 2 * 31)
    if name == "split":
        return reads_case(31, split_reads(31), 40)
    if name == "shared":
        return reads_case(31, shared_reads(31), 40)
    if name == "edge":  # a SNP (arms of K = max_kmers) and two neighbouring substitutions (arms of K + 1)
        return reads_case(31, chain_reads(31, mids=((1, 1), (2, 2))), 31)
    if name == "ties":  # every read once: the arms of a bubble have the same mean; the indel goes to the longer arm, the SNP to the lower number
        reads = chain_reads(31, seed=131, mids=((1, 0), (1, 1)))
        return reads_case(31, reads, 40, tally=list(reads))
    if name == "cross":
        return reads_case(15, homopolymer_reads(15, 3), 10, tally=cross_counts)
    if name == "long-pair":
        return reads_case(31, long_pair_reads(31), 300, tally=lambda kmers, table, k: np.full(len(kmers), MAX, dtype=np.uint32))
    if name == "nested":
        return reads_case(31, nested_reads(31), 5 * 31)
    if name == "chain":
        return reads_case(31, chain_reads(31), 31)
    if name == "loop":
        return reads_case(31, loop_reads(31), 31)
    if name.startswith("mirror"):
        return reads_case(31, mirror_reads(31, int(name[6:])), 40)
    if name == "strands":  # every second read as its reverse complement
        reads = chain_reads(31, seed=137, mids=((1, 1), (1, 0), (1, 1, 1)))
        reads = [r if j % 2 == 0 else revcomp_str(r.decode()).encode() for j, r in enumerate(reads)]
        return reads_case(31, reads, 40)
    if name == "tipped":
        return reads_case(31, tipped_reads(31), 31)
    if name == "deep":
        reads = deep_reads(15)
        return reads_case(15, reads, 15, pb=6, tally=[reads[-1]] * 3 + reads[:-1])  # the trunk three times
    assert name.startswith("sized")
    return reads_case(31, sized_reads(31, int(name[5:])), 31)


def cross_counts(kmers, table, k: int):
    """kc = 7 on the arm of 3 k-mers and 9 on the arm of 4 (7 / 3 > 9 / 4: 28 > 27), 5 per k-mer elsewhere."""
    counts = np.full(len(kmers), 5, dtype=np.uint32)
    mem = am.members(table)
    short = [u for u, o in enumerate(mem) if len(o) == 3]
    long_ = [u for u, o in enumerate(mem) if len(o) == 4]
    assert len(short) == 1 and len(long_) == 1
    am.spread(7, 3, mem[short[0]], counts)
    am.spread(9, 4, mem[long_[0]], counts)
    return counts


def counts_of_case(m: PyCBL, kmers, table, tally):
    """The counts of a case on the model index: a tally of its reads from zeros, or its function."""
    if callable(tally):
        return np.asarray(tally(kmers, table, m.P["K"]), dtype=np.uint32)
    return am.tally_model(m, tally)[0]


def features(marks, canonical: bool):
    """What a case exercises, from the marks of its first round."""
    t, lt, kind = marks["table"], marks["links"], marks["kind"]
    length = t["length"]
    rev_of = {}
    start = [int(s) for s in lt["link_start"]]
    for a in range(len(start) - 1):
        for ln in range(start[a], start[a + 1]):
            rev_of[(a, 2 * int(lt["link_to"][ln]) + int(lt["link_rev"][ln]))] = int(lt["link_rev"][ln])
    live = {key: mem for key, mem in marks["groups"].items() if len(mem) >= 2}
    arms = [(a, x, tt) for a, x, tt in marks["arms"] if kind[x >> 1]]
    return {"groups": sorted(len(mem) for mem in live.values()), "popped_lengths": sorted(length[kind == 1].tolist()), "kept_lengths": sorted(length[kind == 2].tolist()),
            "singles": sum(1 for mem in marks["groups"].values() if len(mem) == 1), "entered_reversed": any(rev_of[(a, x)] for a, x, _ in arms),
            "source_odd": any(a & 1 for a, _, _ in arms), "self_mirror": any(a == tt ^ 1 for a, _, tt in arms), "loop": any(a >> 1 == tt >> 1 for a, _, tt in arms),
            "unitigs": len(length)}
