"""Bidirected unitigs on the CPU: (i) the definition as a sequential walk over the oriented k-mers of a canonical set in iteration
order, (ii) the route the device takes restated with numpy — links from the neighbour masks, unitigs_model.jump_model on 2 n ids, tails / keep / number —
(iii) the text, and (iv) the crafted inputs of the GPU tests. Pure CPU; no expectation comes from the GPU path. A helper, not a test file.

    stored k-mer i      x_i, the form with an even number of set bits (K is odd: exactly one of x and rc(x)); i its index in the iteration order
    oriented k-mer      (i, s) spells sigma(i, 0) = x_i, sigma(i, 1) = rc(x_i); id v = 2 i + s; mirror (i, 1 - s)
    edge                (i, s) -> (j, t) when sigma(j, t) = append(sigma(i, s), c) and x_j is in the set; its mirror (j, 1 - t) -> (i, 1 - s) is one too
    simple              out(i, s) = 1, in(j, t) = 1 and j != i (an edge between a stored k-mer and itself still counts in the degrees)
    unitig              one image of each mirror pair of paths / cycles of simple edges: of a path with head (h, s) and tail (t, u) the image with h < t,
                        or h = t and s = 0; of a pure cycle the image in which the member with the smallest ordinal, its head, has s = 0 (circular)
    numbering           by ascending ordinal of the heads; offset = simple edges from the head; reversed[i] = the s of i's copy on the kept image"""
from __future__ import annotations

import random

import numpy as np

import neighbors_model as nm
import unitigs_model as um
from neighbors_model import NUCS, _rand, append, pack, prepend, unpack  # noqa: F401  (re-exported for the tests)

NONE = um.NONE


# ---- oriented k-mers -------------------------------------------------------------------------------------------------------------------------------
def rc(x: int, k: int) -> int:
    y = 0
    for _ in range(k):
        y = (y << 2) | ((x & 3) ^ 2)
        x >>= 2
    return y


def is_fwd(x: int) -> bool:
    return bin(x).count("1") % 2 == 0


def canon(x: int, k: int):
    """(stored form, t): t = 1 when x is the form that is not stored."""
    return (x, 0) if is_fwd(x) else (rc(x, k), 1)


def sigma(kmers, v: int, k: int) -> int:
    return rc(kmers[v >> 1], k) if v & 1 else kmers[v >> 1]


def masks_of_set(kmers, k: int):
    """The neighbour masks of the stored k-mers of a canonical set against that set (the neighbour is canonicalised, section 6j)."""
    held = set(kmers)
    out = np.zeros(len(kmers), dtype=np.uint8)
    for i, x in enumerate(kmers):
        m = 0
        for j, y in enumerate(nm.neighbors(x, k)):
            if canon(y, k)[0] in held:
                m |= 1 << j
        out[i] = m
    return out


def oriented_edges(kmers, k: int):
    """succ[v] = the ids w with an edge v -> w, straight from the definition (no masks)."""
    assert k % 2 == 1 and all(is_fwd(x) for x in kmers)
    ordinal = {x: i for i, x in enumerate(kmers)}
    assert len(ordinal) == len(kmers)
    succ = []
    for v in range(2 * len(kmers)):
        z = sigma(kmers, v, k)
        ws = []
        for c in range(4):
            y, t = canon(append(z, c, k), k)
            if y in ordinal:
                ws.append(2 * ordinal[y] + t)
        succ.append(ws)
    return succ


def simple_links_by_definition(kmers, k: int):
    succ = oriented_edges(kmers, k)
    n2 = len(succ)
    indeg = [len(succ[v ^ 1]) for v in range(n2)]  # in(i, s) = out(i, 1 - s): the mirror of every in-edge is an out-edge of the mirror
    count_in = [0] * n2
    for v in range(n2):
        for w in succ[v]:
            count_in[w] += 1
    assert count_in == indeg
    nxt = np.full(n2, NONE, dtype=np.uint32)
    prv = np.full(n2, NONE, dtype=np.uint32)
    for v in range(n2):
        if len(succ[v]) == 1:
            w = succ[v][0]
            if indeg[w] == 1 and (w >> 1) != (v >> 1):
                nxt[v] = w
                assert prv[w] == NONE
                prv[w] = v
    for v in range(n2):  # simple edges come in mirror pairs
        if nxt[v] != NONE:
            assert prv[v ^ 1] == (int(nxt[v]) ^ 1)
    return nxt, prv


# ---- (i) the definition: a sequential walk -------------------------------------------------------------------------------------------------------
def _table(n, kept):
    """kept: [(head ordinal, [member ids in offset order], circular)] -> the table, numbered by ascending head."""
    kept = sorted(kept, key=lambda u: u[0])
    t = {"unitig": np.zeros(n, dtype=np.uint32), "offset": np.zeros(n, dtype=np.uint32), "reversed": np.zeros(n, dtype=np.uint8),
         "head": np.array([u[0] for u in kept], dtype=np.uint32), "length": np.array([len(u[1]) for u in kept], dtype=np.uint32),
         "flags": np.array([1 if u[2] else 0 for u in kept], dtype=np.uint8), "n_circular": sum(1 for u in kept if u[2])}
    written = np.zeros(n, dtype=np.int64)
    for number, (_, members, _) in enumerate(kept):
        for off, v in enumerate(members):
            t["unitig"][v >> 1], t["offset"][v >> 1], t["reversed"][v >> 1] = number, off, v & 1
            written[v >> 1] += 1
    assert (written == 1).all()  # every stored k-mer lies on exactly one kept unitig
    return t


def walk_model(kmers, k: int):
    """The table by following the simple edges one oriented k-mer at a time: from every path head, then — what is left lies on pure cycles — from the
    smallest id not yet seen; of every mirror pair one image is kept."""
    nxt, prv = simple_links_by_definition(kmers, k)
    n = len(kmers)
    seen = [False] * (2 * n)
    kept = []

    def follow(h):
        members, v = [], h
        while v != NONE and not seen[v]:
            seen[v] = True
            members.append(v)
            v = int(nxt[v])
        return members, v

    for h in range(2 * n):
        if prv[h] == NONE:
            members, end = follow(h)
            assert end == NONE
            ords = [v >> 1 for v in members]
            assert len(set(ords)) == len(ords)  # no path holds both orientations of a stored k-mer
            hh, tt = members[0] >> 1, members[-1] >> 1
            if hh < tt or (hh == tt and (h & 1) == 0):
                kept.append((hh, members, False))
    for h in range(2 * n):
        if not seen[h]:
            members, end = follow(h)
            assert end == h and len(members) >= 2 and (h >> 1) == min(v >> 1 for v in members)
            if (h & 1) == 0:
                kept.append((h >> 1, members, True))
    t = _table(n, kept)
    t["n_simple"] = int((nxt != NONE).sum()) // 2  # L: mirror pairs of simple edges
    return t


# ---- (ii) the device's route ---------------------------------------------------------------------------------------------------------------------
def links_from_masks(kmers, masks, k: int):
    """next / prev over 2 n ids as k_biunitig_links makes them: the degrees come from the masks alone."""
    ordinal = {x: i for i, x in enumerate(kmers)}
    n = len(kmers)
    nxt = np.full(2 * n, NONE, dtype=np.uint32)
    prv = np.full(2 * n, NONE, dtype=np.uint32)
    for i in range(n):
        m = int(masks[i])
        for s in (0, 1):
            out = (((m >> 4) & 3) << 2 | (m >> 6)) if s else (m & 15)
            if bin(out).count("1") != 1:
                continue
            z = rc(kmers[i], k) if s else kmers[i]
            y, t = canon(append(z, out.bit_length() - 1, k), k)
            r = ordinal[y]
            mr = int(masks[r])
            if r == i or bin((mr & 15) if t else (mr >> 4)).count("1") != 1:
                continue
            nxt[2 * i + s] = 2 * r + t
            assert prv[2 * r + t] == NONE  # one writer
            prv[2 * r + t] = 2 * i + s
    return nxt, prv


def route_model(kmers, k: int, masks=None):
    masks = masks_of_set(kmers, k) if masks is None else masks
    n = len(kmers)
    nxt0, prv0 = links_from_masks(kmers, masks, k)
    anc, dist, nxt, prv, circular, rounds = um.jump_model(nxt0, prv0)
    n2 = 2 * n
    ids = np.arange(n2, dtype=np.int64)
    tail = np.zeros(n2, dtype=np.int64)
    tails = np.flatnonzero(nxt == NONE)
    tail[anc[tails]] = tails  # one writer per head
    is_head = prv == NONE
    h, s, t = ids >> 1, ids & 1, tail >> 1
    keep = is_head & np.where(circular == 1, s == 0, (h < t) | ((h == t) & (s == 0)))
    keep = keep.astype(np.int64)
    uid = np.cumsum(keep) - keep
    nu = int(keep.sum())
    table = {"unitig": np.zeros(n, dtype=np.uint32), "offset": np.zeros(n, dtype=np.uint32), "reversed": np.zeros(n, dtype=np.uint8),
             "head": np.zeros(nu, dtype=np.uint32), "length": np.zeros(nu, dtype=np.uint32), "flags": np.zeros(nu, dtype=np.uint8)}
    if n:
        on = np.flatnonzero(keep[anc] == 1)
        assert np.array_equal(np.sort(on >> 1), np.arange(n))  # each stored k-mer written exactly once
        table["unitig"][on >> 1] = uid[anc[on]]
        table["offset"][on >> 1] = dist[on]
        table["reversed"][on >> 1] = on & 1
        heads = np.flatnonzero(keep == 1)
        table["head"][uid[heads]] = heads >> 1
        table["flags"][uid[heads]] = circular[heads]
        kt = on[nxt[on] == NONE]
        table["length"][uid[anc[kt]]] = dist[kt] + 1
    assert int(circular.sum()) % 2 == 0
    table["n_circular"] = int(circular.sum()) // 2
    table["n_simple"] = int((nxt0 != NONE).sum()) // 2
    table["rounds"] = rounds
    return table


def same_table(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("unitig", "offset", "reversed", "head", "length", "flags")) and a["n_circular"] == b["n_circular"]


def check_identities(t, n: int, n_simple=None):
    """unitigs_model.check_identities (every ordinal once as (unitig, offset), the lengths add up to n, U = n - L + circular, heads ascend), and
    `reversed` holds 0 / 1."""
    um.check_identities(t, n, n_simple=n_simple)
    assert len(t["reversed"]) == n and not (t["reversed"] & 0xFE).any()


# ---- (iii) the text ------------------------------------------------------------------------------------------------------------------------------
def text_model(kmers, t, k: int) -> bytes:
    """Line u = the K letters of sigma(head), the last letter of sigma of every following member in offset order, a newline."""
    nu = len(t["head"])
    members = [[None] * int(ln) for ln in t["length"]]
    for i, (u, off) in enumerate(zip(t["unitig"].tolist(), t["offset"].tolist())):
        members[u][off] = i
    lines = []
    for u in range(nu):
        m = members[u]
        assert m[0] == int(t["head"][u])
        spell = [unpack(sigma(kmers, 2 * i + int(t["reversed"][i]), k), k) for i in m]
        assert all(a[1:] == b[:-1] for a, b in zip(spell, spell[1:]))  # consecutive members overlap by K - 1
        lines.append(spell[0] + "".join(w[-1] for w in spell[1:]))
    text = "".join(ln + "\n" for ln in lines).encode()
    assert len(text) == len(kmers) + nu * k
    return text


def stored_kmers_of_text(text: bytes, k: int):
    """The k-mers of the lines, canonicalised, in line order."""
    return [canon(x, k)[0] for x in um.kmers_of_text(text, k)]


# ---- what a case exercises -----------------------------------------------------------------------------------------------------------------------
def features(kmers, k: int, t, masks=None):
    """circular: a circular unitig of length >= 2; hairpin: an edge (i, s) -> (i, 1 - s); reversed: a unitig of length >= 2 with a reversed member;
    shared: a stored k-mer whose out- and in-nibble name the same stored neighbour (for odd K that neighbour is the k-mer itself: a homopolymer,
    or a k-mer like ATATA whose successor and predecessor are both its own reverse complement — the edges that count in the degrees only)."""
    held = {x: i for i, x in enumerate(kmers)}
    succ = oriented_edges(kmers, k)
    shared = False
    for i, x in enumerate(kmers):
        outs = {held.get(canon(append(x, c, k), k)[0]) for c in range(4)} - {None}
        ins = {held.get(canon(prepend(x, c, k), k)[0]) for c in range(4)} - {None}
        shared = shared or bool(outs & ins)
    long = t["length"][t["unitig"]] >= 2 if len(kmers) else np.zeros(0, dtype=bool)
    return {"circular": bool(((t["flags"] & 1) & (t["length"] >= 2)).any()),
            "hairpin": any((v ^ 1) in ws for v, ws in enumerate(succ)),
            "reversed": bool((long & (t["reversed"] == 1)).any()),
            "shared": shared}


# ---- (iv) crafted inputs: lists of reads (bytes) -------------------------------------------------------------------------------------------------
def revcomp(s: str) -> str:
    return nm.revcomp_str(s)


def cycle_reads(k: int, lengths=(2, 7, 40), seed: int = 23):
    """Pure cycles: s + s[:K - 1] (random sets gave 3 circular unitigs in 900: the cycles must be crafted)."""
    rng = random.Random(seed + k)
    out = []
    for ln in lengths:
        s = "AC" if ln == 2 else _rand(rng, ln)  # ACAC..A / CACA..C: a 2-cycle
        while not nm._primitive(s):
            s = _rand(rng, ln)
        out.append(((s * (k // ln + 2))[: ln + k - 1]).encode())
    return out


def hairpin_reads(k: int, seed: int = 29):
    u = _rand(random.Random(seed + k), 3 * k)
    return [(u + revcomp(u)).encode()]


def strand_reads(k: int, seed: int = 31):
    """(first, second): a read, then its reverse complement — the same stored k-mers, nothing new in the second flush."""
    r = _rand(random.Random(seed + k), 200 + k)
    return [r.encode()], [revcomp(r).encode()]


def reversed_overlap_reads(k: int, seed: int = 37):
    """(first, second): a + b, then rc(b + c): one unitig a + b + c through both reads, with members stored in either orientation."""
    rng = random.Random(seed + k)
    a, b, c = _rand(rng, 60), _rand(rng, 2 * k), _rand(rng, 60)
    return [(a + b).encode()], [revcomp(b + c).encode()]


def homopolymer_reads(k: int):
    return [(ch * k).encode() for ch in NUCS]


def at_repeat_reads(k: int):
    return [("AT" * k)[:k].encode()]  # its successor by T is its own reverse complement


def stored_kmers_of_reads(reads, k: int):
    """Distinct stored forms of the k-mers of the reads, in first-occurrence order (NOT the iteration order: for the CPU tests that need a set only)."""
    seen, out = set(), []
    for r in reads:
        r = r.decode()
        for i in range(len(r) - k + 1):
            x = canon(pack(r[i: i + k]), k)[0]
            if x not in seen:
                seen.add(x)
                out.append(x)
    return out


CRAFTED = ["graph15", "graph31", "graph33", "graph59", "edges31", "edges33", "dense", "cycles", "hairpin", "strands", "overlap", "branch", "homopolymers", "at"]


def crafted(name):
    """(k, pb, flushes) of a crafted case: the CPU and the GPU tests insert the same flushes into a canonical index."""
    if name.startswith("graph"):
        k = int(name[5:])
        g = nm.Graph(k)
        return k, {15: 6, 31: 24, 33: 16, 59: 28}[k], [g.batch1, g.batch2]
    if name.startswith("edges"):
        k = int(name[5:])
        return k, 24 if k == 31 else 16, [um.path_edge_reads(k)]
    k, pb = 31, 24
    if name == "dense":
        return 9, 4, [um.dense_reads()]
    if name == "cycles":
        return k, pb, [cycle_reads(k)]
    if name == "hairpin":
        return k, pb, [hairpin_reads(k)]
    if name == "strands":
        return k, pb, list(strand_reads(k))
    if name == "overlap":
        return k, pb, list(reversed_overlap_reads(k))
    if name == "branch":
        return k, pb, list(um.branch_reads(k))
    if name == "homopolymers":
        return k, pb, [homopolymer_reads(k)]
    assert name == "at"
    return k, pb, [at_repeat_reads(k)]
