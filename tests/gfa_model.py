"""Links between unitigs and the GFA text on the CPU, in both forms: the plain unitigs of a non-canonical set (section 6k,
tests/unitigs_model.py) and the bidirected ones of a canonical set with odd K (section 6l, tests/biunitigs_model.py). (i) The definition: every edge
of the graph, enumerated from the set, classified against walk_model's table. (ii) The route the device takes, restated with numpy: counts from the
masks and the table, the fill through a rank dictionary, the side from `reversed`. (iii) The GFA text, on text_model of the two models, and its way back
to the edge set without any model. Pure CPU; no expectation comes from the GPU path. A helper, not a test file.

    image, slot     unitig u has its kept image, side 0 ('+'), and in the bidirected form its mirror, side 1 ('-'): the oriented k-mers (i, 1 - s) in
                    reverse offset order. Slot 2 u + side; in the plain form only even slots hold anything.
    link            every edge (self-edges and hairpins included) that does not join two consecutive offsets of one image
    link table      link_start (uint64, 2 U + 1: the CSR over the slots), link_to (uint32: the target unitig), link_rev (uint8: 0 = the target is entered
                    at the head of its kept image, 1 = at the head of its mirror); within a slot by ascending code of the appended base
    mirror          of the link a -> b (slot ids) the link b ^ 1 -> a ^ 1; the GFA text writes the one whose pair is lexicographically <= the other's"""
from __future__ import annotations

import numpy as np

import biunitigs_model as bm
import unitigs_model as um
from neighbors_model import NUCS, append, revcomp_str, unpack  # noqa: F401  (re-exported for the tests)

HEADER = b"H\tVN:Z:1.0\n"


def walk_model(kmers, k: int, canonical: bool):
    """The table of the form: `reversed` is all 0 in the plain form."""
    if canonical:
        return bm.walk_model(kmers, k)
    t = um.walk_model(kmers, k)
    t["reversed"] = np.zeros(len(kmers), dtype=np.uint8)
    return t


def masks_of_set(kmers, k: int, canonical: bool):
    return bm.masks_of_set(kmers, k) if canonical else um.masks_of_set(kmers, k)


def text_model(kmers, t, k: int, canonical: bool) -> bytes:
    return bm.text_model(kmers, t, k) if canonical else um.text_model(kmers, t, k)


# ---- (i) the definition ----------------------------------------------------------------------------------------------------------------------------
def edges(kmers, k: int, canonical: bool):
    """[(v, c, w)]: every edge of the graph from oriented k-mer v by base c to w, straight from the set. Ids are 2 i + s in both forms (s = 0 only in the
    plain one)."""
    out = []
    if canonical:
        for v, ws in enumerate(_succ_with_bases(kmers, k)):
            out += [(v, c, w) for c, w in ws]
        return out
    ordinal = {x: i for i, x in enumerate(kmers)}
    for i, x in enumerate(kmers):
        for c in range(4):
            j = ordinal.get(append(x, c, k))
            if j is not None:
                out.append((2 * i, c, 2 * j))
    return out


def _succ_with_bases(kmers, k: int):
    """biunitigs_model.oriented_edges with the base of every edge (and checked against it)."""
    ordinal = {x: i for i, x in enumerate(kmers)}
    succ = []
    for v in range(2 * len(kmers)):
        z = bm.sigma(kmers, v, k)
        ws = []
        for c in range(4):
            y, t = bm.canon(append(z, c, k), k)
            if y in ordinal:
                ws.append((c, 2 * ordinal[y] + t))
        succ.append(ws)
    assert [[w for _, w in ws] for ws in succ] == bm.oriented_edges(kmers, k)
    return succ


def place(t, v: int):
    """(unitig, side, position) of oriented k-mer v = 2 i + s on the image of its unitig that holds it."""
    i, s = v >> 1, v & 1
    u, off = int(t["unitig"][i]), int(t["offset"][i])
    side = int(s != int(t["reversed"][i]))
    return u, side, (int(t["length"][u]) - 1 - off) if side else off


def links_by_definition(kmers, k: int, canonical: bool, t):
    """[(from slot, base, to slot, leaves a tail, enters a head)] of every edge that does not join two consecutive offsets of one image, in table
    order."""
    out = []
    for v, c, w in edges(kmers, k, canonical):
        (u1, side1, p1), (u2, side2, p2) = place(t, v), place(t, w)
        if u1 == u2 and side1 == side2 and p2 == p1 + 1:
            continue
        out.append((2 * u1 + side1, c, 2 * u2 + side2, p1 == int(t["length"][u1]) - 1, p2 == 0))
    out.sort(key=lambda e: (e[0], e[1]))
    return out


def table_of_links(links, nu: int):
    """The link table of [(from slot, base, to slot, ...)] in table order."""
    start = np.zeros(2 * nu + 1, dtype=np.uint64)
    for e in links:
        start[e[0] + 1] += 1
    start = np.cumsum(start).astype(np.uint64)
    return {"link_start": start, "link_to": np.array([e[2] >> 1 for e in links], dtype=np.uint32),
            "link_rev": np.array([e[2] & 1 for e in links], dtype=np.uint8), "n_unitigs": nu, "n_links": len(links)}


def definition_model(kmers, k: int, canonical: bool, t=None):
    t = walk_model(kmers, k, canonical) if t is None else t
    links = links_by_definition(kmers, k, canonical, t)
    assert all(tail and head for _, _, _, tail, head in links)  # every link leaves the tail of an image and enters the head of one
    assert len({(e[0], e[2]) for e in links}) == len(links)  # two links never share both end slots
    return table_of_links(links, len(t["head"]))


# ---- (ii) the device's route -----------------------------------------------------------------------------------------------------------------------
def out_nibble(m: int, s: int) -> int:
    """The out-nibble of (i, s) from the mask of stored k-mer i: bit c of the out-nibble of (i, 1) is bit 4 + (c ^ 2) of the mask."""
    return ((((m >> 4) & 3) << 2) | (m >> 6)) if s else (m & 15)


def route_model(kmers, k: int, canonical: bool, t=None, masks=None):
    """k_gfa_link_counts, the scan, k_gfa_link_fill: counts from the masks at the tails of the images, targets through the rank of the appended word."""
    t = walk_model(kmers, k, canonical) if t is None else t
    masks = masks_of_set(kmers, k, canonical) if masks is None else masks
    n, nu = len(kmers), len(t["head"])
    cnt = np.zeros(2 * nu, dtype=np.uint32)
    for i in range(n):
        u, off, rev, m = int(t["unitig"][i]), int(t["offset"][i]), int(t["reversed"][i]), int(masks[i])
        if off + 1 == int(t["length"][u]):
            cnt[2 * u] = bin(out_nibble(m, rev)).count("1")
        if canonical and off == 0:
            cnt[2 * u + 1] = bin(out_nibble(m, rev ^ 1)).count("1")
    start = np.concatenate([[0], np.cumsum(cnt.astype(np.uint64))]).astype(np.uint64)
    nl = int(start[-1])
    to, rv = np.full(nl, 0xFFFFFFFF, dtype=np.uint32), np.full(nl, 0xFF, dtype=np.uint8)
    rank = {x: i for i, x in enumerate(kmers)}
    for i in range(n):
        for s in ((0, 1) if canonical else (0,)):
            u, off, rev = int(t["unitig"][i]), int(t["offset"][i]), int(t["reversed"][i])
            side = 0 if s == rev else 1
            if (off + 1 != int(t["length"][u])) if side == 0 else (off != 0):
                continue
            z = bm.rc(kmers[i], k) if s else kmers[i]
            at = int(start[2 * u + side])
            for c in range(4):
                if not (out_nibble(int(masks[i]), s) >> c) & 1:
                    continue
                y, tt = bm.canon(append(z, c, k), k) if canonical else (append(z, c, k), 0)
                r = rank[y]
                assert to[at] == 0xFFFFFFFF  # one writer
                to[at], rv[at] = t["unitig"][r], int(int(t["reversed"][r]) != tt)
                at += 1
            assert at == int(start[2 * u + side + 1])
    assert nl == 0 or (int(to.max()) < nu and int(rv.max()) <= 1)  # every element written
    return {"link_start": start, "link_to": to, "link_rev": rv, "n_unitigs": nu, "n_links": nl}


def same_links(a, b):
    return all(np.array_equal(a[key], b[key]) for key in ("link_start", "link_to", "link_rev")) and a["n_unitigs"] == b["n_unitigs"] and a["n_links"] == b["n_links"]


def slot_pairs(lt):
    """[(from slot, to slot)] of a link table, in table order."""
    start = [int(s) for s in lt["link_start"]]
    return [(a, 2 * int(lt["link_to"][ln]) + int(lt["link_rev"][ln])) for a in range(len(start) - 1) for ln in range(start[a], start[a + 1])]


def written(pair, canonical: bool) -> bool:
    """Whether the GFA text writes the link: of a mirror pair the one whose (from, to) is lexicographically <= its mirror's (to ^ 1, from ^ 1)."""
    a, b = pair
    return not canonical or (a, b) <= (b ^ 1, a ^ 1)


# ---- (iii) the text --------------------------------------------------------------------------------------------------------------------------------
def gfa_model(kmers, k: int, canonical: bool, t, lt) -> bytes:
    lines = text_model(kmers, t, k, canonical).split(b"\n")[:-1]
    assert len(lines) == lt["n_unitigs"]
    out = [HEADER] + [b"S\t%d\t%s\n" % (u, ln) for u, ln in enumerate(lines)]
    for a, b in slot_pairs(lt):
        if written((a, b), canonical):
            out.append(b"L\t%d\t%s\t%d\t%s\t%dM\n" % (a >> 1, b"-" if a & 1 else b"+", b >> 1, b"-" if b & 1 else b"+", k - 1))
    return b"".join(out)


def n_l_lines(lt, canonical: bool) -> int:
    return sum(1 for p in slot_pairs(lt) if written(p, canonical))


def k1mers_of_gfa(text: bytes, k: int, canonical: bool):
    """The set of (K + 1)-mers (str) the text spells: inside the S lines, and across every L line — the last K letters of the first segment in its
    orientation and the letter that follows the overlap in the second; closed under reverse complement where `canonical`. No model is used."""
    rows = text.decode().split("\n")
    assert rows[0] == HEADER.decode().rstrip("\n") and rows[-1] == ""
    seg, out = {}, set()
    for row in rows[1:-1]:
        f = row.split("\t")
        if f[0] == "S":
            assert int(f[1]) == len(seg) and len(f) == 3  # numbered 0 .. U - 1 in order
            seg[int(f[1])] = f[2]
            out |= {f[2][i: i + k + 1] for i in range(len(f[2]) - k)}
        else:
            assert f[0] == "L" and len(f) == 6 and f[5] == "%dM" % (k - 1) and f[2] in "+-" and f[4] in "+-"
            a = seg[int(f[1])] if f[2] == "+" else revcomp_str(seg[int(f[1])])
            b = seg[int(f[3])] if f[4] == "+" else revcomp_str(seg[int(f[3])])
            assert a[len(a) - (k - 1):] == b[: k - 1]  # the overlap is K - 1 letters
            out.add(a[len(a) - k:] + b[k - 1])
    if canonical:
        out |= {revcomp_str(w) for w in out}
    return out


def k1mers_of_set(kmers, k: int, canonical: bool):
    """The edge set of S as (K + 1)-mers (str): both K-mers of the word are in the set (canonicalised where `canonical`)."""
    held = set(kmers)
    has = (lambda x: bm.canon(x, k)[0] in held) if canonical else (lambda x: x in held)
    out = set()
    for x in kmers:
        for z in ((x, bm.rc(x, k)) if canonical else (x,)):
            for c in range(4):
                if has(append(z, c, k)):
                    out.add(unpack(z, k) + NUCS[c])
    return out
