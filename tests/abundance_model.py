"""K-mer abundances on the CPU: the tally of a batch of reads into an array of counts by ordinal, the spectrum, the coverage of
the unitigs, the GFA text with LN / KC tags, and the filter under both rules as one WordSet::remove_batch on an oracle.pyref.PyCBL; and the crafted inputs
of the CPU and the GPU tests. Pure CPU; no expectation comes from the GPU path. A helper, not a test file.

    occurrence      one word of the oracle's own enumeration of a batch (Oracle.seq_words, or oracle.pyref.seq_words for a PyCBL): sequence after sequence,
                    get_seq_words order, invalid bytes skipped as the oracle skips them; a sequence shorter than K gives none
    ordinal         the index of a stored word in the iteration order (Oracle.iter_words / tips_model.iteration_words)
    tally           counts[i] = min(2^32 - 1, counts[i] + occurrences whose word has ordinal i)
    spectrum        hist[j] = ordinals with counts == j for j < 255, hist[255] = those with counts >= 255
    kc[u]           the sum of counts over the k-mers of unitig u of gfa_model.walk_model's table
    tagged text     gfa_model's text with "\\tLN:i:<length + K - 1>" and, with counts, "\\tKC:i:<kc>" behind the letters of every S line
    filter          k-mer rule: counts[i] < min_count; unitig rule: kc[u] < min_count * length[u]; the selected words in iteration order, one remove_batch"""
from __future__ import annotations

import random

import numpy as np

from oracle import pyref
from oracle.pyref import PyCBL

import gfa_model as gm
import removal_model as rm
import tips_model as tm
from neighbors_model import _rand, revcomp_str

MAX = (1 << 32) - 1
STATS = ("kmers", "removed_kmers", "unitigs", "removed_unitigs", "kmers_left", "min_count")


# ---- occurrences and the tally -------------------------------------------------------------------------------------------------------------------------
def enumerate_words(o, seq: bytes):
    """The words of one sequence as `o` (an oracle.Oracle or a PyCBL) enumerates them; none for a sequence shorter than K."""
    k = o.k if hasattr(o, "seq_words") else o.P["K"]
    if len(seq) < k:
        return []
    return o.seq_words(seq) if hasattr(o, "seq_words") else pyref.seq_words(seq, o.P, o.canonical)


def occurrences(o, seqs):
    return [w for s in seqs for w in enumerate_words(o, s)]


def iteration_order(o):
    """The stored words in iteration order."""
    return o.iter_words() if hasattr(o, "iter_words") else tm.iteration_words(o)


def ordinals(words):
    return {w: i for i, w in enumerate(words)}


def accumulate(counts, hits):
    """counts (uint32 array) + hits (int per ordinal), saturating: a new uint32 array."""
    s = np.asarray(counts, dtype=np.uint32).astype(np.uint64) + np.asarray(hits, dtype=np.uint64)
    return np.minimum(s, MAX).astype(np.uint32)


def tally_model(o, seqs, counts=None, order=None):
    """(counts after, total, found) of one tally call on the index `o` holds; counts = None: zeros."""
    order = iteration_order(o) if order is None else order
    rank = ordinals(order)
    hits = np.zeros(len(order), dtype=np.uint64)
    total = found = 0
    for w in occurrences(o, seqs):
        total += 1
        i = rank.get(w)
        if i is not None:
            found += 1
            hits[i] += 1
    before = np.zeros(len(order), dtype=np.uint32) if counts is None else counts
    assert len(before) == len(order)
    return accumulate(before, hits), total, found


def spectrum(counts):
    c = np.minimum(np.asarray(counts, dtype=np.uint32).astype(np.int64), 255)
    return np.bincount(c, minlength=256).astype(np.uint64)


def solid_threshold(hist):
    """The rule of CBL.solid_threshold, restated by its definition: the first bin j >= 1 of the first run of equal bins that is followed by a higher bin."""
    h = [int(v) for v in hist]
    for j in range(1, len(h) - 1):
        e = j
        while e + 1 < len(h) and h[e + 1] == h[j]:
            e += 1
        if e + 1 < len(h) and h[e + 1] > h[j] and (j == 1 or h[j - 1] != h[j]):
            return j
    return None


# ---- coverage and the tagged text ----------------------------------------------------------------------------------------------------------------------
def kc_model(table, counts):
    kc = [0] * len(table["head"])
    for u, c in zip(table["unitig"].tolist(), np.asarray(counts, dtype=np.uint32).tolist()):
        kc[u] += c
    return kc  # Python ints: up to length * (2^32 - 1)


def tagged_text(text: bytes, table, k: int, kc=None) -> bytes:
    """gfa_model's text with the tags of section 6p on the S lines; the H line and the L lines as they are."""
    out = []
    for row in text.split(b"\n")[:-1]:
        if row.startswith(b"S\t"):
            u = int(row.split(b"\t")[1])
            row += b"\tLN:i:%d" % (int(table["length"][u]) + k - 1)
            if kc is not None:
                row += b"\tKC:i:%d" % kc[u]
        out.append(row + b"\n")
    return b"".join(out)


def untag(text: bytes):
    """(the text without tags, [(u, LN, KC or None)]) of a tagged text, parsed without a model."""
    out, tags = [], []
    for row in text.split(b"\n")[:-1]:
        f = row.split(b"\t")
        if f[0] == b"S":
            assert len(f) in (4, 5) and f[3].startswith(b"LN:i:") and (len(f) == 4 or f[4].startswith(b"KC:i:"))
            ln, kc = f[3][5:], (f[4][5:] if len(f) == 5 else None)
            for num in (ln,) + ((kc,) if kc is not None else ()):
                assert num.isdigit() and (num == b"0" or not num.startswith(b"0"))  # decimal without padding
            assert int(ln) == len(f[2])
            tags.append((int(f[1]), int(ln), None if kc is None else int(kc)))
            row = b"\t".join(f[:3])
        out.append(row + b"\n")
    return b"".join(out), tags


# ---- the filter ------------------------------------------------------------------------------------------------------------------------------------------
def select_model(counts, min_count: int, table=None):
    """Per ordinal, whether the k-mer goes; table = None: the k-mer rule; else the unitig rule on gfa_model.walk_model's table. Also the unitigs that go."""
    assert min_count >= 1
    c = np.asarray(counts, dtype=np.uint32)
    if table is None:
        return c < min_count, []
    kc = kc_model(table, c)
    gone = [u for u, ln in enumerate(table["length"].tolist()) if kc[u] < min_count * ln]
    flag = np.zeros(len(kc), dtype=bool)
    flag[gone] = True
    return (flag[table["unitig"].astype(np.int64)] if len(c) else np.zeros(0, dtype=bool)), gone


def table_of(m: PyCBL):
    words = tm.iteration_words(m)
    kmers = [tm.kmer_of_word(w, m.P) for w in words]
    return gm.walk_model(kmers, m.P["K"], m.canonical)


def filter_model(m: PyCBL, counts, min_count: int, unitigs: bool, table=None):
    """cblx_abundance_filter on m, in place: the stats. An empty index: all zero."""
    st = dict.fromkeys(STATS, 0)
    words = tm.iteration_words(m)
    assert len(counts) == len(words)
    if not words:
        return st
    st["kmers"], st["min_count"] = len(words), min_count
    if unitigs:
        table = table_of(m) if table is None else table
        st["unitigs"] = len(table["head"])
    sel, gone = select_model(counts, min_count, table if unitigs else None)
    st["removed_kmers"], st["removed_unitigs"] = int(sel.sum()), len(gone)
    if sel.any():
        rm.remove_batch(m, [w for w, f in zip(words, sel.tolist()) if f])
    st["kmers_left"] = m.count()
    return st


# ---- crafted counts --------------------------------------------------------------------------------------------------------------------------------------
def spread(total: int, length: int, ordinals_of_unitig, counts):
    """Sets the counts of a unitig's k-mers so that they add up to `total`: as even as the ceiling allows, the remainder on the first ones."""
    assert 0 <= total <= length * MAX and len(ordinals_of_unitig) == length
    q, r = divmod(total, length)
    for j, i in enumerate(ordinals_of_unitig):
        counts[i] = q + (1 if j < r else 0)


def members(table):
    """Per unitig, the ordinals of its k-mers."""
    out = [[] for _ in table["head"]]
    for i, u in enumerate(table["unitig"].tolist()):
        out[u].append(i)
    return out


DIGIT_TARGETS = [v for e in range(1, 13) for v in (10 ** e - 1, 10 ** e)]  # 9, 10, 99, 100, ... 10^12 - 1, 10^12


def digit_counts(table):
    """Counts (uint32) that make kc hit DIGIT_TARGETS on the unitigs long enough for them, the largest targets on the longest unitigs; the longest
    unitig of all is at 2^32 - 1 per k-mer, every unitig without a target at 0 or 1 by turns. Returns (counts, kc)."""
    mem = members(table)
    n = len(table["unitig"])
    counts = np.zeros(n, dtype=np.uint32)
    by_len = sorted(range(len(mem)), key=lambda u: (-len(mem[u]), u))
    top = by_len[0]
    counts[mem[top]] = MAX
    free = by_len[1:]
    for t in sorted(DIGIT_TARGETS, reverse=True):
        for u in free:
            if len(mem[u]) * MAX >= t:
                spread(t, len(mem[u]), mem[u], counts)
                free.remove(u)
                break
        else:
            raise AssertionError(f"no unitig can hold kc = {t}")
    for j, u in enumerate(free):
        counts[mem[u]] = j & 1
    return counts, kc_model(table, counts)


def kmer_edge_counts(n: int, min_count: int, seed: int = 3):
    """Counts at min_count - 1 and min_count, with 0, min_count + 1 and 2^32 - 1 among them."""
    rng = random.Random(seed + n)
    vals = [min_count - 1, min_count, min_count - 1, min_count, 0, min_count + 1, MAX]
    return np.array([vals[rng.randrange(len(vals))] if i >= len(vals) else vals[i] for i in range(n)], dtype=np.uint32)


def unitig_edge_counts(table, min_count: int):
    """kc[u] = min_count * length[u] - 1 (goes), exactly min_count * length[u] (stays) and 0 by turns over the unitigs, spread unevenly where the unitig
    has two k-mers or more: its first k-mer takes what the others, at min_count + 1 each, leave — so the two rules select differently."""
    mem = members(table)
    counts = np.zeros(len(table["unitig"]), dtype=np.uint32)
    for u, ords in enumerate(mem):
        ln = len(ords)
        total = (min_count * ln - 1, min_count * ln, 0)[u % 3]
        rest = min(total, (min_count + 1) * (ln - 1))
        if ln > 1:
            spread(rest, ln - 1, ords[1:], counts)
        counts[ords[0]] = total - rest
    return counts


# ---- crafted reads ---------------------------------------------------------------------------------------------------------------------------------------
def long_unitig_reads(k: int, seed: int = 61, long_ones: int = 26, kmers: int = 300, singles: int = 4):
    """`long_ones` random reads of `kmers` k-mers each — isolated unitigs long enough for kc up to 10^12 and for 300 k-mers at 2^32 - 1 — and `singles`
    reads of one k-mer."""
    rng = random.Random(seed + k)
    return [_rand(rng, kmers + k - 1).encode() for _ in range(long_ones)] + [_rand(rng, k).encode() for _ in range(singles)]


def tally_reads(k: int, index_reads, seed: int = 67):
    """Named batches against an index built of index_reads (bytes): the contents the tally has to get right."""
    rng = random.Random(seed + k)
    src = max(index_reads, key=len)  # the two halves of the longest read
    assert len(src) >= 4 * k + 4
    r0, r1 = src[: len(src) // 2], src[len(src) // 2:]
    filler = [_rand(rng, k + 40).encode() for _ in range(30)]  # reads that miss
    dirty = bytearray(r0)
    dirty[k + 3] = ord("N")
    dirty[k + 9: k + 12] = bytes(dirty[k + 9: k + 12]).lower()
    dirty[2 * k + 1] = ord("-")
    return {
        "poly-a": [b"A" * 300],
        "far-apart": [r0[: k + 5]] + filler[:15] + [r0[: k + 5]] + filler[15:] + [r0[2: k + 4]],
        "both-strands": [r1, revcomp_str(r1.decode()).encode()],
        "dirty": [bytes(dirty), bytes(dirty).lower(), b"N" * (k + 3) + r1[: k + 2] + b"n"],
        "short": [r0[: k - 1], r1[: k], b"ACG", r0[5: 5 + k + 1]],
        "only-short": [r0[: k - 1], b""],
        "none": [],
        "miss": filler[:5],
    }


def exact_batch(k: int, index_reads, nk: int):
    """A batch of exactly nk k-mers out of the index's own reads: whole pieces of at most 40 k-mers."""
    out, left, j = [], nk, 0
    while left:
        src = index_reads[j % len(index_reads)]
        m = min(left, 40, len(src) - k + 1)
        out.append(src[: m + k - 1])
        left -= m
        j += 1
    return out
