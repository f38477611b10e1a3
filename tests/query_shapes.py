"""Crafted resident sets for the read side (k_contains, k_query_join, k_export_kmers): buckets of an exact length, and the
queries that hit and miss them. Pure CPU: `oracle.Oracle` for the words of a sequence, `random` / numpy for the rest.

`craft` starts from a seeded random genome G. `o.seq_words(G)` gives every k-mer's word in stream order; the distinct words,
grouped by prefix, are the candidates. For every target length one prefix with enough candidates gives a random subset of
exactly that length as its resident bucket; the other candidates of the prefix are misses that share the bucket (below,
between and above the resident elements), and the words of every prefix that was not picked miss the directory. Each length
gets up to two buckets: "inner" leaves the smallest and the largest candidate out (keys below the first and above the last
element), "outer" keeps both (hits on the first and the last element). The expected flags are `word in set(resident)`.

Necklace prefixes are heavily skewed (the smallest rotation of a random k-mer starts with A A ...), so a plain random genome
fills one or two prefixes at PREFIX_BITS <= 6. G is therefore a chain of segments, each drawn at random under a rule that
steers where its necklaces start: the bases of a segment are >= X, and X is only followed by bases >= Y (order A C T G, the
2-bit codes), for the nine pairs X <= Y below; for PREFIX_BITS = 16 a segment without A carries an A-rich 8-base motif every
`MOTIF_PERIOD` bases instead, and the k-mers that hold one motif share its prefix.
"""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np

from oracle import Oracle, pyref

QL = 8                # kernels_bucket.hpp QL: lanes per query of k_contains, the width of its last equality step
QL1 = QL + 1          # kernels_bucket.hpp (QL + 1u): fan-out of the Trie search, the first length that takes a search step
THRESHOLD = 1024      # common.hpp VEC_THRESHOLD (Consts "threshold"): a batch leaves a Vec up to here, a Trie beyond
JOIN_FULL_MAX = 2730  # kernels_kmer.hpp JOIN_FULL_MAX: longest bucket whose suffixes go into the "full" LDS table
JOIN_TAB_MAX = 4095   # kernels_kmer.hpp JOIN_TAB_MAX: longest bucket of the tag / index LDS table; longer ones are searched or scanned
VEC, TRIE = 0, 1      # kernels_bucket.hpp KIND_VEC / KIND_TRIE

# every length at which k_contains or k_query_join takes another path, and its neighbours
EDGE_LENGTHS = (1, QL, QL1, THRESHOLD, THRESHOLD + 1, JOIN_FULL_MAX - 1, JOIN_FULL_MAX, JOIN_FULL_MAX + 1, JOIN_TAB_MAX - 1, JOIN_TAB_MAX,
                JOIN_TAB_MAX + 1, JOIN_TAB_MAX + 2)
# the Trie search's fan-out cubed (9^3 = 729: one more step from 730 on) and the longest Vec-sized Trie
SHORT_TRIE_LENGTHS = tuple(range(1, 101)) + (QL1 ** 3 - 1, QL1 ** 3, QL1 ** 3 + 1, THRESHOLD - 1)

_ORDER = b"ACTG"  # 2-bit codes 0 .. 3
_STYLES = [(x, y) for x in range(3) for y in range(x, 4)]
MOTIF_PERIOD = 41  # K = 33: a k-mer holds at most one whole motif
MOTIFS_16 = tuple(b"AAAAA" + bytes([a, b, c]) for a in b"CT" for b in b"CTG" for c in b"CT")  # twelve prefixes at PREFIX_BITS = 16

Bucket = namedtuple("Bucket", "prefix length kind edges elements candidates")  # edges: "inner" / "outer"; both lists ascending words
Shape = namedtuple("Shape", "k pb canonical sb genome words resident expected buckets")


def batch_kind(length):
    """What one batch into an empty index leaves (src/wordset/mod.rs:213-214)."""
    return VEC if length <= THRESHOLD else TRIE


def _segment(rng, n, x, y, motif=b"", period=0):
    out = bytearray()
    prev = None
    while len(out) < n:
        if motif and len(out) % period == 0:
            out += motif
            prev = motif[-1]
            continue
        b = _ORDER[rng.randrange(y if prev == _ORDER[x] else x, 4)]
        out.append(b)
        prev = b
    return bytes(out[:n])


def genome(seed, seglen, motifs=()):
    rng = random.Random(seed)
    if motifs:
        return b"".join(_segment(rng, seglen, 1, 1, m, MOTIF_PERIOD) for m in motifs)
    return b"".join(_segment(rng, seglen, x, y) for x, y in _STYLES)


def candidates_by_prefix(words, sb):
    by = {}
    for w in set(words):
        by.setdefault(w >> sb, []).append(w)
    for v in by.values():
        v.sort()
    return by


def craft(k, pb, canonical, targets, seed, seglen, motifs=(), first="inner", kind_of=batch_kind, ascending=False):
    """A Shape whose resident words fill one bucket ("inner") or two ("inner" and "outer") of every length in `targets`.

    Lengths are served longest first, each from the prefix with the fewest candidates that still has length + 3 of them (so
    that the long ones keep the crowded prefixes) as `first` says; a second round hands the prefixes left over, but one, to buckets of the other
    edges the same way. `resident` is shuffled (the order of insertion: a Vec keeps it), or ascending for the recipe that installs Tries."""
    rng = random.Random(seed)
    o = Oracle(k, pb, canonical)
    G = genome(seed, seglen, motifs)
    words = o.seq_words(G)
    sb = pyref.params(k, pb)["SB"]
    by = candidates_by_prefix(words, sb)
    free = sorted(by, key=lambda p: (len(by[p]), p))
    buckets = {}
    for edges in (first, "outer" if first == "inner" else "inner"):
        for n in sorted(targets, reverse=True):
            p = next((p for p in free if len(by[p]) >= n + 3), None)
            if p is None or (edges != first and len(free) == 1):  # (one populated prefix stays without a bucket)
                continue
            free.remove(p)
            cand = by[p]
            if edges == "inner":
                el = sorted(rng.sample(cand[1:-1], n))
                while n >= 2 and cand.index(el[-1]) - cand.index(el[0]) == n - 1:  # no miss between the elements: draw again
                    el = sorted(rng.sample(cand[1:-1], n))
            else:
                el = sorted([cand[0], cand[-1]][: n] + rng.sample(cand[1:-1], max(n - 2, 0)))
            buckets[p] = Bucket(p, n, kind_of(n), edges, el, cand)
    resident = [w for p in sorted(buckets) for w in buckets[p].elements]
    if not ascending:
        rng.shuffle(resident)
    rs = set(resident)
    expected = np.fromiter((w in rs for w in words), dtype=bool, count=len(words))
    return Shape(k, pb, canonical, sb, G, words, resident, expected, buckets)


def delivered(shape):
    """{length: [edges of its buckets]}: what the shape reaches."""
    out = {}
    for b in shape.buckets.values():
        out.setdefault(b.length, []).append(b.edges)
    return out


def border_words(bucket):
    """The four border candidates: smallest / largest resident element, smallest / largest candidate of the prefix."""
    return [bucket.elements[0], bucket.elements[-1], bucket.candidates[0], bucket.candidates[-1]]


def bucket_of(shape, word):
    """(prefix, length, kind, rank of the word among the elements) for a failure message."""
    import bisect

    b = shape.buckets.get(word >> shape.sb)
    return None if b is None else (b.prefix, b.length, b.kind, bisect.bisect_left(b.elements, word))


def iteration_order(shape):
    """CBL::iter over the crafted index: prefixes ascending, a Vec as inserted, a Trie ascending (words)."""
    stored = {}
    for w in shape.resident:
        stored.setdefault(w >> shape.sb, []).append(w)
    out = []
    for p in sorted(shape.buckets):
        out += stored[p] if shape.buckets[p].kind == VEC else shape.buckets[p].elements
    return out


def shares(shape, n):
    """The resident words dealt into n disjoint lists, every bucket's elements in equal parts (for `|=`)."""
    out = [[] for _ in range(n)]
    stored = {}
    for w in shape.resident:
        stored.setdefault(w >> shape.sb, []).append(w)
    for p in sorted(stored):
        for i, w in enumerate(stored[p]):
            out[i * n // len(stored[p])].append(w)
    return out


def all_but_one(k, pb, n_kmers, seed, absent):
    """A random sequence of n_kmers k-mers with distinct words, and its words without the one at index `absent` (None: all)."""
    rng = random.Random(seed)
    o = Oracle(k, pb)
    seq = bytes(rng.choice(b"ACGT") for _ in range(n_kmers + k - 1))
    words = o.seq_words(seq)
    assert len(words) == n_kmers == len(set(words))
    return seq, words, [w for i, w in enumerate(words) if i != absent]


# ---- the parameter sets of tests/test_gpu_query_classes.py; tests/test_query_shapes.py pins what each delivers -------------------
# name -> (k, pb, canonical, targets, seed, seglen, motifs[, first]). Shapes with few populated prefixes come in two rounds, the
# second with "outer" buckets.
_E = EDGE_LENGTHS
EDGE_SHAPES = {
    "15-6": (15, 6, False, _E, 1, 14000, ()),                  # narrow word, SB = 29: all four join classes
    "31-5": (31, 5, False, _E, 2, 14000, ()),                  # SB = 63: `full` still applies
    "31-4-a": (31, 4, False, (1, QL1, 1025, 2731, 4095, 4096), 3, 14000, ()),   # SB = 64: never `full`, the tag table from length 1
    "31-4-b": (31, 4, False, (QL, 1024, 2730, 4094, 4097), 4, 14000, (), "outer"),
    "31-3-a": (31, 3, False, (QL1, 1025, 4095, 4096), 5, 14000, ()),           # SB = 65: wide suffix, no flags by join
    "31-3-b": (31, 3, False, (QL, 1024, 4094, 4097), 6, 14000, (), "outer"),
    "33-16": (33, 16, False, _E, 7, 14000, MOTIFS_16),         # wide word, narrow suffix: hi bits under the ordinal
    "45-6": (45, 6, False, _E, 8, 14000, ()),                  # WB = 97 > 96: tallies by join, flags per query
    "15-6-canonical": (15, 6, True, _E, 9, 14000, ()),
}
SHORT_TRIE_SHAPE = (15, 10, False, SHORT_TRIE_LENGTHS, 10, 17000, ())
MERGE_SHAPES = {"15-6": (15, 6, False, (4500, 2500), 11, 14000, ()), "35-6": (35, 6, False, (4500, 2500), 12, 14000, ())}
MERGE_SHARES = 5
ONE_ABSENT = [(31, 24), (59, 28)]
ONE_ABSENT_KMERS = 2 * 2048 + 777  # three chunks of 2048 k-mers (CHUNK_KMERS, Consts "chunk_size")
ONE_ABSENT_AT = (0, ONE_ABSENT_KMERS - 1, 2047, 2048, None)

_cache = {}


def shape(spec, **kw):
    """craft(*spec), computed once per process and left unchanged by its users."""
    key = (spec[:3], tuple(spec[3]), spec[4:], tuple(sorted(kw)))
    if key not in _cache:
        _cache[key] = craft(*spec, **kw)
    return _cache[key]
