"""De Bruijn neighbourhoods on the CPU: the definitions of DESIGN.md section 6j on Python ints and on ACTG strings, the neighbour mask of a k-mer against
an `oracle.Oracle` (eight `contains_kmer` calls: the oracle canonicalises as the reference does), the degree table of a list of masks, and the crafted
graphs the GPU tests insert. Pure CPU; no expectation comes from the GPU path.

Base codes are the reference's (src/kmer.rs:11-27): A 0, C 1, T 2, G 3; a packed k-mer holds its first base in the most significant two bits."""
from __future__ import annotations

import random

import numpy as np

NUCS = "ACTG"
CODE = {c: i for i, c in enumerate(NUCS)}
COMPLEMENT = {"A": "T", "T": "A", "C": "G", "G": "C"}

# (K, PREFIX_BITS, canonical): one per word class of tests/query_shapes.py, plus the benchmark's
CONFIGS = [(15, 6, False), (15, 6, True), (31, 24, False), (31, 24, True), (31, 4, False),  # (31, 4): SUFFIX_BITS = 64
           (31, 3, False),                                                                  # wide suffix: never joins
           (33, 16, False), (33, 16, True),                                                 # the prepend shift is exactly 64
           (45, 6, False),                                                                  # a word of more than 96 bits: never joins
           (59, 28, True)]


# ---- the definitions, on ints ----------------------------------------------------------------------------------------------------------------
def append(x: int, c: int, k: int) -> int:
    return ((x << 2) | c) & ((1 << (2 * k)) - 1)


def prepend(x: int, c: int, k: int) -> int:
    return (x >> 2) | (c << (2 * (k - 1)))


def neighbors(x: int, k: int):
    """The eight neighbours in mask-bit order."""
    return [append(x, c, k) for c in range(4)] + [prepend(x, c, k) for c in range(4)]


# ---- the same on strings ---------------------------------------------------------------------------------------------------------------------
def pack(s: str) -> int:
    x = 0
    for ch in s:
        x = (x << 2) | CODE[ch]
    return x


def unpack(x: int, k: int) -> str:
    return "".join(NUCS[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def neighbors_str(s: str):
    return [s[1:] + c for c in NUCS] + [c + s[:-1] for c in NUCS]


def revcomp_str(s: str) -> str:
    return "".join(COMPLEMENT[ch] for ch in reversed(s))


def canonical_str(s: str) -> str:
    """Kmer::canonical (src/kmer.rs:94-106): a k-mer whose packed form has an even number of set bits is kept, any other is reverse-complemented
    (K is odd, so exactly one of a k-mer and its reverse complement is kept)."""
    return s if bin(pack(s)).count("1") % 2 == 0 else revcomp_str(s)


def mask_str(held: set, s: str, canonical: bool) -> int:
    """The neighbour mask of k-mer `s` against a Python set of k-mer strings (of canonical forms where `canonical`)."""
    m = 0
    for j, y in enumerate(neighbors_str(s)):
        if (canonical_str(y) if canonical else y) in held:
            m |= 1 << j
    return m


# ---- against the oracle ----------------------------------------------------------------------------------------------------------------------
def mask_model(oracle, x: int, k: int) -> int:
    m = 0
    for j, y in enumerate(neighbors(x, k)):
        if oracle.contains_kmer(y):
            m |= 1 << j
    return m


def masks_model(oracle, kmers, k: int):
    memo = {}
    out = np.empty(len(kmers), dtype=np.uint8)
    for i, x in enumerate(kmers):
        if x not in memo:
            memo[x] = mask_model(oracle, x, k)
        out[i] = memo[x]
    return out


def table_model(masks):
    t = np.zeros((5, 5), dtype=np.uint64)
    for m in np.asarray(masks, dtype=np.uint8).tolist():
        t[bin(m & 15).count("1"), bin(m >> 4).count("1")] += 1
    return t


def oracle_kmers(oracle):
    """The k-mers of the oracle's set in iteration order (CBL::iter)."""
    return [oracle.kmer_of_word(w) for w in oracle.iter_words()]


# ---- crafted graphs --------------------------------------------------------------------------------------------------------------------------
def _rand(rng, n):
    return "".join(rng.choice(NUCS) for _ in range(n))


def _primitive(s):
    return all(s[i:] + s[:i] != s for i in range(1, len(s)))


class Graph:
    """Two batches of reads for one K, and the k-mers the tests look at by name."""

    def __init__(self, k: int, seed: int = 11):
        rng = random.Random(seed * 1000 + k)
        self.k = k
        main = _rand(rng, 3000)
        reads = [main, _rand(rng, k), _rand(rng, k + 1), _rand(rng, k + 6)]  # mostly simple-path nodes; the ends are sources and sinks
        # a 4-way fork behind k-mer P and a 4-way join in front of k-mer Q
        self.fork, self.join = _rand(rng, k), _rand(rng, k)
        reads += [self.fork + c + _rand(rng, 5) for c in NUCS]
        reads += [_rand(rng, 5) + c + self.join for c in NUCS]
        # the four homopolymers: a self-loop in both nibbles (poly-A is k-mer 0, poly-G the all-ones k-mer)
        reads += [c * (k + 3) for c in NUCS]
        # a rotation ring: the K rotations of a primitive s share one necklace at K positions; each is the next one's predecessor
        s = _rand(rng, k)
        while not _primitive(s):
            s = _rand(rng, k)
        self.ring = s
        reads.append(s + s)
        # the dinucleotide repeat ACAC...A and its partner CACA...C: a 2-cycle on a periodic necklace
        self.dinuc = ("AC" * k)[:k]
        self.dinuc_partner = ("CA" * k)[:k]
        reads.append(("AC" * k)[: k + 1])
        self.batch1 = [r.encode() for r in reads]
        # a second batch: new reads and pieces that overlap the first, so that Vec buckets take words behind the ones they hold
        self.batch2 = [_rand(rng, 400).encode(),(main[700:760] + _rand(rng, 40)).encode(), (_rand(rng, 30) + main[1500:1580]).encode()]
        self.late = (main[100:130] + _rand(rng, 2 * k)).encode()  # one more read, for the insert_seq that is not flushed

    @staticmethod
    def arrays(reads):
        bases = np.frombuffer(b"".join(reads), dtype=np.uint8).copy()
        offsets = np.zeros(len(reads) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum([len(r) for r in reads])
        return bases, offsets


def queries(graph: Graph, oracle, canonical: bool, seed: int = 3):
    """The query list of the GPU tests: the named k-mers, absent ones and duplicates up front (the prefixes of the list are tested at the lane-group,
    wave and workgroup edges), then every resident k-mer, each of the first residents with one base changed, and — canonical — reverse complements of
    resident k-mers: the orientation that is not stored."""
    k = graph.k
    rng = random.Random(seed)
    res = oracle_kmers(oracle)
    named = [pack(s) for s in (graph.fork, graph.join, graph.ring, graph.dinuc, graph.dinuc_partner)] + [pack(c * k) for c in NUCS]
    absent = [rng.getrandbits(2 * k) for _ in range(60)]
    sample = rng.sample(res, min(120, len(res)))
    changed = [x ^ (rng.randrange(1, 4) << (2 * rng.randrange(k))) for x in sample[:60]]
    rcs = [pack(revcomp_str(unpack(x, k))) for x in sample[:60]] if canonical else []
    head = []
    for group in zip(named * 7, absent, sample, changed, (rcs or sample[60:])):
        head += list(group)
    head += head[:20]  # duplicates
    assert len(head) >= 257
    return head + res + changed + rcs
