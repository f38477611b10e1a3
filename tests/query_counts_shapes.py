"""Crafted batches for the per-sequence query tallies (k_chunk_tally, k_seq_tally, k_seq_tally_long) and a numpy model of the
two-level tally. Pure CPU: `oracle.Oracle` for words and membership, numpy for the rest.

The device sums flags in two levels. The flags of a batch lie sequence after sequence, each in get_seq_words order; chunk c owns
the flags [kmer_off[c], kmer_off[c + 1]) and sequence s the chunks [seq_chunk[s], seq_chunk[s + 1]). `chunk_tables` restates
both tables on the host: a sequence of L bases has ceil((L - K + 1) / 2048) chunks, chunk j covers the bases
[2048 j, min(2048 j + 2048 + K - 1, L)), and it yields 1 + (valid bytes behind its first K) k-mers — get_seq_words makes one word
from the first K bytes whatever they are and one more per valid byte that follows (src/cbl.rs:277-287 of the reference), so a
chunk inside a run of N, and a sequence of N alone, still hold one k-mer each. `tally_model` then sums flags -> chunks ->
sequences. tests/test_query_counts_model.py holds the model against a direct per-sequence count from the oracle.

`batch(k)` strings together every length and edge the kernels tell apart; `NAMES` says which sequence is which.
"""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np

from oracle import Oracle

CHUNK_KMERS = 2048   # common.hpp CHUNK_KMERS (src/cbl.rs:67)
LANE_MAX = 8         # kernels_kmer.hpp SEQ_TALLY_LANE_MAX: most chunks of a sequence that one lane sums; longer ones go to a workgroup
LONG_THREADS = 256   # kernels_kmer.hpp SEQ_TALLY_LONG_THREADS
N_READS = 300        # reads of K + 9 bases: segment edges at every position relative to a wave (64) and a workgroup (256)

Batch = namedtuple("Batch", "k bases offsets names seqs")  # bases uint8, offsets uint64[n + 1], names[n], seqs[n] (bytes)
Expect = namedtuple("Expect", "total positive flags")      # per sequence uint32 / uint32, per k-mer bool (batch order)

_VALID = np.zeros(256, dtype=bool)
_VALID[list(b"ACGTacgt")] = True


def short_read_len(k):
    """Reads of 40 bases around the long sequence; K + 9 where 40 bases hold no k-mer (K > 40)."""
    return 40 if k <= 40 else k + 9


def _rand(rng, n):
    return bytearray(rng.choice(b"ACGT") for _ in range(n))


def batch(k, seed=7):
    """The named sequences, in this order (name -> what it is there for):
    len-K, len-K+1                      one and two k-mers
    one-chunk, chunk+1, three-chunks+5  2048 + K - 1, 2048 + K (a second chunk of one k-mer) and 3 * 2048 + K + 5 bases
    lane-max, lane-max+1                exactly LANE_MAX chunks (one lane) and LANE_MAX chunks + one k-mer (the workgroup route)
    short-a, long-35-chunks, short-b    70 000 bases (35 chunks) between two short reads
    read-0 .. read-299                  N_READS reads of K + 9 bases (ten k-mers each), with `parity` (one k-mer) in their middle
    N-first, N-last, N-mid, lower-first, lower-last, lower-mid   one such byte in a sequence of a chunk and a half
    N-run                               a run of N longer than a chunk inside a sequence of four chunks and more
    all-N                               K + 20 bytes of N
    tail-read                           a last clean read, so that the batch does not end on a special case"""
    rng = random.Random(seed * 1000 + k)
    C = CHUNK_KMERS
    named = [("len-K", _rand(rng, k)), ("len-K+1", _rand(rng, k + 1)), ("one-chunk", _rand(rng, C + k - 1)), ("chunk+1", _rand(rng, C + k)),
             ("three-chunks+5", _rand(rng, 3 * C + k + 5)), ("lane-max", _rand(rng, LANE_MAX * C + k - 1)), ("lane-max+1", _rand(rng, LANE_MAX * C + k)),
             ("short-a", _rand(rng, short_read_len(k))), ("long-35-chunks", _rand(rng, 70_000)), ("short-b", _rand(rng, short_read_len(k)))]
    named += [("read-%d" % i, _rand(rng, k + 9)) for i in range(N_READS // 2)]
    named.append(("parity", _rand(rng, k)))  # one k-mer: the flag segments of the reads behind it start at the odd offsets
    named += [("read-%d" % i, _rand(rng, k + 9)) for i in range(N_READS // 2, N_READS)]
    half = C + C // 2 + k
    for name, at, how in (("N-first", 0, "N"), ("N-last", half - 1, "N"), ("N-mid", C // 2 + 7, "N"), ("lower-first", 0, "lower"),
                          ("lower-last", half - 1, "lower"), ("lower-mid", C // 2 + 7, "lower")):
        s = _rand(rng, half)
        s[at] = ord("N") if how == "N" else s[at] | 0x20
        named.append((name, s))
    s = _rand(rng, 4 * C + k + 300)
    s[1500: 2 * C + k + 600] = b"N" * (2 * C + k + 600 - 1500)  # covers chunk 1 = bases [2048, 4096 + K - 1) and more
    named.append(("N-run", s))
    named.append(("all-N", bytearray(b"N" * (k + 20))))
    named.append(("tail-read", _rand(rng, k + 9)))
    seqs = [bytes(s) for _, s in named]
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return Batch(k, np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offsets, [n for n, _ in named], seqs)


def chunk_tables(bases, offsets, k):
    """(seq_chunk[n + 1], kmer_off[nchunks + 1]) as plan_chunks leaves them (int64), with chunk k-mer counts that honour invalid bytes."""
    valid = _VALID[np.asarray(bases, dtype=np.uint8)]
    seq_chunk, nk = [0], []
    for a, b in zip(offsets[:-1].tolist(), offsets[1:].tolist()):
        L = b - a
        assert L >= k
        for start in range(0, L - k + 1, CHUNK_KMERS):
            end = min(start + CHUNK_KMERS + k - 1, L)
            nk.append(1 + int(valid[a + start + k: a + end].sum()))
        seq_chunk.append(len(nk))
    kmer_off = np.zeros(len(nk) + 1, dtype=np.int64)
    kmer_off[1:] = np.cumsum(nk)
    return np.array(seq_chunk, dtype=np.int64), kmer_off


def tally_model(flags, kmer_off, seq_chunk):
    """flags -> per-chunk sums over kmer_off -> per-sequence sums over seq_chunk: (total, positive, chunk_pos)."""
    flags = np.asarray(flags).astype(np.int64)
    assert len(flags) == kmer_off[-1]
    run = np.concatenate([[0], np.cumsum(flags)])
    chunk_pos = run[kmer_off[1:]] - run[kmer_off[:-1]]                       # k_chunk_tally
    crun = np.concatenate([[0], np.cumsum(chunk_pos)])
    positive = crun[seq_chunk[1:]] - crun[seq_chunk[:-1]]                    # k_seq_tally / k_seq_tally_long
    total = kmer_off[seq_chunk[1:]] - kmer_off[seq_chunk[:-1]]
    return total.astype(np.uint32), positive.astype(np.uint32), chunk_pos


def direct_counts(o: Oracle, seqs):
    """Per sequence, straight from the oracle: Oracle.seq_words, then contains_word per word."""
    total, positive, flags = [], [], []
    for s in seqs:
        f = [o.contains_word(w) for w in o.seq_words(s)]
        total.append(len(f))
        positive.append(sum(f))
        flags += f
    return Expect(np.array(total, dtype=np.uint32), np.array(positive, dtype=np.uint32), np.array(flags, dtype=bool))


def index_reads(k, n=200, length=150, seed=99):
    """Random reads that go into the index next to every second sequence of the batch (they match nothing of it)."""
    rng = random.Random(seed + k)
    return [bytes(_rand(rng, max(length, k + 9))) for _ in range(n)]


def resident_seqs(b: Batch):
    """What the index of the tests is built from: every second sequence of the batch, then random reads."""
    return b.seqs[::2] + index_reads(b.k)


def as_arrays(seqs):
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return np.frombuffer(b"".join(seqs), dtype=np.uint8).copy(), offsets


_cache = {}


def case(k, pb, canonical=False):
    """(batch, oracle holding resident_seqs, Expect of the batch against it), computed once per process and left unchanged."""
    key = (k, pb, canonical)
    if key not in _cache:
        b = batch(k)
        o = Oracle(k, pb, canonical)
        o.insert_seqs(*as_arrays(resident_seqs(b)))
        _cache[key] = (b, o, direct_counts(o, b.seqs))
    return _cache[key]


CONFIGS = [(31, 24, False), (31, 24, True), (59, 28, False), (11, 8, False)]  # K = 59 / PB = 28: wide words, k_contains at any size
