"""A numpy model of the panel query's tallies (k_chunk_tally_mask, k_seq_tally_mask, k_seq_tally_long_mask) and the expectations of
tests/test_gpu_panel_query.py. Pure CPU: `oracle.Oracle` for the words of a sequence and of an index, numpy for the rest.

A panel query leaves one 64-bit membership mask per k-mer of the batch, bit j = index j holds it, in the order of the flags of
`contains_seqs` (tests/query_counts_shapes.py). The device reduces the masks in the two levels of the flag tallies, n counts at a time:

  chunk level   one wave per chunk takes 64 mask words per round, word l in lane l (the lanes past a short last round hold 0). For j < n the
                ballot of bit j over the 64 lanes is row j of the transposed 64 x 64 bit matrix; lane j adds its popcount. `chunk_tally_mask`
                restates that round by round: chunk_pos[c, j].
  sequence      one lane per (sequence, index) sums the chunks of a sequence of up to LANE_MAX chunks; a longer one is summed by a workgroup of
                LONG_THREADS lanes, lane t taking the chunks t, t + LONG_THREADS, ... `seq_tally_mask` restates both: positive[j, s].

`expect(oracles, seqs)` is the direct count the model is held against and the GPU tests expect: Oracle.seq_words per sequence, membership in
the Python set of each index's iter_words, then query_counts_shapes.tally_model per index.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import query_counts_shapes as qc

WAVE = 64
M64 = (1 << 64) - 1
FILL32 = 0xA5A5A5A5
FILL64 = 0xA5A5A5A5A5A5A5A5

Panel = namedtuple("Panel", "total positive mask flags")  # uint32[nseq], uint32[n, nseq], uint64[nk], bool[n, nk]


def masks_of(flags):
    """flags bool[n, nk] -> uint64[nk]: bit j of word i = flags[j, i]."""
    flags = np.asarray(flags, dtype=bool)
    mask = np.zeros(flags.shape[1], dtype=np.uint64)
    for j in range(flags.shape[0]):
        mask |= flags[j].astype(np.uint64) << np.uint64(j)
    return mask


def _popcount64(x):
    return bin(int(x)).count("1")


def chunk_tally_mask(mask, kmer_off, n):
    """chunk_pos int64[nchunks, n] by the ballot transpose: per round of 64 words, lane j takes bit j of every word."""
    mask = np.asarray(mask, dtype=np.uint64)
    lanes = np.arange(WAVE, dtype=np.uint64)
    out = np.zeros((len(kmer_off) - 1, n), dtype=np.int64)
    for c in range(len(kmer_off) - 1):
        a, cnt = int(kmer_off[c]), int(kmer_off[c + 1] - kmer_off[c])
        for i0 in range(0, cnt, WAVE):
            m = np.zeros(WAVE, dtype=np.uint64)
            m[: min(WAVE, cnt - i0)] = mask[a + i0: a + min(i0 + WAVE, cnt)]  # a short last round: the lanes past the end hold no bit
            if not m.any():
                continue
            for j in range(n):
                row = np.bitwise_or.reduce(((m >> np.uint64(j)) & np.uint64(1)) << lanes)  # the ballot of bit j: bit l = lane l's vote
                out[c, j] += _popcount64(row)                                               # lane j adds its popcount
    return out


def seq_tally_mask(chunk_pos, seq_chunk):
    """positive uint32[n, nseq] from chunk_pos[nchunks, n]: one lane per (sequence, index), a workgroup for a long sequence."""
    chunk_pos = np.asarray(chunk_pos, dtype=np.int64)
    n, nseq = chunk_pos.shape[1], len(seq_chunk) - 1
    out = np.zeros((n, nseq), dtype=np.uint32)
    for s in range(nseq):
        a, b = int(seq_chunk[s]), int(seq_chunk[s + 1])
        for j in range(n):
            if b - a <= qc.LANE_MAX:
                out[j, s] = sum(int(chunk_pos[ch, j]) for ch in range(a, b))
            else:  # lane t: chunks a + t, a + t + LONG_THREADS, ...; then the sum over the lanes
                out[j, s] = sum(int(chunk_pos[a + t: b: qc.LONG_THREADS, j].sum()) for t in range(qc.LONG_THREADS))
    return out


def tallies_from_masks(mask, kmer_off, seq_chunk, n):
    """(total uint32[nseq], positive uint32[n, nseq]) as the device reduces them."""
    total = (kmer_off[seq_chunk[1:]] - kmer_off[seq_chunk[:-1]]).astype(np.uint32)
    return total, seq_tally_mask(chunk_tally_mask(mask, kmer_off, n), seq_chunk)


def expect(oracles, seqs, words=None):
    """The panel of `oracles` (same K, PREFIX_BITS, canonical) asked about `seqs` (bytes each), from the CPU alone. `words`: the words of
    the batch in order when the caller has them already (Oracle.seq_words of every sequence, strung together)."""
    o = oracles[0]
    sets = [set(x.iter_words()) for x in oracles]
    if words is None:
        words = [w for s in seqs for w in o.seq_words(s)]
    flags = np.array([[w in st for w in words] for st in sets], dtype=bool).reshape(len(sets), len(words))
    bases, offsets = qc.as_arrays(seqs)
    seq_chunk, kmer_off = qc.chunk_tables(bases, offsets.astype(np.int64), o.k)
    assert int(kmer_off[-1]) == len(words)
    total, rows = None, []
    for j in range(len(sets)):
        total, pos, _ = qc.tally_model(flags[j], kmer_off, seq_chunk)
        rows.append(pos)
    return Panel(total, np.stack(rows).astype(np.uint32), masks_of(flags), flags)


def classify_model(total, positive, min_fraction=0.5, min_hits=0):
    """CBL.classify in plain Python: the index with the most hits among those passing the matching rule, ties to the lowest, else -1."""
    import math

    out = []
    for s, t in enumerate(np.asarray(total).tolist()):
        best, arg = -1, -1
        for j in range(len(positive)):
            p = int(positive[j][s])
            if t > 0 and p >= max(int(min_hits), math.ceil(min_fraction * t)) and p > best:
                best, arg = p, j
        out.append(arg)
    return np.array(out, dtype=np.int64)
