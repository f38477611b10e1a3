"""KRN-1 on its own after the necklace's bit operations were fused (cbl_amd/csrc/necklace.hpp: rotations without a ring mask of their
own under an AND, three-input instructions on gfx950) and the uniform-reads loop of k_encode began to carry its chunk products as
running sums: the words of seq_words_device against the CPU oracle's words for the same reads, bit for bit and in order, and the
index built from the same reads against the oracle's serialized bytes (of the 4 100-bp reads, all go through KRN-1 and the first 500
into the index).

Read sets of about 2 000 reads: random 150-bp reads; poly-A, poly-T, (AC)n, (ACGT)n; a K-mer (and a 31-mer) repeated, read at
one-base shifts; A-runs of 5, 6 and 7 bases among C / G / T (zero runs of 10 .. 15 bits: either side of the L = 11 step); reads with
an N and lower case (the dirty-chunk kernel); lengths mixed 40 .. 300 bp (the loop that reads the chunk tables); equal lengths of K,
K + 1, 31, 32 and 4 100 bp (the uniform loop with one and two k-mers per read, chunks that straddle a 4 KiB tile, one read longer than
a tile; 150 bp is the first set). K = 21, 31 and 59 have a loop of their own, K = 29 reads K from the parameter block."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

NREADS = 2000
PREFIX_BITS = 24
BUILD_BASES = 500 * 4100
KS = (21, 29, 31, 59)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _rand(rng, n, alphabet=b"ACGT"):
    return np.frombuffer(alphabet, dtype=np.uint8)[rng.integers(0, len(alphabet), size=n)].tobytes()


def _equal_length(L):
    def make(rng, k):
        return [_rand(rng, L) for _ in range(NREADS)]
    return make


def _low_complexity(rng, k):
    out = []
    for i in range(NREADS // 4):
        ph = i % 4
        out += [b"A" * 150, b"T" * 150, (b"AC" * 80)[ph % 2: ph % 2 + 150], (b"ACGT" * 40)[ph: ph + 150]]
    return out


def _shifted_repeats(rng, k):
    out = []
    periods = sorted({31, k})
    for period in periods:
        for _ in range(NREADS // 75 // len(periods) + 1):
            unit = _rand(rng, period)
            long = unit * (300 // period + 3)
            out += [long[s: s + 150] for s in range(75)]  # more shifts than the period: every rotation, some twice
    return out[:NREADS]


def _a_runs(rng, k):
    out = []
    for i in range(NREADS):
        r = bytearray(_rand(rng, 150, b"CGT"))
        for _ in range(1 + i % 3):
            n = 5 + int(rng.integers(3))
            p = int(rng.integers(0, 150 - n))
            r[p: p + n] = b"A" * n
        out.append(bytes(r))
    return out


def _dirty(rng, k):
    out = []
    for i in range(NREADS):
        r = bytearray(_rand(rng, 150))
        if i % 3 == 0:
            r[int(rng.integers(150))] = ord("N")
        if i % 3 == 1:
            a = int(rng.integers(140))
            r[a: a + 10] = bytes(r[a: a + 10]).lower()
        if i % 50 == 7:
            r[int(rng.integers(k))] = ord("n")  # inside the first K bytes of the chunk
        out.append(bytes(r))
    return out


def _mixed_lengths(rng, k):
    return [_rand(rng, int(rng.integers(max(40, k), 301))) for _ in range(NREADS)]


SETS = {"random150": _equal_length(150), "low_complexity": _low_complexity, "shifted_repeats": _shifted_repeats, "a_runs": _a_runs, "n_and_lower_case": _dirty,
        "mixed_lengths": _mixed_lengths, "len31": _equal_length(31), "len32": _equal_length(32), "len4100": _equal_length(4100)}


def _cases():
    out = []
    for k in KS:
        names = [n for n in SETS if not (n in ("len31", "len32") and int(n[3:]) < k)]
        for n in names:
            out.append((k, n))
        for L in (k, k + 1):  # one and two k-mers per read
            if "len%d" % L not in names:
                out.append((k, "len%d" % L))
    return out


def _reads(k, name):
    rng = np.random.default_rng(zlib.crc32(("%d %s" % (k, name)).encode()))
    make = SETS[name] if name in SETS else _equal_length(int(name[3:]))
    seqs = make(rng, k)
    assert all(len(s) >= k for s in seqs)
    bases = np.frombuffer(b"".join(seqs), dtype=np.uint8)
    offsets = np.zeros(len(seqs) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(s) for s in seqs])
    return seqs, bases, offsets


def _oracle_words(o, seqs):
    """The oracle's words of every read, in order, as (lo, hi) uint64 arrays (its C entry point fills them directly: the wrapper's
    seq_words makes a Python int of every word, which the 2 M k-mers of the long reads do not need)."""
    cap = sum(len(s) for s in seqs) + 1
    lo, hi = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    at = 0
    for s in seqs:
        n = o._L.oracle_seq_words(o._h, s, len(s), 0, lo[at:].ctypes.data, hi[at:].ctypes.data, cap - at)
        assert n >= 0
        at += n
    return lo[:at], hi[:at]


def _gpu_words(g, bases, offsets, nseq):
    nmax = int(len(bases))
    pad = (-len(bases)) % 16 + 16
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(pad, np.uint8)])).cuda()
    d_o = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_lo = torch.zeros(nmax + 1, dtype=torch.int64, device="cuda")
    hb = g.consts()["hi_bytes"]
    d_hi = None if hb == 0 else torch.zeros(nmax + 1, dtype=torch.uint8 if hb == 1 else torch.int64, device="cuda")
    n = g.seq_words_device(d_b, d_o, nseq, d_lo, d_hi, nmax)
    lo = d_lo[:n].cpu().numpy().view(np.uint64)
    hi = np.zeros(n, dtype=np.uint64) if d_hi is None else d_hi[:n].cpu().numpy().astype(np.uint64 if hb == 1 else np.int64).view(np.uint64)
    return lo, hi


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,name", _cases())
def test_encode_words_and_index_match_the_oracle(k, name, canonical):
    _need_gpu()
    seqs, bases, offsets = _reads(k, name)
    g = cbl_amd.CBL(k, PREFIX_BITS, canonical=canonical)
    o = Oracle(k, PREFIX_BITS, canonical)
    want_lo, want_hi = _oracle_words(o, seqs)
    lo, hi = _gpu_words(g, bases, offsets, len(seqs))
    assert len(lo) == len(want_lo)
    bad = np.flatnonzero((lo != want_lo) | (hi != want_hi))
    assert bad.size == 0, "%d of %d words differ, the first at k-mer %d: gpu %#x:%016x, oracle %#x:%016x" % (
        bad.size, len(lo), bad[0], hi[bad[0]], lo[bad[0]], want_hi[bad[0]], want_lo[bad[0]])
    if len(bases) > BUILD_BASES:  # the long reads: the index of the first 500 (the oracle takes 5 s for all of them)
        n = int(np.searchsorted(offsets, BUILD_BASES, side="right")) - 1
        bases, offsets = bases[: int(offsets[n])], offsets[: n + 1]
    g.insert_seqs(bases, offsets)
    o.insert_seqs(bases, offsets)
    assert g.count() == o.count()
    assert g.serialize() == o.serialize(), "serialized index differs from the oracle"
    g.close()
