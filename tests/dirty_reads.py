"""Deterministic dirt for the synthetic read stream (cbl_amd/synth.py): lower case, N, IUPAC and other skipped bytes.

Every change is a function of the byte's GLOBAL stream position p (and of the seed, the read length L, K, and the cut and
all-N lists, which are global too), never of where a slice starts. So a rank dirties its own slice on the device (torch,
`dirty_torch`) and the test dirties the same range on the host for the oracle (numpy, `dirty_np`), and both get the same
bytes. The reference keeps A C G T a c g t and skips every other byte (/root/reference/src/kmer.rs:13-24).

Classes, in the order they are applied (a later class overwrites an earlier one):
- per base, from splitmix64(seed ^ _S_BASE, p): lower case (2 %), `N` (0.3 %), one of `_OTHER` (0.3 %);
- runs of `N`, 1 .. 3 K long: block j = p >> 6 of the stream holds a run with probability 6 / 256, starting inside the block;
- per read r = p // L, from splitmix64(seed ^ _S_READ, r): the read is all `N` (3 / 256), the read keeps only its first
  1 .. K - 1 bases (3 / 256: fewer than K valid bases), one skipped byte among its first K bytes (8 / 256);
- `cuts` (global base positions, e.g. the slice cuts): bytes c-2 and c+1 in lower case, c-1 `N`, c `n`;
- `all_n` (global [a, b) ranges): every byte `N` (a rank's whole batch: it has reads but no k-mer).

Only ACGT input is expected (what synth produces); the dirt keeps invalid bytes invalid whatever the order.
"""
from __future__ import annotations

import numpy as np

from cbl_amd import synth

_S_BASE, _S_RUN, _S_READ = 0x5D1B7A3C9E2F4860, 0x1C6E2B9D7F3A5048, 0x6A09E667F3BCC908
LOWER_PER_64K, N_PER_64K, OTHER_PER_64K = 1311, 197, 197  # 2.0 %, 0.3 %, 0.3 % of the bases
RUN_PER_256_BLOCKS = 6
READ_ALL_N, READ_SHORT, READ_HEAD = 3, 3, 8  # per 256 reads
_OTHER = b"nRY-*.\xe9\xff\xc1\xd4"  # (0xC1 / 0xD4: 'A' / 'T' with bit 7 set)


def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


class _Np:
    @staticmethod
    def mix(seed, j):
        return synth.splitmix64_at(seed & ((1 << 64) - 1), j.astype(np.uint64)).view(np.int64)

    where = staticmethod(np.where)

    @staticmethod
    def lut(b, like):
        return np.frombuffer(b, dtype=np.uint8)

    @staticmethod
    def zeros_bool(like):
        return np.zeros(like.shape, dtype=bool)


class _Torch:
    @staticmethod
    def mix(seed, j):  # synth.reads_torch's splitmix64 on int64 (wrapping)
        def lsr(z, s):
            return (z >> s) & ((1 << (64 - s)) - 1)

        z = (j + 1) * _s64(0x9E3779B97F4A7C15) + _s64(seed)
        z = (z ^ lsr(z, 30)) * _s64(0xBF58476D1CE4E5B9)
        z = (z ^ lsr(z, 27)) * _s64(0x94D049BB133111EB)
        return z ^ lsr(z, 31)

    @staticmethod
    def where(c, a, b):
        import torch

        return torch.where(c, a, b)

    @staticmethod
    def lut(b, like):
        import torch

        return torch.tensor(list(b), dtype=torch.uint8, device=like.device)

    @staticmethod
    def zeros_bool(like):
        import torch

        return torch.zeros(like.shape, dtype=torch.bool, device=like.device)


def classes(xp, p, seed, L, k):
    """Boolean masks of the per-position classes at the int64 positions p, and the replacement byte of each position for the
    classes that write a skipped byte. Used by `dirty_*`; the rates test reads it directly."""
    hp = xp.mix(seed ^ _S_BASE, p)
    u = hp & 0xFFFF
    lower = u < LOWER_PER_64K
    n1 = (u >= LOWER_PER_64K) & (u < LOWER_PER_64K + N_PER_64K)
    other = (u >= LOWER_PER_64K + N_PER_64K) & (u < LOWER_PER_64K + N_PER_64K + OTHER_PER_64K)
    other_byte = xp.lut(_OTHER, p)[((hp >> 16) & 0xFFFF) % len(_OTHER)]
    run = xp.zeros_bool(p)
    blk = p >> 6
    for d in range((63 + 3 * k) // 64 + 1):  # the blocks whose run can reach p
        jj = blk - d
        ok = jj >= 0
        jj = xp.where(ok, jj, 0 * jj)
        hb = xp.mix(seed ^ _S_RUN, jj)
        s = jj * 64 + ((hb >> 8) & 63)
        ln = 1 + ((hb >> 16) & 0xFFFF) % (3 * k)
        run = run | (ok & ((hb & 255) < RUN_PER_256_BLOCKS) & (p >= s) & (p < s + ln))
    r, o = p // L, p % L
    hr = xp.mix(seed ^ _S_READ, r)
    c = hr & 255
    all_n = c < READ_ALL_N
    short = (c >= READ_ALL_N) & (c < READ_ALL_N + READ_SHORT) & (o >= 1 + ((hr >> 8) & 0xFFFF) % (k - 1))
    head = (c >= READ_ALL_N + READ_SHORT) & (c < READ_ALL_N + READ_SHORT + READ_HEAD) & (o == ((hr >> 8) & 0xFFFF) % k)
    head_byte = xp.lut(b"N" + _OTHER, p)[((hr >> 24) & 0xFFFF) % (len(_OTHER) + 1)]
    return dict(lower=lower, n=n1, other=other, other_byte=other_byte, run=run, read_all_n=all_n, read_short=short, head=head,
                head_byte=head_byte)


def _apply(xp, b, p, seed, L, k, cuts, all_n):
    m = classes(xp, p, seed, L, k)
    N = ord("N")
    b = xp.where(m["lower"], b | 0x20, b)
    b = xp.where(m["n"], b * 0 + N, b)
    b = xp.where(m["other"], m["other_byte"], b)
    b = xp.where(m["run"] | m["read_all_n"] | m["read_short"], b * 0 + N, b)
    b = xp.where(m["head"], m["head_byte"], b)
    start, end = int(p[0]) if len(p) else 0, (int(p[-1]) + 1) if len(p) else 0
    for c in cuts:
        for q, how in ((c - 2, "lower"), (c - 1, "N"), (c, "n"), (c + 1, "lower")):
            if start <= q < end:
                i = q - start
                b[i] = (b[i] | 0x20) if how == "lower" else ord(how)
    for a, z in all_n:
        a, z = max(a, start), min(z, end)
        if z > a:
            b[a - start: z - start] = N
    return b


def dirty_np(bases, start, seed, L, k, cuts=(), all_n=()):
    """The bytes of stream positions [start, start + len(bases)), dirtied (a new uint8 array)."""
    bases = np.asarray(bases, dtype=np.uint8)
    p = np.arange(start, start + len(bases), dtype=np.int64)
    return np.ascontiguousarray(_apply(_Np, bases.copy(), p, seed, L, k, cuts, all_n), dtype=np.uint8)


def dirty_torch(bases, start, count, seed, L, k, cuts=(), all_n=()):
    """A copy of the uint8 tensor `bases` (CPU or GPU) whose first `count` bytes, stream positions [start, start + count), are
    dirtied; what follows them (reads_torch's 16-byte pad) is kept."""
    import torch

    out = bases.clone()
    if count:
        p = torch.arange(start, start + count, dtype=torch.int64, device=bases.device)
        out[:count] = _apply(_Torch, out[:count].clone(), p, seed, L, k, cuts, all_n)
    return out


def slice_cuts(per, L, slices, batches=None):
    """Global base positions of every rank's slice cuts (ShardedBuilder.slice_bounds) in a job whose batch `bt` gives rank r
    per[r][bt] reads, dealt in stream order batch-major, then rank-major (the multi-rank tests' layout)."""
    from cbl_amd.sharded import ShardedBuilder

    world = len(per)
    nb = len(per[0]) if batches is None else batches
    out = set()
    first = 0
    for bt in range(nb):
        for r in range(world):
            for a, b in ShardedBuilder.slice_bounds(per[r][bt], slices):
                out.update(((first + a) * L, (first + b) * L))
            first += per[r][bt]
    return sorted(out)


def write_dirty_fastx(path, seed, nrec, fastq=False, k=31):
    """A FASTA (or FASTQ) file of `nrec` dirty records, returned as the records' bases (what the reader hands on): lower case,
    IUPAC letters, `-` `*` `.`, runs of `N` up to 3 K, lines of 60 and of 10 000 bases, CRLF line ends on every third record.
    Record 1 is 9 000 bases with a 3 500-base `N` run in its middle (it crosses any cut of the file into 3 000-byte regions),
    record 2 is `N` only, record 3 has fewer than K valid bases. Every record is at least 64 bases long."""
    import random

    rng = random.Random(seed)
    recs = []
    with open(path, "wb") as f:
        for i in range(nrec):
            n = 9000 if i == 1 else rng.choice([64, 150, 151, 300, 777, 2500, 5000])
            s = bytearray(rng.choice(b"ACGT") for _ in range(n))
            for _ in range(n // 40):
                j = rng.randrange(n)
                what = rng.random()
                if what < 0.55:
                    s[j] |= 0x20
                elif what < 0.85:
                    s[j] = rng.choice(b"NnRYKMSWBDHVrykm-*.")
                else:
                    ln = rng.randint(1, 3 * k)
                    s[j: j + ln] = b"N" * len(s[j: j + ln])
            if i == 1:
                s[2500:6000] = b"N" * 3500
            elif i == 2:
                s[:] = b"N" * n
            elif i == 3:
                s[:] = bytes(rng.choice(b"ACGTacgt") for _ in range(k - 1)) + b"n" * (n - k + 1)
            s = bytes(s)
            recs.append(s)
            eol = b"\r\n" if i % 3 == 1 else b"\n"
            if fastq:
                f.write(b"@r%d" % i + eol + s + eol + b"+" + eol + b"I" * n + eol)
            else:
                f.write(b">r%d some text" % i + eol)
                w = rng.choice([60, 10_000])
                for a in range(0, n, w):
                    f.write(s[a: a + w] + eol)
    return recs


def cases(clean, dirty):
    """pytest parameters of a test that takes a trailing `dirty` flag: the clean cases keep the ids they had before the flag
    (pytest's own, the values joined by '-'), the dirty ones end in '-dirty'."""
    import pytest

    def ident(c):
        return "-".join(str(v) for v in c)

    return [pytest.param(*c, False, id=ident(c)) for c in clean] + [pytest.param(*c, True, id=ident(c) + "-dirty") for c in dirty]
