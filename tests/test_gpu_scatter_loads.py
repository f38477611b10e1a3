"""The record loads of k_radix_scatter's generic arm (cbl_amd/csrc/kernels_radix.hpp): every load of a tile is issued before the first digit is
computed, the digits come from a loop of their own. The slots behind a ragged tile's last record re-read slot 0, take digit 255 and must never be
written back: every case puts a tile of n_tile = 1, 63 | 64 | 65, 511 | 512 | 513 or 4095 | 4096 records (alone, and behind a full tile) at the end of
a pass that runs one of the instantiations with that arm, and compares the index bytes with the CPU oracle's, byte for byte.

Which pass ends in that tile:
  * One sequence of N + K - 1 random bases gives N k-mers: pass A's last tile holds N % 4096 records. Pass A runs the generic arm for every word
    without a one-byte hi part: K = 29 (<NoHi, NoHi>), K = 33 and K = 59 (<u64, u64>); at K = 31 the sequences cover the routes behind it
    (PREFIX_BITS = 28 by the prefix split and by FINE bins, canonical, a second insert, reads with N).
  * The LSD passes tile every pass-A segment on its own, the last of them every (segment, low digit) group: crafted words (insert_words_device,
    the oracle's insert_batch on the same words) put n records into one segment with random low digits (pass B ends that segment in a tile of
    n % 4096), n records into one group of another segment (pass C ends that group in one) and pad the batch so that pass A's last tile holds
    n % 4096 too. K = 31 at PREFIX_BITS = 24 and 16 (<NoHi, NoHi> in passes B and C), K = 21 (<NoHi, NoHi> from pass A on), K = 33 (<u64, u64>).
  * partition_words_device (DigitDest, one pass over plain tiles) on the same crafted words against numpy's stable partition.
  * DigitBin: the plain receiver of the "bins" protocol, two ranks sharing this GPU over the callback transport, each rank a thread of this process
    with a gloo group of its own (tests/rank_threads.py), K = 21: the senders' first pass is <NoHi, NoHi, DigitBin, REDIR>.
  * k_prefix_split (PREFIX_BITS = 28 with the FINE bins off) and k_boundaries (PREFIX_BITS <= 8) load their records the same way and are covered
    by the same comparison."""
import random
import socket
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

import rank_threads  # noqa: E402  (tests/)

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
M64 = (1 << 64) - 1
TILE = 4096
TAILS = (1, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097)      # a ragged tile alone (4097: a full tile and one record)
SIZES = TAILS + (TILE + 63, TILE + 513, 2 * TILE - 1)          # ... and behind a full tile
CRAFTED = ((31, 24), (31, 16), (21, 24), (33, 24))


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _layout(k, pb):
    """(suffix bits, hi bytes) of the K-mer word: 2K bits of necklace + the rotation"""
    kb = 2 * k
    wb = kb + (kb - 1).bit_length()
    return wb - pb, (0 if wb <= 64 else (1 if kb <= 64 else 8))


def _sequence(seed, n_kmers, k):
    rng = np.random.default_rng(seed)
    bases = rng.choice(ACGT, size=n_kmers + k - 1).astype(np.uint8)
    return bases, np.array([0, bases.size], dtype=np.uint64)


def _same_index(k, pb, inserts, canonical=False):
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    try:
        assert g.consts()["hi_bytes"] == _layout(k, pb)[1]
        o = Oracle(k, pb, canonical)
        for bases, offsets in inserts:
            g.insert_seqs(bases, offsets)
            o.insert_seqs(bases, offsets)
            assert g.count() == o.count()
            assert g.serialize() == o.serialize(), "serialized index differs from the oracle"
    finally:
        g.close()


# ---- pass A ends in the ragged tile: sequences -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k,pb", [(29, 24), (33, 24), (59, 28)])
def test_pass_a_tail_tile(k, pb, n):
    _need_gpu()
    _same_index(k, pb, [_sequence(100 * k + n, n, k)])


@pytest.mark.parametrize("n", (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4097))
@pytest.mark.parametrize("k,pb", [(29, 8), (21, 5), (33, 8), (59, 8)])
def test_no_lsd_pass_directory_from_the_sorted_records(k, pb, n):
    """PREFIX_BITS <= 8: pass A alone, the bucket starts come from k_boundaries, four records per thread (its loads are grouped the same way):
    n either side of a thread's four records, of a wave's 256 and of a workgroup's 1024."""
    _need_gpu()
    _same_index(k, pb, [_sequence(11 * k + n, n, k)])


@pytest.mark.parametrize("n", (1, 65, 513, 4095, 4097, TILE + 513))
@pytest.mark.parametrize("fine", ("1", "0"))
@pytest.mark.parametrize("k", (31, 21))
def test_prefix_bits_28_by_fine_bins_and_by_the_prefix_split(k, fine, n, monkeypatch):
    _need_gpu()
    monkeypatch.setenv("CBLX_FINE_MIN", "0")
    monkeypatch.setenv("CBLX_FINE_BINS", fine)
    g = cbl_amd.CBL(k, 28)
    try:
        bases, offsets = _sequence(7 * n + k, n, k)
        o = Oracle(k, 28, False)
        g.insert_seqs(bases, offsets)
        g.flush()
        o.insert_seqs(bases, offsets)
        if fine == "0" or n >= TILE - 1:
            assert g.fine_builds() == (1 if fine == "1" else 0)
        assert g.serialize() == o.serialize(), "serialized index differs from the oracle"
    finally:
        g.close()


@pytest.mark.parametrize("k,pb", [(31, 24), (29, 24), (33, 24), (59, 28)])
def test_second_insert_into_a_non_empty_index(k, pb):
    _need_gpu()
    _same_index(k, pb, [_sequence(k, 3 * TILE + 513, k), _sequence(k + 1, TILE + 65, k), _sequence(k, 3 * TILE + 513, k)])


@pytest.mark.parametrize("k,pb", [(31, 24), (21, 16), (33, 24), (59, 28)])
def test_canonical(k, pb):
    _need_gpu()
    _same_index(k, pb, [_sequence(3 * k, 2 * TILE + 511, k)], canonical=True)


@pytest.mark.parametrize("k,pb,L", [(31, 24, 150), (29, 24, 150), (59, 28, 250)])
def test_reads_with_n(k, pb, L):
    """A few thousand reads, every 50th with an N at a position of its own: the k-mer stream is cut into pieces of odd lengths."""
    _need_gpu()
    n_reads = 2000
    rng = np.random.default_rng(41 + k)
    bases = rng.choice(ACGT, size=n_reads * L).astype(np.uint8)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)
    for r in range(0, n_reads, 50):
        bases[r * L + 4 + r // 50] = ord("N")
    _same_index(k, pb, [(bases, offsets)])


# ---- the LSD passes end a segment / a group in the ragged tile: crafted words ----------------------------------------------------------------------
class _Crafted:
    """One batch of words for (k, pb, n), on the device and as Python integers, and the oracle's bytes for it: computed once per case, left unchanged."""

    def __init__(self, k, pb, n):
        sb, hb = _layout(k, pb)
        rng = random.Random("scatter loads %d/%d/%d" % (k, pb, n))
        low_bits = pb - 8                                    # prefix bits behind pass A's digit
        seg_x, seg_y, seg_z = rng.sample(range(256), 3)      # (K = 31: the top four prefix bits lie in the hi byte)
        pad = (-n) % TILE                                    # pass A: 2n + pad records, the last tile holds n % 4096 (or is full)
        prefix = [(seg_x << low_bits) | rng.getrandbits(low_bits) for _ in range(n)]
        if low_bits > 8:   # two LSD passes: one (segment, low digit) group of n records with random middle digits
            c = rng.choice((0, 1, 128, 254, 255))
            prefix += [(seg_y << low_bits) | (rng.getrandbits(low_bits - 8) << 8) | c for _ in range(n)]
        else:
            prefix += [(seg_y << low_bits) | rng.getrandbits(low_bits) for _ in range(n)]
        prefix += [(seg_z << low_bits) | rng.getrandbits(low_bits) for _ in range(pad)]
        rng.shuffle(prefix)
        self.k, self.pb, self.sb, self.hb = k, pb, sb, hb
        self.words = [(p << sb) | rng.getrandbits(sb) for p in prefix]
        self.prefix = np.array(prefix, dtype=np.uint64)
        self.n = len(self.words)
        assert self.n % TILE == n % TILE
        self.lo_np = np.array([w & M64 for w in self.words], dtype=np.uint64)
        self.lo = torch.from_numpy(self.lo_np.view(np.int64)).cuda()
        self.hi_np, self.hi = None, None
        if hb:
            a = np.array([w >> 64 for w in self.words], dtype=np.uint64)
            self.hi_np = a.astype(np.uint8) if hb == 1 else a.view(np.int64)
            self.hi = torch.from_numpy(self.hi_np).cuda()
        o = Oracle(k, pb, False)
        o.insert_words(self.words)
        self.count, self.blob = o.count(), o.serialize()


_crafted = {}


def crafted(k, pb, n):
    if (k, pb, n) not in _crafted:
        _crafted[(k, pb, n)] = _Crafted(k, pb, n)
    return _crafted[(k, pb, n)]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k,pb", CRAFTED)
def test_insert_words_device_at_segment_and_group_tails(k, pb, n):
    _need_gpu()
    w = crafted(k, pb, n)
    g = cbl_amd.CBL(k, pb)
    try:
        assert g.consts()["suffix_bits"] == w.sb and g.consts()["hi_bytes"] == w.hb
        g.insert_words_device(w.lo, w.hi, w.n)
        assert g.count() == w.count
        assert g.serialize() == w.blob, "serialized index differs from the oracle"
        g.insert_words_device(w.lo, w.hi, w.n)  # the same batch into the index it left: nothing changes
        assert g.serialize() == w.blob, "the same batch again: serialized index differs from the oracle"
    finally:
        g.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("k,pb", [(21, 24), (33, 24)])
def test_partition_words_device_at_tile_tails(k, pb, n):
    """Three destinations cut at the terciles of the data; the reference is numpy's stable partition by destination = #{bounds <= prefix}."""
    _need_gpu()
    w = crafted(k, pb, n)
    ranked = np.sort(w.prefix)
    bounds = np.array([ranked[w.n // 3], ranked[2 * w.n // 3]], dtype=np.uint32)
    dest = np.searchsorted(bounds.astype(np.uint64), w.prefix, side="right")
    order = np.argsort(dest, kind="stable")
    out_lo = torch.zeros_like(w.lo)
    out_hi = None if w.hi is None else torch.zeros_like(w.hi)
    g = cbl_amd.CBL(k, pb)
    try:
        counts = g.partition_words_device(w.lo, w.hi, w.n, bounds, 3, out_lo, out_hi)
    finally:
        g.close()
    assert counts == np.bincount(dest, minlength=3).tolist()
    assert np.array_equal(out_lo.cpu().numpy().view(np.uint64), w.lo_np[order])
    assert w.hi is None or np.array_equal(out_hi.cpu().numpy(), w.hi_np[order])


# ---- DigitBin: the senders' first pass of the "bins" protocol, plain receiver, callback transport ----------------------------------------------------
def _bins_rank(rank, world, port, k, pb, shards, out, errors):
    from cbl_amd import sharded

    try:
        torch.cuda.set_device(0)
        dist = rank_threads.group(rank, world, port, True)
        comm = cbl_amd.Comm.over_group(dist, rank, world, 0)  # host callbacks: the ranks share this GPU
        comm.set_recv_groups(1)  # the ungrouped receiver: bins refined by the destination rank (DigitBin)
        g = cbl_amd.CBL(k, pb, device=0)
        sb = sharded.ShardedBuilder(g, dist, slices=1, comm=comm, protocol="bins")
        bases, offsets = shards[rank]
        d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, np.uint8)])).cuda()
        d_o = torch.from_numpy(offsets.astype(np.int64)).cuda()
        sb.insert_seqs_device(d_b, d_o, len(offsets) - 1)
        used = comm.groups_used()
        blob = sharded.gather_serialized(g.serialize(), dist)
        if rank == 0:
            out.append((blob, used))
        comm.close()
        g.close()
    except BaseException as e:  # noqa: BLE001 - reported by the test
        errors.append(e)


def test_bins_protocol_over_callbacks_with_ragged_shards():
    """Rank 0 holds TILE + 513 k-mers, rank 1 4095: each sender's pass A ends in a ragged tile. One slice, so the job's order is rank order."""
    _need_gpu()
    k, pb, world = 21, 24, 2
    shards = [_sequence(5, TILE + 513, k), _sequence(6, TILE - 1, k)]
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    out, errors = [], []
    threads = [threading.Thread(target=_bins_rank, args=(r, world, port, k, pb, shards, out, errors), daemon=True) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    assert all(not t.is_alive() for t in threads) and len(out) == 1
    blob, used = out[0]
    assert used == 0  # the plain receiver, not the grouped one
    o = Oracle(k, pb, False)
    for bases, offsets in shards:
        o.insert_seqs(bases, offsets)
    assert blob == o.serialize()
