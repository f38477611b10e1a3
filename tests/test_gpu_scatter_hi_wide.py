"""The one-byte hi parts of 65..72-bit words, read by the partition kernels as one 8-byte word per lane and handed to their lanes through
LDS (cbl_amd/csrc/kernels_radix.hpp: tile_hi_fetch / tile_hi_spread). A wave takes that path when its 512 records lie wholly inside
the tile and its bytes start on an 8-byte boundary; every other wave reads bytes. The index must not depend on which path a wave took.

One sequence of N + K - 1 random bases gives exactly N k-mers, so pass A runs on ceil(N / 4096) tiles of which the last holds
N % 4096 records: N is taken either side of every wave edge (512 records) and tile edge, so that a full wave stands next to a partial
one, or a tile has neither. At N = 65 537 canonical k-mers, PREFIX_BITS 8 (pass A alone), 16 and 28 (the FINE route: bins from a
table), and a second insert into the non-empty index. The other word widths with a one-byte hi part would be K = 30 (66 bits) and
K = 32 (70 bits): K must be odd, here as in the reference (its build.rs), so neither index nor oracle exists for them and the test can
only hold the library to refusing them; K = 31 (68 bits) is the one K whose words have a one-byte hi part. Callers' arrays: the
words of seq_words_device with the hi bytes at every offset 1 .. 7 of an 8-byte boundary go through insert_words_device (no wave is
aligned: byte path everywhere, same index) and through partition_words_device (k_radix_hist and the scatter with a hi part on both
sides) against a numpy stable partition. Reads with N cut the stream into chunks of odd lengths.

Unless said otherwise the reference is the CPU oracle: serialized index bytes, byte for byte."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
EDGE_N = (1, 7, 8, 9, 511, 512, 513, 1023, 1024, 4095, 4096, 4097, 4096 + 511, 4096 + 512, 4096 + 513, 8 * 4096 + 1)
N_ROUTES = 65537
N_WORDS = 4096 * 3 + 517
OFFSETS = (1, 2, 3, 4, 5, 6, 7)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _sequence(seed, n_kmers, k):
    rng = np.random.default_rng(seed)
    bases = rng.choice(ACGT, size=n_kmers + k - 1).astype(np.uint8)
    return bases, np.array([0, bases.size], dtype=np.uint64)


def _same_index(k, pb, inserts, canonical=False):
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    assert g.consts()["hi_bytes"] == 1
    o = Oracle(k, pb, canonical)
    for bases, offsets in inserts:
        g.insert_seqs(bases, offsets)
        o.insert_seqs(bases, offsets)
        assert g.count() == o.count()
        assert g.serialize() == o.serialize(), "serialized index differs from the oracle"
    g.close()


@pytest.mark.parametrize("n", EDGE_N)
def test_wave_and_tile_edges(n):
    _need_gpu()
    _same_index(31, 24, [_sequence(2000 + n, n, 31)])


@pytest.mark.parametrize("k,pb,canonical", [(31, 24, True), (31, 8, False), (31, 16, False), (31, 28, False)])
def test_routes(k, pb, canonical):
    _need_gpu()
    _same_index(k, pb, [_sequence(7 * k + pb, N_ROUTES, k)], canonical)


@pytest.mark.parametrize("k", [30, 32])
def test_even_k_has_no_index(k):
    """66- and 70-bit words would take the same one-byte hi part, but no even K can be built (nor can the oracle's)."""
    _need_gpu()
    with pytest.raises(cbl_amd.CblxError, match="K must be odd"):
        cbl_amd.CBL(k, 24)


def test_second_insert_into_a_non_empty_index():
    _need_gpu()
    _same_index(31, 24, [_sequence(21, N_ROUTES, 31), _sequence(22, N_ROUTES, 31)])


class _Words:
    """The words of one sequence of N_WORDS k-mers (K = 31, PREFIX_BITS = 24) on the device, the index bytes insert_seqs gives for it and
    the oracle's: computed once, left unchanged by the tests."""

    def __init__(self):
        k, pb = 31, 24
        self.k, self.pb = k, pb
        bases, offsets = _sequence(31, N_WORDS, k)
        pad = (-len(bases)) % 16 + 16
        d_b = torch.from_numpy(np.concatenate([bases, np.zeros(pad, np.uint8)])).cuda()
        d_o = torch.from_numpy(offsets.astype(np.int64)).cuda()
        g = cbl_amd.CBL(k, pb)
        self.suffix_bits = g.consts()["suffix_bits"]
        assert g.consts()["hi_bytes"] == 1 and g.consts()["word_bits"] == self.suffix_bits + pb
        self.lo = torch.zeros(N_WORDS + 1, dtype=torch.int64, device="cuda")
        hi = torch.zeros(N_WORDS + 1, dtype=torch.uint8, device="cuda")
        assert g.seq_words_device(d_b, d_o, 1, self.lo, hi, N_WORDS) == N_WORDS
        self.hi = hi[:N_WORDS].clone()
        g.insert_seqs(bases, offsets)
        self.blob = g.serialize()
        g.close()
        o = Oracle(k, pb, False)
        o.insert_seqs(bases, offsets)
        self.oracle_blob = o.serialize()
        self.lo_np = self.lo[:N_WORDS].cpu().numpy().view(np.uint64)
        self.hi_np = self.hi.cpu().numpy()

    def hi_at(self, off):
        """the hi bytes at buf[off : off + n] of a fresh allocation (allocations start on a 256-byte boundary at least)"""
        buf = torch.zeros(N_WORDS + 16, dtype=torch.uint8, device="cuda")
        assert buf.data_ptr() % 8 == 0
        view = buf[off: off + N_WORDS]
        view.copy_(self.hi)
        assert view.data_ptr() % 8 == off
        return buf, view


_words = None


def words():
    global _words
    if _words is None:
        _words = _Words()
    return _words


def test_the_word_stream_is_the_sequence():
    _need_gpu()
    w = words()
    assert w.blob == w.oracle_blob


@pytest.mark.parametrize("off", OFFSETS)
def test_insert_words_with_misaligned_hi(off):
    _need_gpu()
    w = words()
    buf, hi = w.hi_at(off)
    g = cbl_amd.CBL(w.k, w.pb)
    g.insert_words_device(w.lo, hi, N_WORDS)
    blob = g.serialize()
    g.close()
    assert blob == w.blob, "index differs from insert_seqs on the same reads"
    assert blob == w.oracle_blob, "index differs from the oracle"
    del buf


@pytest.mark.parametrize("off", (0,) + OFFSETS)
def test_partition_words_with_misaligned_hi(off):
    """Three destinations; the reference is a numpy stable partition of the input words by destination = #{bounds <= prefix}."""
    _need_gpu()
    w = words()
    buf, hi = w.hi_at(off)
    sb = np.uint64(w.suffix_bits)
    prefix = ((w.lo_np >> sb) | (w.hi_np.astype(np.uint64) << (np.uint64(64) - sb))) & np.uint64((1 << w.pb) - 1)
    ranked = np.sort(prefix)
    bounds = np.array([ranked[N_WORDS // 3], ranked[2 * N_WORDS // 3]], dtype=np.uint32)  # terciles of the data: no destination is empty
    dest = np.searchsorted(bounds.astype(np.uint64), prefix, side="right")
    want_counts = np.bincount(dest, minlength=3).tolist()
    assert min(want_counts) > 0, want_counts
    order = np.argsort(dest, kind="stable")
    out_lo = torch.zeros(N_WORDS, dtype=torch.int64, device="cuda")
    out_hi = torch.zeros(N_WORDS, dtype=torch.uint8, device="cuda")
    g = cbl_amd.CBL(w.k, w.pb)
    counts = g.partition_words_device(w.lo, hi, N_WORDS, bounds, 3, out_lo, out_hi)
    g.close()
    assert counts == want_counts
    assert np.array_equal(out_lo.cpu().numpy().view(np.uint64), w.lo_np[order])
    assert np.array_equal(out_hi.cpu().numpy(), w.hi_np[order])
    del buf


def test_dirty_reads():
    """2 000 reads of 150 bp, every 50th with an N at a position of its own: the k-mer stream is cut into pieces of odd lengths."""
    _need_gpu()
    k, n_reads, L = 31, 2000, 150
    rng = np.random.default_rng(41)
    bases = rng.choice(ACGT, size=n_reads * L).astype(np.uint8)
    offsets = np.arange(n_reads + 1, dtype=np.uint64) * np.uint64(L)
    n_kmers = 0
    for r in range(n_reads):
        if r % 50 == 0:
            p = 4 + r // 50  # 4 .. 43
            bases[r * L + p] = ord("N")
            n_kmers += max(p - k + 1, 0) + max(L - p - 1 - k + 1, 0)
        else:
            n_kmers += L - k + 1
    assert n_kmers % 8 != 0, n_kmers
    _same_index(k, 24, [(bases, offsets)])
