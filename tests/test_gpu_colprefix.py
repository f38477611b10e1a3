"""The partition with two-level column prefixes (cbl_amd/csrc/colprefix.hpp: 16 tiles to a super-tile, u16 prefixes inside it, a flat
scan over the super-tile sums only): the serialized index of a build against the CPU oracle's for the same input, byte for byte.

One sequence of N + K - 1 bases gives exactly N k-mers, so pass A runs on exactly ceil(N / 4096) tiles: N is taken either side of
every super-tile edge (1, 15, 16, 17 and 33 tiles; the segment tiles of the passes behind it are ragged by nature). At N = 65 537
every route of the partition: PREFIX_BITS 8 (pass A alone), 12, 16, 20 (one and two LSD passes, tables or fused directory), 28
(the FINE route), K = 21 (no hi part), K = 59 (u64 hi, wide suffix), and a second insert into the non-empty index. A skewed
sequence of 600 000 k-mers (P(A) = 0.5) puts more than 262 144 words into the segment of top digit 0, which then takes group-cut
tiles and k_dir_gather while the other segments stay cold; with P(A) = 0.7 the largest bucket takes the long-run path, whose own
partition keeps the flat column prefixes next to the two-level ones."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
EDGE_N = (1, 4095, 4096, 4097, 61441, 65535, 65536, 65537, 69633, 131073)
N_ROUTES = 65537


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _sequence(seed, n_kmers, k, p_a=0.25):
    rng = np.random.default_rng(seed)
    rest = (1.0 - p_a) / 3
    bases = rng.choice(ACGT, size=n_kmers + k - 1, p=[p_a, rest, rest, rest]).astype(np.uint8)
    return bases, np.array([0, bases.size], dtype=np.uint64)


def _same_index(k, pb, inserts):
    g = cbl_amd.CBL(k, pb)
    o = Oracle(k, pb, False)
    for bases, offsets in inserts:
        g.insert_seqs(bases, offsets)
        o.insert_seqs(bases, offsets)
        assert g.count() == o.count()
        assert g.serialize() == o.serialize(), "serialized index differs from the oracle"
    g.close()
    return o


@pytest.mark.parametrize("n", EDGE_N)
def test_super_tile_edges(n):
    _need_gpu()
    _same_index(31, 24, [_sequence(1000 + n, n, 31)])


@pytest.mark.parametrize("k,pb", [(31, 8), (31, 12), (31, 16), (31, 20), (31, 28), (21, 24), (59, 24)])
def test_routes(k, pb):
    _need_gpu()
    _same_index(k, pb, [_sequence(7 * k + pb, N_ROUTES, k)])


def test_second_insert_into_a_non_empty_index():
    _need_gpu()
    _same_index(31, 24, [_sequence(11, N_ROUTES, 31), _sequence(12, N_ROUTES, 31)])


def _top_digit_counts(o, bases, k, pb):
    """records per value of the top 8 prefix bits (the segments of pass A), from the oracle's words"""
    cap = bases.size + 1
    lo, hi = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    seq = bases.tobytes()
    n = o._L.oracle_seq_words(o._h, seq, len(seq), 0, lo.ctypes.data, hi.ctypes.data, cap)
    assert n == bases.size - k + 1
    wb = 2 * k + (2 * k - 1).bit_length()
    assert 64 < wb <= 72
    sh = np.uint64(wb - 8)
    top = ((lo[:n] >> sh) | (hi[:n] << np.uint64(64 - (wb - 8)))) & np.uint64(255)
    return np.bincount(top.astype(np.int64), minlength=256)


def test_group_cut_tiles_and_dir_gather():
    """P(A) = 0.5: the segment of top digit 0 is above the 262 144-record threshold (64 tiles) and is cut at its groups; every other
    segment that holds records stays below it."""
    _need_gpu()
    k, pb, n = 31, 24, 600000
    bases, offsets = _sequence(5, n, k, p_a=0.5)
    o = _same_index(k, pb, [(bases, offsets)])
    seg = _top_digit_counts(o, bases, k, pb)
    assert seg[0] >= 262144, seg[0]
    others = seg[1:][seg[1:] > 0]
    assert others.size > 0 and others.max() < 262144, others.max()


def test_long_run_path_keeps_the_flat_form():
    """P(A) = 0.7: the largest bucket (tens of thousands of words) goes down the long-run path, which partitions with a histogram
    and a flat column scan of its own."""
    _need_gpu()
    k, pb, n = 31, 24, 600000
    bases, offsets = _sequence(5, n, k, p_a=0.7)
    g = cbl_amd.CBL(k, pb)
    g.insert_seqs(bases, offsets)
    o = Oracle(k, pb, False)
    o.insert_seqs(bases, offsets)
    assert g.count() == o.count()
    _, length, _ = g.bucket_table_np()
    assert int(length.max()) > 4096  # longer than the in-LDS bucket classes take
    assert g.serialize() == o.serialize(), "serialized index differs from the oracle"
    g.close()
