"""The arithmetic chunk plan (cbl_amd/csrc/uniform_plan.hpp, plan_chunks in pipeline.hpp, the prologue of k_encode): a batch of reads of
one length L, K <= L <= K + 2047, without an invalid byte builds no chunk table; KRN-1 takes chunk and tile positions from
(offsets[0], L, K). Any other batch builds the tables as before.

Every case inserts the same device batches twice, with the arithmetic plan allowed and with CBLX_UNIFORM_PLAN=0, and holds both
serialized indexes against the CPU oracle's, byte for byte. CBL.uniform_plans() says which plan ran: it must rise by one per batch
exactly where the case expects the arithmetic plan, and never with the switch off.

Shapes: L = K, K + 1, 64 (divides the 4 KiB tile) and 150 with 3001 reads (reads straddle tile edges at every phase); L = K + 2047
(2048 k-mers: the largest single chunk, arithmetic) and K + 2048 (two chunks per read: tables); 1, 2, 27 and 28 reads of 150 bp (a tile
holds 27.3); offsets[0] 1 .. 15 bytes past a 16-byte boundary with N in front of it; canonical; K = 21 and 59; PREFIX_BITS 8, 24, 28; a
second insert into the non-empty index. Fallbacks: one read a base longer (first, middle, last), alone and with another read a base
shorter so that the total still divides; an N as the first, a middle and the last byte; a read shorter than K (same error text either
way). Lower case bases stay arithmetic."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
N_MANY = 3001


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _reads(seed, lengths, lead=0):
    """Random reads of the given lengths back to back behind `lead` bytes of N: (bases, offsets) with offsets[0] = lead."""
    lengths = np.asarray(lengths, dtype=np.uint64)
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.uint64) + np.uint64(lead)
    bases = np.concatenate([np.full(lead, ord("N"), np.uint8), rng.choice(ACGT, size=int(lengths.sum())).astype(np.uint8)])
    return bases, offsets


def _device(bases, offsets):
    pad = (-len(bases)) % 16 + 16
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(pad, np.uint8)])).cuda()
    assert d_b.data_ptr() % 16 == 0
    return d_b, torch.from_numpy(offsets.astype(np.int64)).cuda()


def _check(monkeypatch, k, pb, canonical, batches, arithmetic):
    """batches: [(bases, offsets)]; arithmetic: per batch, whether the arithmetic plan must take it."""
    _need_gpu()
    o = Oracle(k, pb, canonical)
    for bases, offsets in batches:
        o.insert_seqs(bases, offsets)
    want = o.serialize()
    dev = [_device(b, off) for b, off in batches]
    for allowed in (True, False):
        if allowed:
            monkeypatch.delenv("CBLX_UNIFORM_PLAN", raising=False)
        else:
            monkeypatch.setenv("CBLX_UNIFORM_PLAN", "0")
        g = cbl_amd.CBL(k, pb, canonical=canonical)
        for (d_b, d_o), (_, offsets), fast in zip(dev, batches, arithmetic):
            before = g.uniform_plans()
            g.insert_seqs_device(d_b, d_o, len(offsets) - 1)
            assert g.uniform_plans() - before == (1 if fast and allowed else 0), (allowed, fast)
        assert g.count() == o.count(), allowed
        blob = g.serialize()
        g.close()
        assert blob == want, "serialized index differs from the oracle (arithmetic plan %s)" % ("allowed" if allowed else "off")


@pytest.mark.parametrize("L", [31, 32, 64, 150])
def test_read_lengths(monkeypatch, L):
    _check(monkeypatch, 31, 24, False, [_reads(100 + L, [L] * N_MANY)], [True])


def test_largest_single_chunk_is_arithmetic(monkeypatch):
    _check(monkeypatch, 31, 24, False, [_reads(7, [31 + 2047] * 5)], [True])


def test_two_chunks_per_read_take_the_tables(monkeypatch):
    _check(monkeypatch, 31, 24, False, [_reads(8, [31 + 2048] * 5)], [False])


@pytest.mark.parametrize("nseq", [1, 2, 27, 28])
def test_few_reads(monkeypatch, nseq):
    _check(monkeypatch, 31, 24, False, [_reads(200 + nseq, [150] * nseq)], [True])


@pytest.mark.parametrize("lead", range(1, 16))
def test_offsets_inside_a_larger_buffer(monkeypatch, lead):
    """offsets[0] = lead: the bytes in front of it are N and belong to no read."""
    _check(monkeypatch, 31, 24, False, [_reads(300 + lead, [150] * 301, lead=lead)], [True])


@pytest.mark.parametrize("k,pb,canonical", [(31, 24, True), (21, 24, False), (21, 24, True), (59, 24, False), (59, 24, True), (31, 8, False), (31, 28, False),
                                            (31, 28, True)])
def test_word_layouts_and_prefix_bits(monkeypatch, k, pb, canonical):
    _check(monkeypatch, k, pb, canonical, [_reads(400 + k + pb, [150] * N_MANY)], [True])


def test_second_insert_into_a_non_empty_index(monkeypatch):
    _check(monkeypatch, 31, 24, False, [_reads(51, [150] * N_MANY), _reads(52, [100] * 2000, lead=5), _reads(53, [150] * 999 + [151])], [True, True, False])


@pytest.mark.parametrize("where", [0, 150, 300])
def test_one_longer_read(monkeypatch, where):
    lengths = [150] * 301
    lengths[where] = 151
    _check(monkeypatch, 31, 24, False, [_reads(60 + where, lengths)], [False])


@pytest.mark.parametrize("where", [0, 150, 300])
def test_one_longer_and_one_shorter_read(monkeypatch, where):
    """The total still divides by the number of reads: only the probe's look at every length tells."""
    lengths = [150] * 301
    lengths[where] = 151
    lengths[(where + 7) % 301] = 149
    _check(monkeypatch, 31, 24, False, [_reads(70 + where, lengths)], [False])


@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_one_invalid_byte(monkeypatch, where):
    bases, offsets = _reads(81, [150] * 301, lead=3)
    at = {"first": 3, "middle": 3 + 150 * 150 + 77, "last": len(bases) - 1}[where]
    bases[at] = ord("N")
    _check(monkeypatch, 31, 24, False, [(bases, offsets)], [False])


def test_lower_case_is_arithmetic(monkeypatch):
    bases, offsets = _reads(91, [150] * N_MANY)
    bases[::3] |= 0x20
    _check(monkeypatch, 31, 24, False, [(bases, offsets)], [True])


@pytest.mark.parametrize("lengths", [[40] * 5 + [20] + [40] * 5, [60, 20] + [40] * 9, [20] * 11])
def test_short_read_gives_the_same_error(monkeypatch, lengths):
    _need_gpu()
    bases, offsets = _reads(95, lengths)
    d_b, d_o = _device(bases, offsets)
    texts = []
    for allowed in (True, False):
        if allowed:
            monkeypatch.delenv("CBLX_UNIFORM_PLAN", raising=False)
        else:
            monkeypatch.setenv("CBLX_UNIFORM_PLAN", "0")
        g = cbl_amd.CBL(31, 24)
        with pytest.raises(cbl_amd.CblxError) as e:
            g.insert_seqs_device(d_b, d_o, len(lengths))
            g.flush()
        assert g.uniform_plans() == 0
        g.close()
        assert e.value.code == cbl_amd.ESHORT
        texts.append(str(e.value))
    assert texts[0] == texts[1]
    assert "Sequence size (20) is smaller than K (31)" in texts[0]
