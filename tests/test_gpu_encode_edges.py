"""KRN-1 (cbl_amd/csrc/kernels_encode.hpp: the chunk-table kernels, k_encode, k_encode_dirty_wave) on the crafted batches of tests/encode_shapes.py,
whose geometry tests/test_encode_shapes.py pins on the CPU: the fullest tile the chunk rules allow and the most chunks a tile can own (every LDS
capacity of k_encode, three windows of the fused histogram); equal-length reads of 1, 2, 3, 127 .. 129, 255 .. 257, 511, 2047 and 2048 k-mers (the
carried (chunk, position) of the in-tile uniform loop around the divisors of 256) with a twin whose last read is one base longer; reads of 1, 2,
2047 .. 2049, 4095 .. 4097 and 6145 k-mers in three orders (chunk seams, canonical reordering at every seam, a last tile without a chunk start);
a full chunk that starts at byte 4094 .. 4097 of the stream with offsets[0] 0, 1, 8, 15 bytes past a 16-byte boundary; one N at every place
of a three-chunk read that matters (first K bytes, 64-byte ballot steps, chunk overlaps), reads of N alone, `n` at bytes 62 .. 64; dirty reads
among clean ones (idle waves in the last workgroup of the dirty kernel, three k_dirty_list workgroups); and, for every odd K from 5 to 59, the
zero-run families of tests/host/necklace_fused_unit.cpp as k-mers, so that the device's three-input forms of the necklace see them.

Words: cblx_seq_words_device through the raw ABI into arrays of n + 3 elements filled with 0xA5: the count, every word in order against
oracle.pyref (the first difference is reported with its read, chunk and slot from the model), and the three elements behind stay as they were.
Index: insert_seqs_device into an empty index with the arithmetic plan allowed and with CBLX_UNIFORM_PLAN=0, bytes against the C++ oracle's
(the only observer of the fused histogram); uniform_plans() rises exactly where the model says the plan is arithmetic. Every case canonical and not;
PREFIX_BITS 24, or 8 where the word is shorter than that (K <= 9)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd import synth  # noqa: E402
from oracle import Oracle  # noqa: E402

import encode_shapes as es  # noqa: E402

FILL = 0xA5
FILL64 = 0xA5A5A5A5A5A5A5A5
PAD = 3
FIRST_READS = 3000


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _param(cases):
    return pytest.mark.parametrize("case", cases, ids=[es.case_id(c) for c in cases])


def _device(bases, offsets):
    pad = (-len(bases)) % 16 + 16
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(pad, np.uint8)])).cuda()
    assert d_b.data_ptr() % 16 == 0
    return d_b, torch.from_numpy(offsets.astype(np.int64)).cuda()


def _check_words(case, canonical):
    _need_gpu()
    b = es.batch(case)
    want = es.reference_words(b, canonical)
    n = len(want)
    g = cbl_amd.CBL(b.K, b.pb, canonical=canonical)
    hb = g.consts()["hi_bytes"]
    d_b, d_o = _device(b.bases, b.offsets)
    d_lo = torch.from_numpy(np.full(n + PAD, FILL64, dtype=np.uint64).view(np.int64)).cuda()
    d_hi = None if hb == 0 else torch.full((n + PAD,), FILL, dtype=torch.uint8, device="cuda") if hb == 1 else d_lo.clone()
    got = C.c_uint64(12345)
    rc = cbl_amd.lib().cblx_seq_words_device(g._h, d_b.data_ptr(), d_o.data_ptr(), len(b.reads), d_lo.data_ptr(), None if d_hi is None else d_hi.data_ptr(), n,
                                             C.byref(got))
    assert rc == 0, g._L.cblx_last_error(g._h)
    assert got.value == n == b.geometry.n_kmers
    lo = d_lo.cpu().numpy().view(np.uint64)
    hi = None if d_hi is None else d_hi.cpu().numpy() if hb == 1 else d_hi.cpu().numpy().view(np.uint64)
    g.close()
    wlo, whi = es.words_as_arrays(want)
    assert hb != 0 or not whi.any()
    if hb == 1:
        assert int(whi.max(initial=0)) < 256
    diff = lo[:n] != wlo
    if hi is not None:
        diff |= hi[:n].astype(np.uint64) != whi
    bad = np.flatnonzero(diff)
    if len(bad):
        i = int(bad[0])
        pytest.fail("%d of %d words differ, the first at slot %d: gpu %#x:%016x, pyref %#x:%016x; %s" % (
            len(bad), n, i, 0 if hi is None else int(hi[i]), int(lo[i]), int(whi[i]), int(wlo[i]), es.locate(b.geometry, i)))
    assert (lo[n:] == FILL64).all(), "elements behind the last word were written"
    if hi is not None:
        assert (hi[n:] == (FILL if hb == 1 else FILL64)).all(), "hi elements behind the last word were written"


def _check_index(monkeypatch, case, canonical, first=None):
    """The batch into an empty index (or behind `first`, a batch of its own), tables allowed to be arithmetic and not: bytes against the oracle's."""
    _need_gpu()
    b = es.batch(case)
    o = Oracle(b.K, b.pb, canonical)
    batches = ([first] if first is not None else []) + [(b.bases, b.offsets)]
    for bases, offsets in batches:
        o.insert_seqs(bases, offsets)
    want = o.serialize()
    dev = [_device(bases, offsets) for bases, offsets in batches]
    for allowed in (True, False):
        if allowed:
            monkeypatch.delenv("CBLX_UNIFORM_PLAN", raising=False)
        else:
            monkeypatch.setenv("CBLX_UNIFORM_PLAN", "0")
        g = cbl_amd.CBL(b.K, b.pb, canonical=canonical)
        for (d_b, d_o), (_, offsets) in zip(dev[:-1], batches[:-1]):
            g.insert_seqs_device(d_b, d_o, len(offsets) - 1)
        before = g.uniform_plans()
        g.insert_seqs_device(dev[-1][0], dev[-1][1], len(b.reads))
        rose = g.uniform_plans() - before
        count, blob = g.count(), g.serialize()
        g.close()
        assert rose == (1 if allowed and b.geometry.arithmetic else 0), (allowed, b.geometry.arithmetic)
        assert count == o.count(), allowed
        assert blob == want, "serialized index differs from the oracle (arithmetic plan %s)" % ("allowed" if allowed else "off")


@pytest.mark.parametrize("canonical", [False, True])
@_param(es.CASES)
def test_words(case, canonical):
    _check_words(case, canonical)


@pytest.mark.parametrize("canonical", [False, True])
@_param(es.NECKLACE_CASES)
def test_necklace_words(case, canonical):
    _check_words(case, canonical)


@pytest.mark.parametrize("canonical", [False, True])
@_param(es.CASES)
def test_index(monkeypatch, case, canonical):
    name, args = case
    arithmetic = es.batch(case).geometry.arithmetic
    if name == "uniform_nk0":  # the plan is arithmetic for the equal-length batches and for nothing with a longer read, a second chunk or an N
        assert arithmetic == (not args[2])
    else:
        assert arithmetic == (name == "most_chunks")
    _check_index(monkeypatch, case, canonical)


@pytest.mark.parametrize("canonical", [False, True])
@_param([c for c in es.NECKLACE_CASES if c[1][0] in es.NECKLACE_INDEX_K])
def test_necklace_index(monkeypatch, case, canonical):
    _check_index(monkeypatch, case, canonical)


@pytest.mark.parametrize("canonical", [False, True])
@_param([c for c in es.CASES if c[0] in ("fullest_tile", "dirty_among_clean")])
def test_index_second_insert(monkeypatch, case, canonical):
    """behind 3 000 random reads of 150 bases: a non-empty index"""
    _check_index(monkeypatch, case, canonical, first=synth.reads(17, FIRST_READS, 150))
