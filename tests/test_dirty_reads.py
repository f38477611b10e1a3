"""tests/dirty_reads.py, the dirt the multi-rank tests put into the synthetic stream: the device form (torch) gives the host form's
(numpy) bytes for any slice, a slice dirtied on its own is that range of the dirtied stream, and every class of dirt occurs at
its stated rate. No GPU: the torch form runs on CPU tensors here (the GPU tests run it on cuda tensors)."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import dirty_reads as D  # noqa: E402  (tests/)
from cbl_amd import synth  # noqa: E402

_VALID = np.zeros(256, dtype=bool)
_VALID[list(b"ACGTacgt")] = True


@pytest.mark.parametrize("k,L", [(31, 150), (25, 120), (33, 150), (59, 250), (11, 5000)])
def test_numpy_and_torch_forms_give_the_same_bytes_for_any_slice(k, L):
    seed, nr = 41 + k, 700
    cuts = [0, 7 * L, 233 * L, 233 * L + 1, 500 * L, nr * L]
    all_n = [(300 * L, 310 * L), (600 * L + 5, 600 * L + 9)]
    whole, _ = synth.reads(23, nr, L)
    want = D.dirty_np(whole, 0, seed, L, k, cuts, all_n)
    assert want.dtype == np.uint8 and len(want) == len(whole) and not np.array_equal(want, whole)
    for first, n in ((0, nr), (1, 5), (233, 1), (232, 3), (299, 12), (450, 250), (699, 1)):
        for off in (0, 1, 17, L - 1):  # slices that start inside a read, too
            a, b = first * L + off, min((first + n) * L + off, nr * L)
            tb, _ = synth.reads_torch(23, n + 1, L, first_read=first, device="cpu")
            tb = tb[off: off + (b - a) + 16].clone()  # the slice's bytes and 16 more as the pad
            pad = tb[b - a:].clone()
            got = D.dirty_torch(tb, a, b - a, seed, L, k, cuts, all_n)
            assert torch.equal(got[b - a:], pad)  # the pad is left alone
            assert got[: b - a].numpy().tobytes() == want[a:b].tobytes(), (first, n, off)
            alone = D.dirty_np(whole[a:b], a, seed, L, k, cuts, all_n)
            assert alone.tobytes() == want[a:b].tobytes(), (first, n, off)
    assert D.dirty_torch(torch.zeros(16, dtype=torch.uint8), 0, 0, seed, L, k).tolist() == [0] * 16


def test_cuts_and_all_n_ranges():
    k, L, nr = 31, 150, 200
    whole, _ = synth.reads(23, nr, L)
    cuts = [1000, 16 * 90 + 3, 29998]
    d = D.dirty_np(whole, 0, 7, L, k, cuts, [(5000, 5300)])
    for c in cuts:
        assert not _VALID[d[c - 1]] and not _VALID[d[c]]
        for q in (c - 2, c + 1):  # lower case where the byte is still a base
            assert d[q] not in b"ACGT"
    assert (d[5000:5300] == ord("N")).all()


def test_every_class_occurs_at_its_rate():
    k, L, nr = 31, 150, 20000
    n = nr * L
    p = np.arange(n, dtype=np.int64)
    m = D.classes(D._Np, p, 3, L, k)
    frac = {c: m[c].mean() for c in ("lower", "n", "other")}
    assert abs(frac["lower"] - 0.020) < 0.002 and abs(frac["n"] - 0.003) < 0.0006 and abs(frac["other"] - 0.003) < 0.0006, frac
    assert set(np.unique(m["other_byte"][m["other"]]).tobytes()) == set(D._OTHER)
    whole, _ = synth.reads(23, nr, L)
    d = D.dirty_np(whole, 0, 3, L, k)
    # runs of N: every length from 1 to 3 K occurs in the run class (seen through its mask), and one run per ~2700 bases
    r = m["run"].astype(np.int8)
    e = np.flatnonzero(np.diff(np.concatenate([[0], r, [0]])))
    lens = e[1::2] - e[0::2]
    assert 1 <= lens.min() <= 3 and 2 * k < lens.max() <= 3 * k * 2 and abs(len(lens) / (n / 64) - 6 / 256) < 0.006, (lens.min(), lens.max(), len(lens))
    reads = d.reshape(nr, L)
    valid = _VALID[reads]
    nvalid = valid.sum(1)
    all_n = (nvalid == 0).mean()
    few = ((nvalid > 0) & (nvalid < k)).mean()
    head = (~valid[:, :k]).any(1).mean()
    assert abs(all_n - 3 / 256) < 0.004 and 2 / 256 < few < 6 / 256 and head > 8 / 256, (all_n, few, head)
    assert abs(np.isin(d, list(b"acgt")).mean() - 0.02) < 0.003  # lower case bases: valid, kept as bases
    assert set(np.unique(d).tobytes()) >= set(b"ACGTacgtN" + D._OTHER)


def test_lower_case_gives_the_same_index():
    """Lower case bytes are bases: the oracle's index of the dirtied stream equals the index of its upper-cased bytes
    (n / e9 / ff ... stay skipped either way)."""
    from oracle import Oracle

    k, L, nr = 31, 150, 600
    hb, ho = synth.reads(23, nr, L)
    d = D.dirty_np(hb, 0, 9, L, k)
    up = np.frombuffer(d.tobytes().upper(), dtype=np.uint8)
    assert not np.array_equal(d, up)
    a, b, c = Oracle(k, 24), Oracle(k, 24), Oracle(k, 24)
    a.insert_seqs(d, ho)
    b.insert_seqs(up, ho)
    c.insert_seqs(hb, ho)
    assert a.serialize() == b.serialize() and 0 < a.count() < c.count()
