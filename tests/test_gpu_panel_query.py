"""A batch against a panel of up to 64 indexes in one pass on the GPU: contains_seqs_counts_many, contains_seqs_counts_many_device and
`classify`, by the fallback (one k_contains per index on words encoded once) and by the panel join forced for every batch. Every expectation
comes from the CPU oracle through tests/panel_query_model.py (Oracle.seq_words per sequence, the Python set of each index's iter_words,
query_counts_shapes.tally_model per index), never from the GPU path; every output array is pre-filled with 0xA5..., so an entry that is not
written shows."""
import os
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd.__main__ import classify_report  # noqa: E402
from oracle import Oracle  # noqa: E402

import panel_query_model as pm  # noqa: E402  (tests/)
import query_counts_shapes as qc  # noqa: E402  (tests/)
import query_shapes as qs  # noqa: E402  (tests/)

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
JOIN_ENV = "CBLX_QUERY_JOIN_MIN"
FILL, FILL64, M64 = pm.FILL32, pm.FILL64, pm.M64
PAD = 3  # mask words behind the batch's k-mers: they keep their fill


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _routes(monkeypatch):
    """The fallback (small batches), then the panel join forced for every batch."""
    for join in (None, "1"):
        if join is None:
            monkeypatch.delenv(JOIN_ENV, raising=False)
        else:
            monkeypatch.setenv(JOIN_ENV, join)
        yield "join" if join else "fallback"
    monkeypatch.delenv(JOIN_ENV, raising=False)


def _device_batch(bases, offsets):
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros((-len(bases)) % 16 + 16, np.uint8)])).cuda()
    d_o = torch.from_numpy(np.asarray(offsets, dtype=np.uint64).astype(np.int64)).cuda()
    return d_b, d_o


def _filled32(*shape):
    return torch.full(shape, FILL - (1 << 32), dtype=torch.int32, device="cuda")


def _filled64(n):
    return torch.full((n,), FILL64 - (1 << 64), dtype=torch.int64, device="cuda")


def _srcs(cbls):
    return (C.c_void_p * len(cbls))(*[c._h for c in cbls])


def _host_raw(cbls, bases, offsets, total, positive, mask, cap, srcs=None, n=None):
    """cblx_contains_seqs_counts_many through the raw ABI: (status, n_out, positive[n])."""
    n = len(cbls) if n is None else n
    tot, pos = C.c_uint64(FILL64), np.full(max(n, 1), FILL64, dtype=np.uint64)
    rc = cbl_amd.lib().cblx_contains_seqs_counts_many(srcs if srcs is not None else _srcs(cbls), n, bases.ctypes.data, offsets.ctypes.data, len(offsets) - 1,
                                                      None if total is None else total.ctypes.data, None if positive is None else positive.ctypes.data,
                                                      None if mask is None else mask.ctypes.data, cap, C.byref(tot), pos.ctypes.data_as(C.POINTER(C.c_uint64)))
    return rc, tot.value, pos


def _host_many(cbls, bases, offsets, nk, with_mask):
    n, nseq = len(cbls), len(offsets) - 1
    total, positive = np.full(nseq, FILL, dtype=np.uint32), np.full((n, nseq), FILL, dtype=np.uint32)
    mask = np.full(nk + PAD, FILL64, dtype=np.uint64) if with_mask else None
    rc, tot, pos = _host_raw(cbls, bases, offsets, total, positive, mask, nk + PAD if with_mask else 0)
    assert rc == 0, cbls[0]._L.cblx_last_error(cbls[0]._h)
    return total, positive, mask, tot, pos


def _device_many(cbls, d_b, d_o, nseq, nk, with_mask):
    n = len(cbls)
    d_t, d_p, d_m = _filled32(nseq), _filled32(n, nseq), _filled64(nk + PAD) if with_mask else None
    tot, pos = C.c_uint64(FILL64), np.full(n, FILL64, dtype=np.uint64)
    rc = cbl_amd.lib().cblx_contains_seqs_counts_many_device(_srcs(cbls), n, d_b.data_ptr(), d_o.data_ptr(), nseq, d_t.data_ptr(), d_p.data_ptr(),
                                                             d_m.data_ptr() if with_mask else None, nk + PAD if with_mask else 0, C.byref(tot),
                                                             pos.ctypes.data_as(C.POINTER(C.c_uint64)))
    assert rc == 0, cbls[0]._L.cblx_last_error(cbls[0]._h)
    return (d_t.cpu().numpy().view(np.uint32), d_p.cpu().numpy().view(np.uint32), d_m.cpu().numpy().view(np.uint64) if with_mask else None, tot.value, pos)


def _check(got, want, cols, names, what):
    """`cols`: which indexes of `want` the panel holds, in panel order (bit j of the panel = column cols[j] of the expectation)."""
    total, positive, mask, tot, pos = got
    n, nk = len(cols), len(want.mask)
    assert total.dtype == np.uint32 and positive.dtype == np.uint32 and positive.shape == (n, len(want.total)), what
    bad = np.flatnonzero(total != want.total)
    assert not len(bad), f"{what}: total wrong at (sequence, name, got, expected) {[(int(i), names[i] if names else None, int(total[i]), int(want.total[i])) for i in bad[:8]]}"
    for j, col in enumerate(cols):
        bad = np.flatnonzero(positive[j] != want.positive[col])
        assert not len(bad), (f"{what}: row {j} wrong at (sequence, name, got, expected) "
                              f"{[(int(i), names[i] if names else None, int(positive[j][i]), int(want.positive[col][i])) for i in bad[:8]]}")
    assert tot == nk and pos.tolist() == [int(want.positive[col].sum(dtype=np.uint64)) for col in cols], what
    if mask is not None:
        exp = np.zeros(nk, dtype=np.uint64)
        for j, col in enumerate(cols):
            exp |= want.flags[col].astype(np.uint64) << np.uint64(j)
        bad = np.flatnonzero(mask[:nk] != exp)
        assert not len(bad), f"{what}: mask wrong at (k-mer, got, expected) {[(int(i), hex(int(mask[i])), hex(int(exp[i]))) for i in bad[:8]]}"
        assert (mask[nk:] == FILL64).all(), what


def _every_form(cbls, bases, offsets, want, cols, names, what):
    d_b, d_o = _device_batch(bases, offsets)
    nseq, nk = len(offsets) - 1, len(want.mask)
    for with_mask in (False, True):
        _check(_host_many(cbls, bases, offsets, nk, with_mask), want, cols, names, f"{what}, host, mask {with_mask}")
        _check(_device_many(cbls, d_b, d_o, nseq, nk, with_mask), want, cols, names, f"{what}, device, mask {with_mask}")


# ---- 1. every batch shape, every word class --------------------------------------------------------------------------------------------------
_panels = {}


def _panel_case(k, pb, canonical):
    """(batch, three oracles built from different overlapping parts of the batch's resident sequences, the expectation of the three), once per process."""
    key = (k, pb, canonical)
    if key not in _panels:
        b = qc.batch(k)
        res = qc.resident_seqs(b)
        parts = [[s for i, s in enumerate(res) if i % 4 != j] for j in range(3)]
        oracles = []
        for part in parts:
            o = Oracle(k, pb, canonical)
            o.insert_seqs(*qc.as_arrays(part))
            oracles.append(o)
        _panels[key] = (b, parts, oracles, pm.expect(oracles, b.seqs))
    return _panels[key]


@pytest.mark.parametrize("k,pb,canonical", qc.CONFIGS)
def test_panel_of_every_shape(k, pb, canonical, monkeypatch):
    _need_gpu()
    b, parts, oracles, want = _panel_case(k, pb, canonical)
    gs = []
    for part, o in zip(parts, oracles):
        g = cbl_amd.CBL(k, pb, canonical=canonical)
        g.insert_seqs(*qc.as_arrays(part))
        assert g.serialize() == o.serialize()
        gs.append(g)
    blobs = [g.serialize() for g in gs]
    assert len({tuple(r) for r in want.positive.tolist()}) == 3 and 0 < int(want.positive.sum())
    for how in _routes(monkeypatch):
        for n in (1, 2, 3):
            _every_form(gs[:n], b.bases, b.offsets, want, list(range(n)), b.names, f"n = {n}, {how}")
        # on the GPU as well: row j is contains_seqs_counts of index j alone, bit j its contains_seqs flags
        total, positive, mask, _, _ = _host_many(gs, b.bases, b.offsets, len(want.mask), True)
        for j, g in enumerate(gs):
            t1, p1 = g.contains_seqs_counts(b.bases, b.offsets)
            assert np.array_equal(t1, total) and np.array_equal(p1, positive[j]), (how, j)
            flags = g.contains_seqs(b.bases, b.offsets)[0]
            assert np.array_equal(((mask[: len(flags)] >> np.uint64(j)) & np.uint64(1)).astype(bool), flags), (how, j)
        # the Python surface
        t, p = cbl_amd.CBL.contains_seqs_counts_many(gs, b.bases, b.offsets)
        assert p.shape == (3, len(b.seqs)) and np.array_equal(t, want.total) and np.array_equal(p, want.positive), how
        t, p, m = cbl_amd.CBL.contains_seqs_counts_many(gs[::-1], b.bases, b.offsets, masks=True)
        _check((t, p, np.concatenate([m, np.full(PAD, FILL64, dtype=np.uint64)]), len(m), p.sum(axis=1, dtype=np.uint64)), want, [2, 1, 0], b.names, f"python, {how}")
    assert [g.serialize() for g in gs] == blobs and all(g.validate() == 0 for g in gs)  # a query changes nothing
    for g in gs:
        g.close()


# ---- 2. one prefix, every table class in one workgroup ---------------------------------------------------------------------------------------
BIG = 4600  # > JOIN_TAB_MAX words in one bucket; five shares of 920 leave one Vec of them behind `|=`
CLASS_LENGTHS = (1, qs.THRESHOLD, qs.THRESHOLD + 1, qs.JOIN_FULL_MAX, qs.JOIN_FULL_MAX + 1, qs.JOIN_TAB_MAX, qs.JOIN_TAB_MAX + 1)
_BASES = b"ACTG"  # 2-bit codes 0 .. 3, first base most significant


def _kmer_seq(o, word, k):
    x = o.kmer_of_word(word)
    return bytes(_BASES[(x >> (2 * (k - 1 - i))) & 3] for i in range(k))


def _insert_words(g, words):
    lo = torch.from_numpy(np.array([w & M64 for w in words], dtype=np.uint64).view(np.int64)).cuda()
    hb = g.consts()["hi_bytes"]
    hi = None
    if hb:
        a = np.array([w >> 64 for w in words], dtype=np.uint64)
        hi = torch.from_numpy(a.astype(np.uint8) if hb == 1 else a.view(np.int64)).cuda()
    g.insert_words_device(lo, hi, len(words))


def _pair(k, pb, words):
    g, o = cbl_amd.CBL(k, pb), Oracle(k, pb)
    if words:
        _insert_words(g, words)
        o.insert_words(words)
    assert g.serialize() == o.serialize()
    return g, o


def test_one_prefix_every_table_class(monkeypatch):
    _need_gpu()
    k, pb = 31, 5
    s = qs.craft(k, pb, False, (BIG,), 21, 14000)
    bucket = next(bk for bk in s.buckets.values() if bk.length == BIG and bk.edges == "inner")
    rng = random.Random(3)
    stored = list(bucket.elements)
    rng.shuffle(stored)  # the order of insertion: a Vec keeps it
    elsewhere = [w for w in dict.fromkeys(s.words) if w >> s.sb != bucket.prefix][:500]
    assert len(elsewhere) == 500
    pairs = [_pair(k, pb, stored[:L]) for L in CLASS_LENGTHS]  # index j: the first L_j words of the bucket
    pairs.append(_pair(k, pb, elsewhere))                       # does not hold the prefix
    pairs.append(_pair(k, pb, []))                              # empty
    shares = [_pair(k, pb, stored[i * BIG // 5: (i + 1) * BIG // 5]) for i in range(5)]
    g, o = shares[0]
    for g2, o2 in shares[1:]:
        g |= g2
        o.merge(o2)
    assert g.serialize() == o.serialize() and g.count() == BIG
    pairs.append((g, o))                                        # one Vec of BIG words, not ascending
    table = {int(p): (int(ln), int(kd)) for p, ln, kd in zip(*g.bucket_table_np())}
    assert table[bucket.prefix] == (BIG, qs.VEC)
    kinds = [dict((int(p), int(kd)) for p, _, kd in zip(*x.bucket_table_np())).get(bucket.prefix) for x, _ in pairs]
    assert kinds == [qs.VEC, qs.VEC, qs.TRIE, qs.TRIE, qs.TRIE, qs.TRIE, qs.TRIE, None, None, qs.VEC]
    # queries: every word of the bucket, the candidates of the prefix no index holds, 300 copies of one k-mer, some words of other prefixes
    absent = [w for w in bucket.candidates if w not in set(bucket.elements)]
    qwords = list(bucket.elements) + absent + [stored[0]] * 300 + elsewhere[:40] + [stored[qs.THRESHOLD]] * 5
    rng.shuffle(qwords)
    ref = pairs[0][1]
    seqs = [_kmer_seq(ref, w, k) for w in qwords]
    assert [ref.seq_words(q)[0] for q in seqs[:200]] == qwords[:200] and len(absent) >= 3
    assert sum(w >> s.sb == bucket.prefix for w in qwords) > 1024 + 256  # one run: a lane owns several queries
    bases, offsets = qc.as_arrays(seqs)
    want = pm.expect([o for _, o in pairs], seqs, words=qwords)
    assert [int(r.sum()) > 0 for r in want.positive] == [True] * 8 + [False, True]
    gs = [x for x, _ in pairs]
    blobs = [x.serialize() for x in gs]
    orders = [list(range(len(gs))), list(range(len(gs)))[::-1], [9, 0, 6, 8, 1, 5, 7, 2, 4, 3], [3, 6, 0]]  # a short bucket behind a long one and the reverse
    for how in _routes(monkeypatch):
        for order in orders:
            _every_form([gs[i] for i in order], bases, offsets, want, order, None, f"order {order}, {how}")
    assert [x.serialize() for x in gs] == blobs  # Vecs in their stored order among them: nothing was sorted
    for x, _ in pairs + shares[1:]:
        x.close()


# ---- 3. n = 64 -------------------------------------------------------------------------------------------------------------------------------
def _pattern(i):
    """A fixed 64-bit pattern of k-mer i (splitmix64), with the edges up front."""
    fixed = [M64, 1 << 63, 1 << 31, 1 << 32, (1 << 32) | (1 << 31), 0, 1, (1 << 33) - 1, M64 ^ (1 << 32)]
    if i < len(fixed):
        return fixed[i]
    z = (i * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def test_panel_of_64(monkeypatch):
    _need_gpu()
    k, pb = 31, 5
    s = qs.craft(k, pb, False, (400,), 22, 14000)
    bucket = next(bk for bk in s.buckets.values() if bk.length == 400 and bk.edges == "inner")
    others = [w for w in dict.fromkeys(s.words) if w >> s.sb != bucket.prefix][:60]
    words = list(bucket.elements[:300]) + others  # k-mer i: one shared prefix and a few others
    pat = [_pattern(i) for i in range(len(words))]
    pairs = [_pair(k, pb, [w for w, p in zip(words, pat) if (p >> j) & 1]) for j in range(64)]
    ref = pairs[0][1]
    qwords = words + words[:50]  # every k-mer, some twice
    seqs = [_kmer_seq(ref, w, k) for w in qwords]
    bases, offsets = qc.as_arrays(seqs)
    want = pm.expect([o for _, o in pairs], seqs, words=qwords)
    assert want.mask.tolist() == [_pattern(i) for i in range(len(words))] + pat[:50]  # the masks ARE the patterns
    gs = [x for x, _ in pairs]
    for how in _routes(monkeypatch):
        for n in (64, 33):
            got = _host_many(gs[:n], bases, offsets, len(qwords), True)
            _check(got, want, list(range(n)), None, f"n = {n}, {how}")
            assert got[2][: len(qwords)].tolist() == [p & ((1 << n) - 1) for p in pat + pat[:50]], (n, how)  # bits n and above are 0
            _check(_device_many(gs[:n], *_device_batch(bases, offsets), len(seqs), len(qwords), True), want, list(range(n)), None, f"device, n = {n}, {how}")
    # the occupancy histogram of the same panel is the popcount histogram of the distinct k-mers that are held (last: it sorts Vec buckets)
    hist = cbl_amd.CBL.occupancy(gs)
    pop = np.bincount([bin(p).count("1") for p in pat], minlength=65)
    pop[0] = 0
    assert hist.tolist() == pop.tolist()
    for x in gs:
        x.close()


# ---- 4. the contract -------------------------------------------------------------------------------------------------------------------------
def test_contract_cases(monkeypatch):
    _need_gpu()
    k, pb = 31, 24
    b, parts, oracles, want = _panel_case(k, pb, False)
    nseq, nk = len(b.seqs), len(want.mask)
    gs = []
    for part in parts:
        g = cbl_amd.CBL(k, pb)
        g.insert_seqs(*qc.as_arrays(part))
        gs.append(g)
    d_b, d_o = _device_batch(b.bases, b.offsets)
    L = cbl_amd.lib()
    # pending insert_seq calls are seen: the third index gets its sequences one by one, without a flush
    late = cbl_amd.CBL(k, pb)
    for q in parts[2]:
        late.insert_seq(q)
    for how in _routes(monkeypatch):
        first = _host_many(gs[:2] + [late], b.bases, b.offsets, nk, True)
        _check(first, want, [0, 1, 2], b.names, f"pending inserts, {how}")
        assert late.serialize() == oracles[2].serialize()
        again = _host_many(gs[:2] + [late], b.bases, b.offsets, nk, True)  # a second call on the same contexts
        assert all(np.array_equal(x, y) for x, y in zip(first[:3], again[:3])) and first[3] == again[3] and first[4].tolist() == again[4].tolist()
        # empty operands count towards n: their rows and bits are 0, wherever they stand
        e1, e2 = cbl_amd.CBL(k, pb), cbl_amd.CBL(k, pb)
        z = pm.Panel(want.total, np.concatenate([want.positive, np.zeros((1, nseq), dtype=np.uint32)]), want.mask,
                     np.concatenate([want.flags, np.zeros((1, nk), dtype=bool)]))
        _every_form([e1, gs[1], e2, gs[0]], b.bases, b.offsets, z, [3, 1, 3, 0], b.names, f"empty among others, {how}")
        _every_form([e1, gs[2]], b.bases, b.offsets, z, [3, 2], b.names, f"one non-empty behind an empty one, {how}")
        _every_form([e1, e2], b.bases, b.offsets, z, [3, 3], b.names, f"all empty, {how}")
        _every_form([e1], b.bases, b.offsets, z, [3], b.names, f"one empty, {how}")
        e1.close()
        e2.close()
        # a slice of a larger buffer: offsets[0] > 0 and not 16-byte aligned
        a, zz = next(i for i in range(3, 12) if int(b.offsets[i]) % 16), 40
        k0, k1 = int(want.total[:a].sum()), int(want.total[:zz].sum())
        part_want = pm.Panel(want.total[a:zz], want.positive[:, a:zz], want.mask[k0:k1], want.flags[:, k0:k1])
        _check(_host_many(gs, b.bases, b.offsets[a: zz + 1].copy(), k1 - k0, True), part_want, [0, 1, 2], b.names[a:zz], f"slice, host, {how}")
        _check(_device_many(gs, d_b, d_o[a: zz + 1].clone(), zz - a, k1 - k0, True), part_want, [0, 1, 2], b.names[a:zz], f"slice, device, {how}")
        # only some of the arrays
        total = np.full(nseq, FILL, dtype=np.uint32)
        rc, tot, pos = _host_raw(gs, b.bases, b.offsets, total, None, None, 0)
        assert rc == 0 and np.array_equal(total, want.total) and tot == nk and pos.tolist() == want.positive.sum(axis=1, dtype=np.uint64).tolist(), how
        mask = np.full(nk, FILL64, dtype=np.uint64)
        rc, tot, pos = _host_raw(gs, b.bases, b.offsets, None, None, mask, nk)  # a capacity of exactly the k-mer count
        assert rc == 0 and np.array_equal(mask, want.mask), how
        # nseq == 0: nothing is written but the two tallies
        t4, p4, m4 = np.full(4, FILL, dtype=np.uint32), np.full((3, 4), FILL, dtype=np.uint32), np.full(4, FILL64, dtype=np.uint64)
        rc, tot, pos = _host_raw(gs, b.bases, np.zeros(1, dtype=np.uint64), t4, p4, m4, 4)
        assert rc == 0 and tot == 0 and pos.tolist() == [0, 0, 0] and (t4 == FILL).all() and (p4 == FILL).all() and (m4 == FILL64).all(), how
        t0, p0, m0 = cbl_amd.CBL.contains_seqs_counts_many(gs, b.bases[:0], np.zeros(1, dtype=np.uint64), masks=True)
        assert t0.shape == (0,) and p0.shape == (3, 0) and m0.shape == (0,)
        # one sequence of K - 1 bases: ESHORT; a mask capacity one short: ERANGE. The pre-filled arrays, n_out and positive stay as they were
        short_seqs = b.seqs[:3] + [b.seqs[3][: k - 1]] + b.seqs[4:8]
        sb, so = qc.as_arrays(short_seqs)
        for panel in (gs, gs[:1]):
            n = len(panel)
            for bases, offsets, cap, code in ((sb, so, 1 << 20, cbl_amd.ESHORT), (b.bases, b.offsets, nk - 1, cbl_amd.ERANGE)):
                ns = len(offsets) - 1
                t, p, m = np.full(ns, FILL, dtype=np.uint32), np.full((n, ns), FILL, dtype=np.uint32), np.full(nk + PAD, FILL64, dtype=np.uint64)
                rc, tot, pos = _host_raw(panel, bases, offsets, t, p, m, cap)
                assert rc == code and tot == FILL64 and (pos == FILL64).all(), (how, n, code)
                assert (t == FILL).all() and (p == FILL).all() and (m == FILL64).all(), (how, n, code)
                xb, xo = _device_batch(bases, offsets)
                d_t, d_p, d_m = _filled32(ns), _filled32(n, ns), _filled64(nk + PAD)
                tot, pos = C.c_uint64(FILL64), np.full(n, FILL64, dtype=np.uint64)
                rc = L.cblx_contains_seqs_counts_many_device(_srcs(panel), n, xb.data_ptr(), xo.data_ptr(), ns, d_t.data_ptr(), d_p.data_ptr(), d_m.data_ptr(), cap,
                                                             C.byref(tot), pos.ctypes.data_as(C.POINTER(C.c_uint64)))
                assert rc == code and tot.value == FILL64 and (pos == FILL64).all(), (how, n, code)
                assert (d_t.cpu().numpy().view(np.uint32) == FILL).all() and (d_p.cpu().numpy().view(np.uint32) == FILL).all(), (how, n, code)
                assert (d_m.cpu().numpy().view(np.uint64) == FILL64).all(), (how, n, code)
        with pytest.raises(cbl_amd.CblxError) as ei:
            cbl_amd.CBL.contains_seqs_counts_many(gs, sb, so)
        assert ei.value.code == cbl_amd.ESHORT and "smaller than K" in str(ei.value)
    # every refusal of the operand checks: EINVAL, nothing written
    other_k, other_pb, canon = cbl_amd.CBL(29, pb), cbl_amd.CBL(k, 20), cbl_amd.CBL(k, pb, canonical=True)
    t, p = np.full(nseq, FILL, dtype=np.uint32), np.full((65, nseq), FILL, dtype=np.uint32)

    def refused(handles, n=None):
        n = len(handles) if n is None else n
        arr = (C.c_void_p * max(len(handles), 1))(*handles)
        rc, tot, pos = _host_raw(None, b.bases, b.offsets, t, p, None, 0, srcs=arr, n=n)
        d_rc = L.cblx_contains_seqs_counts_many_device(arr, n, d_b.data_ptr(), d_o.data_ptr(), nseq, None, None, None, 0, None, None)
        return rc == d_rc == cbl_amd.EINVAL and tot == FILL64 and (pos == FILL64).all() and (t == FILL).all() and (p == FILL).all()

    h = [g._h for g in gs]
    assert refused(h, n=0)
    assert refused([h[i % 3] for i in range(65)])  # n = 65
    assert refused([h[0], None, h[1]])
    assert refused([h[0], h[1], h[0]])
    assert refused([h[0], other_k._h]) and refused([other_k._h, h[0]])
    assert refused([h[0], other_pb._h])
    assert refused([h[0], canon._h])
    assert L.cblx_contains_seqs_counts_many(None, 2, b.bases.ctypes.data, b.offsets.ctypes.data, nseq, None, None, None, 0, None, None) == cbl_amd.EINVAL
    with pytest.raises(ValueError):
        cbl_amd.CBL.contains_seqs_counts_many([], b.bases, b.offsets)
    with pytest.raises(ValueError):
        cbl_amd.CBL.contains_seqs_counts_many([gs[0], gs[0]], b.bases, b.offsets)
    # the Python device form allocates what it is not given
    d_t, d_p = cbl_amd.CBL.contains_seqs_counts_many_device(gs, d_b, d_o, nseq)
    assert d_p.shape == (3, nseq) and d_t.is_cuda and np.array_equal(d_p.cpu().numpy().view(np.uint32), want.positive)
    d_t, d_p, d_m = cbl_amd.CBL.contains_seqs_counts_many_device(gs, d_b, d_o, nseq, d_mask=_filled64(nk))
    assert np.array_equal(d_m.cpu().numpy().view(np.uint64), want.mask) and np.array_equal(d_t.cpu().numpy().view(np.uint32), want.total)
    for j, (g, o) in enumerate(zip(gs, oracles)):
        assert g.serialize() == o.serialize() and g.validate() == 0  # Vec buckets as stored: nothing was sorted
    for g in gs + [late, other_k, other_pb, canon]:
        g.close()


# ---- 5. the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_classify(tmp_path):
    _need_gpu()
    k, pb = 31, 24
    b, parts, oracles, _ = _panel_case(k, pb, False)
    keep = [i for i, name in enumerate(b.names) if name.startswith(("N-", "lower-", "all-N", "len-K", "short-", "tail"))] + [b.names.index("read-%d" % i) for i in range(40)]
    seqs = [b.seqs[i] for i in keep]
    seqs[3] = seqs[3].lower()
    assert any(b"N" in q for q in seqs) and any(q != q.upper() for q in seqs)
    want = pm.expect(oracles, seqs)
    fa = tmp_path / "reads.fa"
    with open(fa, "wb") as f:
        for i, q in enumerate(seqs):
            f.write(b">r%d some text\n" % i)
            for a in range(0, len(q), 70):
                f.write(q[a: a + 70] + b"\n")
    paths = []
    for j, o in enumerate(oracles):
        paths.append(str(tmp_path / f"index{j}.cbl"))
        with open(paths[-1], "wb") as f:
            f.write(o.serialize())
    for extra, frac, hits in (([], 0.5, 0), (["--min-fraction", "0.0", "--min-hits", "3"], 0.0, 3)):
        out = tmp_path / "classes.tsv"
        cmd = [sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb), "classify"] + paths + [str(fa), "-o", str(out)] + extra
        r = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, cwd=str(ROOT), timeout=300)
        assert r.returncode == 0, r.stderr
        lines, summary, human = classify_report(want.total, want.positive, pm.classify_model(want.total, want.positive, frac, hits))
        assert out.read_text().splitlines() == lines + summary
        assert all(h in r.stderr for h in human) and r.stdout == ""
        assert len({ln.split("\t")[-1] for ln in lines}) >= 3  # several indexes and `-` among the answers
    r = subprocess.run(cmd[: -len(extra) - 2] + extra, env=dict(os.environ), capture_output=True, text=True, cwd=str(ROOT), timeout=300)  # without -o: stdout
    assert r.returncode == 0 and r.stdout.splitlines() == lines + summary
