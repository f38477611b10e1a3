"""De Bruijn neighbourhoods on the GPU: neighbour masks of caller k-mers (host and device arrays), of ranges of the iteration order, and the degree table,
by the per-query route (k_contains) and by the join forced for every pass. Every expectation comes from the CPU oracle through tests/neighbors_model.py
(eight Oracle.contains_kmer calls per k-mer), never from the GPU path; every output is pre-filled with 0xA5 and carries three pad bytes that must keep
the fill, so a byte that is not written, or one written too many, shows."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd.__main__ import graph_report  # noqa: E402
from oracle import Oracle  # noqa: E402

import neighbors_model as nm  # noqa: E402  (tests/)

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
JOIN_ENV, PASS_ENV = "CBLX_QUERY_JOIN_MIN", "CBLX_NEIGHBOR_PASS"
FILL, PAD = 0xA5, 3
SIZES = (0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257)  # lane-group, wave and workgroup edges at 8 lanes per k-mer
M64 = (1 << 64) - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _routes(monkeypatch):
    """The per-query route (small passes), then the join forced for every pass. Where the join does not apply the forced setting must give the same bytes."""
    monkeypatch.delenv(PASS_ENV, raising=False)
    for join in (None, "1"):
        if join is None:
            monkeypatch.delenv(JOIN_ENV, raising=False)
        else:
            monkeypatch.setenv(JOIN_ENV, join)
        yield "join" if join else "per-query"
    monkeypatch.delenv(JOIN_ENV, raising=False)


def _set_pass(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(PASS_ENV, raising=False)
    else:
        monkeypatch.setenv(PASS_ENV, str(value))


# ---- the resident sets and their expectations, once per process ------------------------------------------------------------------------------
_cases = {}


class Case:
    def __init__(self, k, pb, canonical):
        self.k, self.pb, self.canonical = k, pb, canonical
        self.graph = nm.Graph(k)
        self.oracle = Oracle(k, pb, canonical)
        for batch in (self.graph.batch1, self.graph.batch2):
            self.oracle.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = self.oracle.serialize()
        self.resident = nm.oracle_kmers(self.oracle)                              # iteration order
        self.resident_masks = nm.masks_model(self.oracle, self.resident, k)
        self.queries = nm.queries(self.graph, self.oracle, canonical)
        self.query_masks = nm.masks_model(self.oracle, self.queries, k)
        self.table = nm.table_model(self.resident_masks)

    def index(self):
        """A GPU index with the same two batches, the second inserted after the first was built."""
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        for batch in (self.graph.batch1, self.graph.batch2):
            g.insert_seqs(*nm.Graph.arrays(batch))
            g.flush()
        assert g.serialize() == self.blob
        return g


def _case(k, pb, canonical):
    key = (k, pb, canonical)
    if key not in _cases:
        _cases[key] = Case(k, pb, canonical)
    return _cases[key]


def _split(kmers):
    lo = np.array([x & M64 for x in kmers], dtype=np.uint64)
    hi = np.array([x >> 64 for x in kmers], dtype=np.uint64)
    return lo, hi


def _filled(n):
    return np.full(n + PAD, FILL, dtype=np.uint8)


def _host_raw(g, kmers, n, with_hi=True, out="fill"):
    """cblx_neighbors_kmers on the first n of `kmers` through the raw ABI: (status, output of n + PAD bytes)."""
    lo, hi = _split(kmers[:n])
    buf = _filled(n) if isinstance(out, str) else out
    rc = cbl_amd.lib().cblx_neighbors_kmers(g._h, lo.ctypes.data, hi.ctypes.data if with_hi else None, n, None if buf is None else buf.ctypes.data)
    return rc, buf


def _device_raw(g, kmers, n, with_hi=True, null_out=False):
    lo, hi = _split(kmers[:n])
    d_lo = torch.from_numpy(lo.view(np.int64)).cuda()
    d_hi = torch.from_numpy(hi.view(np.int64)).cuda()
    d_out = torch.full((n + PAD,), FILL, dtype=torch.uint8, device="cuda")
    rc = cbl_amd.lib().cblx_neighbors_kmers_device(g._h, d_lo.data_ptr(), d_hi.data_ptr() if with_hi else None, n, None if null_out else d_out.data_ptr())
    return rc, d_out.cpu().numpy()


def _same(got, want, n, what):
    assert got.dtype == np.uint8 and len(got) == n + PAD, what
    bad = np.flatnonzero(got[:n] != want[:n])
    assert not len(bad), f"{what}: mask wrong at (k-mer, got, expected) {[(int(i), hex(int(got[i])), hex(int(want[i]))) for i in bad[:8]]}"
    assert (got[n:] == FILL).all(), f"{what}: the pad bytes behind the masks were written"


def _range_raw(g, first, n, cap):
    """cblx_neighbors_range and its device form: (status, written, output of cap + PAD bytes) each."""
    out = []
    L = cbl_amd.lib()
    buf, got = _filled(cap), C.c_uint64(12345)
    rc = L.cblx_neighbors_range(g._h, first, n, buf.ctypes.data, C.byref(got))
    out.append((rc, got.value, buf))
    d_buf, got = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda"), C.c_uint64(12345)
    rc = L.cblx_neighbors_range_device(g._h, first, n, d_buf.data_ptr(), C.byref(got))
    out.append((rc, got.value, d_buf.cpu().numpy()))
    return out


# ---- 1. caller k-mers, every config, both routes ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", nm.CONFIGS)
def test_masks_of_caller_kmers(k, pb, canonical, monkeypatch):
    _need_gpu()
    cs = _case(k, pb, canonical)
    g = cs.index()
    q, want = cs.queries, cs.query_masks
    assert len(q) > 3000 and 0 < int((want == 0).sum()) < len(q) and len(set(want.tolist())) > 8  # hits, misses and many different masks
    with_hi_device = k > 31  # K <= 31: the host form is given a zero hi array, the device form none
    for how in _routes(monkeypatch):
        for n in SIZES + (len(q),):
            rc, got = _host_raw(g, q, n)
            assert rc == 0, g._L.cblx_last_error(g._h)
            _same(got, want, n, f"host, n = {n}, {how}")
            rc, got = _device_raw(g, q, n, with_hi=with_hi_device)
            assert rc == 0, g._L.cblx_last_error(g._h)
            _same(got, want, n, f"device, n = {n}, {how}")
        # the Python surface; and the route: the join sends its 8 n tagged records through the partition passes, the per-query route sends nothing
        moved = g.stage_units()["radix_scatter"]
        assert np.array_equal(g.neighbors_np(q[:257]), want[:257]), how
        moved = g.stage_units()["radix_scatter"] - moved
        cn = g.consts()
        joins = how == "join" and cn["word_bits"] <= 96 and cn["suffix_bits"] <= 64
        assert (moved >= 8 * 257 and moved % (8 * 257) == 0) if joins else moved == 0, (how, moved)
        lo, hi = _split(q[:257])
        d = g.neighbors_device(torch.from_numpy(lo.view(np.int64)).cuda(), torch.from_numpy(hi.view(np.int64)).cuda(), 257)
        assert d.is_cuda and d.dtype == torch.uint8 and np.array_equal(d.cpu().numpy(), want[:257]), how
        # 2. the pass size does not show: one k-mer, five and thirty-two per pass on 33 k-mers
        for p in (1, 5, 32):
            _set_pass(monkeypatch, p)
            rc, got = _host_raw(g, q, 33)
            assert rc == 0
            _same(got, want, 33, f"pass = {p}, {how}")
            rc, got = _device_raw(g, q, 33, with_hi=with_hi_device)
            assert rc == 0
            _same(got, want, 33, f"device, pass = {p}, {how}")
        _set_pass(monkeypatch, None)
    assert g.serialize() == cs.blob and g.validate() == 0  # an observer: Vec buckets as stored, nothing sorted
    g.close()


# ---- 3. ranges of the iteration order --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", nm.CONFIGS)
def test_masks_of_ranges(k, pb, canonical, monkeypatch):
    _need_gpu()
    cs = _case(k, pb, canonical)
    g = cs.index()
    count, want = len(cs.resident), cs.resident_masks
    assert g.count() == count
    lo, hi = g.kmers_np()
    assert (lo.tolist() if hi is None else [a | (b << 64) for a, b in zip(lo.tolist(), hi.tolist())]) == cs.resident
    _, length, _ = g.bucket_table_np()
    starts = np.concatenate([[0], np.cumsum(length.astype(np.int64))])
    b = int(np.argmax(length[1:-1])) + 1 if len(length) > 2 else 0  # an inner bucket of several elements where there is one
    s0, ln = int(starts[b]), int(length[b])
    windows = [(0, None), (0, 1), (count - 1, 1), (s0, ln), (s0 + ln - 1, 2), (max(s0 - 1, 0), 3), (s0, 1), (s0 + ln - 1, 1), (count // 3, 300), (count - 5, 100)]
    L = cbl_amd.lib()
    for how in _routes(monkeypatch):
        for pass_ in (None, 64):
            _set_pass(monkeypatch, pass_)
            for first, n in windows:
                m = min(count - first, count if n is None else n)
                got = g.neighbors_range_np(first, n)
                assert len(got) == m and np.array_equal(got, want[first: first + m]), (how, pass_, first, n)
                assert np.array_equal(got, g.neighbors_np(g.kmers_np(first, n))), (how, pass_, first, n)
                for rc, written, buf in _range_raw(g, first, count + 7 if n is None else n, m):
                    assert rc == 0 and written == m, (how, first, n)
                    _same(buf, want[first:], m, f"range ({first}, {n}), pass {pass_}, {how}")
        _set_pass(monkeypatch, None)
        # first == count: nothing written; first > count: refused as export_kmers_range refuses it, the output untouched
        for rc, written, buf in _range_raw(g, count, 1, 4):
            assert rc == 0 and written == 0 and (buf == FILL).all(), how
        for rc, written, buf in _range_raw(g, 0, 0, 4):
            assert rc == 0 and written == 0 and (buf == FILL).all(), how
        klo, got = np.zeros(4, dtype=np.uint64), C.c_uint64(12345)
        refused = L.cblx_export_kmers_range(g._h, count + 1, 1, klo.ctypes.data, klo.ctypes.data, C.byref(got))
        assert refused == cbl_amd.EINVAL
        for rc, written, buf in _range_raw(g, count + 1, 1, 4):
            assert rc == refused and written == 12345 and (buf == FILL).all(), how
        assert L.cblx_neighbors_range(g._h, 0, 4, None, None) == cbl_amd.EINVAL and L.cblx_neighbors_range_device(g._h, 0, 4, None, None) == cbl_amd.EINVAL
        d = torch.full((10,), FILL, dtype=torch.uint8, device="cuda")
        assert g.neighbors_range_device(count - 4, 10, d) == 4 and d.cpu().numpy().tolist() == want[count - 4:].tolist() + [FILL] * 6
    assert g.serialize() == cs.blob and g.validate() == 0
    g.close()


# ---- 4. the degree table ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", nm.CONFIGS)
def test_degree_table(k, pb, canonical, monkeypatch):
    _need_gpu()
    cs = _case(k, pb, canonical)
    g = cs.index()
    count = len(cs.resident)
    assert int(cs.table.sum()) == count and int((cs.table > 0).sum()) >= 5  # simple paths and loops, sources, sinks, the fork, the join
    for how in _routes(monkeypatch):
        for p in (None, 1, 7, count):
            _set_pass(monkeypatch, p)
            t = g.degree_table()
            assert t.dtype == np.uint64 and t.shape == (5, 5), (how, p)
            assert np.array_equal(t, cs.table), f"pass {p}, {how}: got {t.tolist()}, expected {cs.table.tolist()}"
            assert int(t.sum()) == g.count()
        _set_pass(monkeypatch, None)
    s = cbl_amd.CBL.degree_summary(g.degree_table())
    assert s["nodes"] == count
    if not canonical:
        assert s["out_edges"] == s["in_edges"]  # every edge is seen once from each end
    assert cbl_amd.lib().cblx_degree_table(g._h, None) == cbl_amd.EINVAL
    assert g.serialize() == cs.blob and g.validate() == 0
    g.close()


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", [(15, 6, False), (31, 24, True), (33, 16, False), (59, 28, True)])
def test_refusals_write_nothing(k, pb, canonical, monkeypatch):
    _need_gpu()
    cs = _case(k, pb, canonical)
    g = cs.index()
    q = list(cs.queries[:33])
    q[16] |= 1 << (2 * k)  # one bit above 2K, in the middle of the batch
    variants = [q]
    if k <= 31:
        high = list(cs.queries[:33])
        high[20] |= 1 << 64  # K <= 31 with a hi array that is not zero
        variants.append(high)
    for how in _routes(monkeypatch):
        for p in (None, 5):  # several passes: the k-mer is refused before the first pass writes
            _set_pass(monkeypatch, p)
            for v in variants:
                rc, got = _host_raw(g, v, 33)
                assert rc == cbl_amd.EINVAL and (got == FILL).all(), (how, p)
                assert b"above 2K" in g._L.cblx_last_error(g._h)
                rc, got = _device_raw(g, v, 33)
                assert rc == cbl_amd.EINVAL and (got == FILL).all(), (how, p)
            with pytest.raises(cbl_amd.CblxError) as e:
                g.neighbors_np(q)
            assert e.value.code == cbl_amd.EINVAL
        _set_pass(monkeypatch, None)
        # a null output, null k-mers
        rc, _ = _host_raw(g, cs.queries, 9, out=None)
        assert rc == cbl_amd.EINVAL
        rc, got = _device_raw(g, cs.queries, 9, null_out=True)
        assert rc == cbl_amd.EINVAL and (got == FILL).all()
        buf = _filled(9)
        assert cbl_amd.lib().cblx_neighbors_kmers(g._h, None, None, 9, buf.ctypes.data) == cbl_amd.EINVAL and (buf == FILL).all()
        if k > 31:  # K >= 33 needs the hi halves
            rc, got = _host_raw(g, cs.queries, 9, with_hi=False)
            assert rc == cbl_amd.EINVAL and (got == FILL).all()
        # n == 0 succeeds and writes nothing, whatever the pointers
        assert cbl_amd.lib().cblx_neighbors_kmers(g._h, None, None, 0, None) == 0 and cbl_amd.lib().cblx_neighbors_kmers_device(g._h, None, None, 0, None) == 0
    assert len(g.neighbors_np([])) == 0
    assert g.serialize() == cs.blob
    g.close()


# ---- 6. an observer that sees pending inserts; 7. an empty index; the index that holds s alone -----------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", [(31, 24, False), (15, 6, True), (33, 16, True), (45, 6, False)])
def test_pending_inserts_empty_index_and_lone_kmer(k, pb, canonical, monkeypatch):
    _need_gpu()
    cs = _case(k, pb, canonical)
    late = cs.graph.late
    o = Oracle(k, pb, canonical)
    o.load(cs.blob)
    o.insert_seq(late)
    late_kmers = [nm.pack(late.decode()[i: i + k]) for i in range(len(late) - k + 1)]
    q = late_kmers + list(cs.queries[:200])
    want = nm.masks_model(o, q, k)
    assert not np.array_equal(want, nm.masks_model(cs.oracle, q, k))  # the read changes the answer
    s = nm.pack(cs.graph.ring)
    alone_o = Oracle(k, pb, canonical)
    alone_o.insert_kmer(s)
    ring_q = [s] + [nm.pack(cs.graph.ring[i:] + cs.graph.ring[:i]) for i in range(1, k)]
    ring_want = nm.masks_model(alone_o, ring_q, k)
    for how in _routes(monkeypatch):
        g = cs.index()
        g.insert_seq(late)  # enqueued, not flushed
        rc, got = _host_raw(g, q, len(q))
        assert rc == 0
        _same(got, want, len(q), f"pending insert, {how}")
        assert g.serialize() == o.serialize()
        assert np.array_equal(g.degree_table(), nm.table_model(nm.masks_model(o, nm.oracle_kmers(o), k))), how
        assert g.serialize() == o.serialize()
        g.close()
        # an empty index: zero masks for any queries, a zero table, an empty range
        e = cbl_amd.CBL(k, pb, canonical=canonical)
        for n in (1, 9, 257):
            rc, got = _host_raw(e, cs.queries, n)
            assert rc == 0 and (got[:n] == 0).all() and (got[n:] == FILL).all(), (how, n)
            rc, got = _device_raw(e, cs.queries, n)
            assert rc == 0 and (got[:n] == 0).all() and (got[n:] == FILL).all(), (how, n)
        assert not e.degree_table().any() and len(e.neighbors_range_np()) == 0
        for rc, written, buf in _range_raw(e, 0, 5, 5):
            assert rc == 0 and written == 0 and (buf == FILL).all()
        assert e.successors(s) == [] and e.predecessors(s) == [] and e.count() == 0
        e.close()
        # an index that holds s alone: its rotations share its necklace at other positions, and none of them is held
        a = cbl_amd.CBL(k, pb, canonical=canonical)
        assert a.insert_kmers([s]).tolist() == [True]
        assert np.array_equal(a.neighbors_np(ring_q), ring_want), how
        if not canonical:
            assert not a.neighbors_np(ring_q)[0] and a.successors(s) == []
        assert np.array_equal(a.degree_table(), nm.table_model(nm.masks_model(alone_o, nm.oracle_kmers(alone_o), k))) and a.serialize() == alone_o.serialize()
        a.close()


# ---- 8. successors and predecessors ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", [(15, 6, False), (31, 24, True), (33, 16, False), (59, 28, True)])
def test_successors_and_predecessors(k, pb, canonical):
    _need_gpu()
    cs = _case(k, pb, canonical)
    g = cs.index()
    fork, join = nm.pack(cs.graph.fork), nm.pack(cs.graph.join)
    assert g.successors(fork) == [nm.append(fork, c, k) for c in range(4)]
    assert g.predecessors(join) == [nm.prepend(join, c, k) for c in range(4)]
    for x in (fork, join, nm.pack(cs.graph.ring), nm.pack(cs.graph.dinuc), 0, (1 << (2 * k)) - 1, cs.queries[1]):
        m = nm.mask_model(cs.oracle, x, k)
        nb = nm.neighbors(x, k)
        assert g.successors(x) == [nb[c] for c in range(4) if (m >> c) & 1], hex(x)
        assert g.predecessors(x) == [nb[4 + c] for c in range(4) if (m >> (4 + c)) & 1], hex(x)
    assert 0 in g.successors(0) and 0 in g.predecessors(0)  # poly-A: a self-loop
    g.close()


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------------
def test_cli_graph(tmp_path):
    _need_gpu()
    k, pb, canonical = 31, 24, True
    cs = _case(k, pb, canonical)
    path = tmp_path / "index.cbl"
    path.write_bytes(cs.blob)
    g = cbl_amd.CBL.load_from_file(str(path), k, pb)
    table = g.degree_table()
    g.close()
    assert np.array_equal(table, cs.table)
    lines, summary, human = graph_report(cs.table)
    cmd = [sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb), "graph", str(path)]
    r = subprocess.run(cmd, env=dict(os.environ), capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == lines + summary
    assert all(h in r.stderr for h in human)
