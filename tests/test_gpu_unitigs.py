"""Unitigs on the GPU: the rank of a k-mer (host and device arrays), the compaction table, the unitig text (device buffer, file, descriptor, generator)
and the `unitigs` command. Every expectation comes from the CPU: the oracle's iteration order through tests/unitigs_model.py (the sequential walk that
states the definition), never from the GPU path; every output is pre-filled with 0xA5 and carries pad elements that must keep the fill, so an element
that is not written, or one written too many, shows."""
import os
import random
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd.__main__ import unitigs_report  # noqa: E402
from oracle import Oracle  # noqa: E402
from oracle.pyref import THRESHOLD, PyCBL  # noqa: E402

import neighbors_model as nm  # noqa: E402  (tests/)
import removal_model as rm  # noqa: E402
import unitigs_model as um  # noqa: E402

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
PASS_ENV = "CBLX_NEIGHBOR_PASS"
FILL, PAD = 0xA5, 3
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
SIZES = (0, 1, 7, 8, 9, 31, 32, 33, 255, 256, 257)  # lane-group, wave and workgroup edges at 8 lanes per k-mer
M64 = (1 << 64) - 1
RANK_CONFIGS = nm.CONFIGS + [(9, 4, False)]
TABLE_CONFIGS = [c for c in RANK_CONFIGS if not c[2]]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _set_pass(monkeypatch, value):
    if value is None:
        monkeypatch.delenv(PASS_ENV, raising=False)
    else:
        monkeypatch.setenv(PASS_ENV, str(value))


def _err(g):
    return g._L.cblx_last_error(g._h)


def _split(kmers):
    lo = np.array([x & M64 for x in kmers], dtype=np.uint64)
    hi = np.array([x >> 64 for x in kmers], dtype=np.uint64)
    return lo, hi


# ---- the resident sets and their expectations, once per process ------------------------------------------------------------------------------
_cases = {}


class Case:
    """An index of `batches` (lists of reads, one flush each): the oracle's iteration order and, where the index is not canonical, the model's table
    and text."""

    def __init__(self, k, pb, canonical, batches):
        self.k, self.pb, self.canonical, self.batches = k, pb, canonical, batches
        self.oracle = Oracle(k, pb, canonical)
        for batch in batches:
            self.oracle.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = self.oracle.serialize()
        self.resident = nm.oracle_kmers(self.oracle)  # iteration order
        self.n = len(self.resident)
        if not canonical:
            self.table = um.walk_model(self.resident, k)
            um.check_identities(self.table, self.n)
            self.text = um.text_model(self.resident, self.table, k)

    def index(self):
        """A GPU index with the same batches, each inserted after the one before was built."""
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        for batch in self.batches:
            g.insert_seqs(*nm.Graph.arrays(batch))
            g.flush()
        assert g.serialize() == self.blob
        return g


def _graph_case(k, pb, canonical):
    key = ("graph", k, pb, canonical)
    if key not in _cases:
        graph = nm.Graph(k)
        _cases[key] = Case(k, pb, canonical, [graph.batch1, graph.batch2])
        _cases[key].graph = graph
    return _cases[key]


def _named_case(name):
    if name not in _cases:
        if name.startswith("edges"):
            k = int(name[5:])
            _cases[name] = Case(k, 24 if k == 31 else 16, False, [um.path_edge_reads(k)])
        elif name == "long":
            _cases[name] = Case(31, 24, False, [um.long_path_reads(31)])
        elif name == "dense":
            _cases[name] = Case(9, 4, False, [um.dense_reads()])
        elif name.startswith("branch"):
            k = int(name[6:])
            _cases[name] = Case(k, {15: 6, 31: 24, 33: 16}[k], False, list(um.branch_reads(k)))
    return _cases[name]


# ---- rank ------------------------------------------------------------------------------------------------------------------------------------
def _canon(x, k, canonical):
    return nm.pack(nm.canonical_str(nm.unpack(x, k))) if canonical else x


def _rank_want(order, queries, k, canonical):
    by = {x: i for i, x in enumerate(order)}
    return np.array([by.get(_canon(x, k, canonical), um.RANK_ABSENT) for x in queries], dtype=np.uint64)


def _rank_host_raw(g, kmers, n, with_hi=True, null_out=False):
    lo, hi = _split(kmers[:n])
    buf = np.full(n + PAD, FILL64, dtype=np.uint64)
    rc = cbl_amd.lib().cblx_rank_kmers(g._h, lo.ctypes.data, hi.ctypes.data if with_hi else None, n, None if null_out else buf.ctypes.data)
    return rc, buf


def _rank_device_raw(g, kmers, n, with_hi=True, null_out=False):
    lo, hi = _split(kmers[:n])
    d_lo = torch.from_numpy(lo.view(np.int64)).cuda()
    d_hi = torch.from_numpy(hi.view(np.int64)).cuda()
    d_out = torch.from_numpy(np.full(n + PAD, FILL64, dtype=np.uint64).view(np.int64)).cuda()
    rc = cbl_amd.lib().cblx_rank_kmers_device(g._h, d_lo.data_ptr(), d_hi.data_ptr() if with_hi else None, n, None if null_out else d_out.data_ptr())
    return rc, d_out.cpu().numpy().view(np.uint64)


def _same_rank(got, want, n, what):
    assert got.dtype == np.uint64 and len(got) == n + PAD, what
    bad = np.flatnonzero(got[:n] != want[:n])
    assert not len(bad), f"{what}: rank wrong at (query, got, expected) {[(int(i), int(got[i]), int(want[i])) for i in bad[:8]]}"
    assert (got[n:] == FILL64).all(), f"{what}: the pad elements behind the ranks were written"


def _model_after_removal(cs, gone):
    """The iteration order after n successive CBL::remove calls, by tests/removal_model.py on the buckets of the oracle's index."""
    py = PyCBL(cs.k, cs.pb, cs.canonical)
    sb = py.P["SB"]
    for w in cs.oracle.iter_words():
        py.buckets.setdefault(w >> sb, ["vec", []])[1].append(w & ((1 << sb) - 1))
    for b in py.buckets.values():
        if len(b[1]) > THRESHOLD:
            b[0] = "trie"  # the insert-only rule; a Trie iterates ascending, which is how the oracle gave it
    for x in gone:
        assert rm.remove_word(py, cs.oracle.word_of_kmer(x))
    return [cs.oracle.kmer_of_word((p << sb) | s) for p in sorted(py.buckets) for s in py.buckets[p][1]]


@pytest.mark.parametrize("k,pb,canonical", RANK_CONFIGS)
def test_rank_of_caller_kmers(k, pb, canonical):
    _need_gpu()
    cs = _graph_case(k, pb, canonical)
    g = cs.index()
    q = nm.queries(cs.graph, cs.oracle, canonical)
    want = _rank_want(cs.resident, q, k, canonical)
    assert len(q) > 3000 and 100 < int((want == um.RANK_ABSENT).sum()) < len(q) - 3000  # residents, absent k-mers, duplicates
    per_prefix = {}
    sb = PyCBL(k, pb).P["SB"]
    for w in cs.oracle.iter_words():
        per_prefix[w >> sb] = per_prefix.get(w >> sb, 0) + 1
    assert min(per_prefix.values()) <= THRESHOLD  # Vec buckets; the second flush appended to them (the serialized bytes equal the oracle's)
    if pb == 4:
        assert max(per_prefix.values()) > THRESHOLD  # and Tries
    with_hi_device = k > 31  # K <= 31: the host form is given a zero hi array, the device form none
    for n in SIZES + (len(q),):
        rc, got = _rank_host_raw(g, q, n)
        assert rc == 0, _err(g)
        _same_rank(got, want, n, f"host, n = {n}")
        rc, got = _rank_device_raw(g, q, n, with_hi=with_hi_device)
        assert rc == 0, _err(g)
        _same_rank(got, want, n, f"device, n = {n}")
    # the rank of the residents is 0 .. n - 1: the inverse of the iteration order
    assert np.array_equal(g.rank_np(g.kmers_np()), np.arange(cs.n, dtype=np.uint64))
    assert np.array_equal(g.rank_np(cs.resident), np.arange(cs.n, dtype=np.uint64))
    lo, hi = _split(q[:257])
    d = g.rank_device(torch.from_numpy(lo.view(np.int64)).cuda(), torch.from_numpy(hi.view(np.int64)).cuda() if k > 31 else None, 257)
    assert d.is_cuda and d.dtype == torch.int64 and np.array_equal(d.cpu().numpy().view(np.uint64), want[:257])
    assert cbl_amd.RANK_ABSENT == um.RANK_ABSENT and len(g.rank_np([])) == 0
    # refusals: bits above 2K in the last element; null arguments; n == 0 succeeds whatever the pointers
    bad = list(q[:33])
    bad[32] |= 1 << (2 * k)
    rc, got = _rank_host_raw(g, bad, 33)
    assert rc == cbl_amd.EINVAL and (got == FILL64).all() and b"above 2K" in _err(g)
    rc, got = _rank_device_raw(g, bad, 33)
    assert rc == cbl_amd.EINVAL and (got == FILL64).all()
    rc, _ = _rank_host_raw(g, q, 9, null_out=True)
    assert rc == cbl_amd.EINVAL
    rc, got = _rank_device_raw(g, q, 9, null_out=True)
    assert rc == cbl_amd.EINVAL and (got == FILL64).all()
    if k > 31:
        rc, got = _rank_host_raw(g, q, 9, with_hi=False)
        assert rc == cbl_amd.EINVAL and (got == FILL64).all()
    L = cbl_amd.lib()
    assert L.cblx_rank_kmers(g._h, None, None, 0, None) == 0 and L.cblx_rank_kmers_device(g._h, None, None, 0, None) == 0
    assert g.serialize() == cs.blob and g.validate() == 0  # an observer: Vec buckets as stored, nothing sorted
    # after the removal of a tenth of the residents (swap_remove moves the last word of a Vec bucket into the hole)
    gone = cs.resident[3::10]
    after = _model_after_removal(cs, gone)
    assert len(after) == cs.n - len(gone)
    assert g.remove_kmers(gone).all()
    want = _rank_want(after, q, k, canonical)
    assert int((want == um.RANK_ABSENT).sum()) > 300
    for n in (257, len(q)):
        rc, got = _rank_host_raw(g, q, n)
        assert rc == 0, _err(g)
        _same_rank(got, want, n, f"after the removal, host, n = {n}")
        rc, got = _rank_device_raw(g, q, n, with_hi=with_hi_device)
        assert rc == 0, _err(g)
        _same_rank(got, want, n, f"after the removal, device, n = {n}")
    g.close()
    # an empty index holds nothing
    e = cbl_amd.CBL(k, pb, canonical=canonical)
    for n in (1, 9, 257):
        rc, got = _rank_host_raw(e, q, n)
        assert rc == 0 and (got[:n] == um.RANK_ABSENT).all() and (got[n:] == FILL64).all()
    e.close()


# ---- table and text ----------------------------------------------------------------------------------------------------------------------------
def _table_raw(g, cap_k, cap_u, device, arrays=True):
    """cblx_unitig_table(_device) through the raw ABI on outputs of cap + PAD filled elements: (status, (n, U, circular), dict of the five arrays)."""
    L = cbl_amd.lib()
    counts = [C.c_uint64(12345) for _ in range(3)]
    names = (("unitig", cap_k, np.uint32, FILL32), ("offset", cap_k, np.uint32, FILL32), ("head", cap_u, np.uint32, FILL32), ("length", cap_u, np.uint32, FILL32),
             ("flags", cap_u, np.uint8, FILL))
    host = {name: np.full(cap + PAD, fill, dtype=dt) for name, cap, dt, fill in names}
    if device:
        dev = {name: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in host.items()}
        ptr = {name: t.data_ptr() for name, t in dev.items()}
        fn = L.cblx_unitig_table_device
    else:
        ptr = {name: a.ctypes.data for name, a in host.items()}
        fn = L.cblx_unitig_table
    if not arrays:
        ptr = {name: None for name in ptr}
    rc = fn(g._h, ptr["unitig"], ptr["offset"], cap_k, ptr["head"], ptr["length"], ptr["flags"], cap_u, *[C.byref(c) for c in counts])
    if device:
        host = {name: (t.cpu().numpy().view(np.uint32) if host[name].dtype == np.uint32 else t.cpu().numpy()) for name, t in dev.items()}
    return rc, tuple(c.value for c in counts), host


def _same_table(got, want, n, nu, what):
    for name, m in (("unitig", n), ("offset", n), ("head", nu), ("length", nu), ("flags", nu)):
        a, w = got[name], want[name]
        fill = FILL if name == "flags" else FILL32
        bad = np.flatnonzero(a[:m] != w[:m])
        assert not len(bad), f"{what}: {name} wrong at (index, got, expected) {[(int(i), int(a[i]), int(w[i])) for i in bad[:8]]}"
        assert len(a) >= m + PAD and (a[m:] == fill).all(), f"{what}: elements behind {name} were written"


def _text_device_raw(g, cap):
    d_buf = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    nbytes, nu = C.c_uint64(12345), C.c_uint64(12345)
    rc = cbl_amd.lib().cblx_unitigs_text_device(g._h, d_buf.data_ptr(), cap, C.byref(nbytes), C.byref(nu))
    return rc, nbytes.value, nu.value, d_buf.cpu().numpy()


def _check_index(cs, g, monkeypatch, passes=(None, 256, 7), host_forms=True):
    """Table and text of g against the model of cs at every pass size, the identities on what the device gave, and that nothing changed."""
    n, want, k = cs.n, cs.table, cs.k
    nu, ncirc = len(want["head"]), want["n_circular"]
    blob = g.serialize()
    for p in passes:
        _set_pass(monkeypatch, p)
        rc, counts, got = _table_raw(g, n, nu, device=True)
        assert rc == 0, _err(g)
        assert counts == (n, nu, ncirc), (p, counts)
        _same_table(got, want, n, nu, f"device table, pass {p}")
        trimmed = {name: a[: (n if name in ("unitig", "offset") else nu)] for name, a in got.items()}
        trimmed["n_circular"] = counts[2]
        um.check_identities(trimmed, n, n_simple=want["n_simple"])
        rc, nbytes, u, buf = _text_device_raw(g, len(cs.text))
        assert rc == 0, _err(g)
        assert (nbytes, u) == (len(cs.text), nu) and nbytes == n + nu * k
        assert buf[:nbytes].tobytes() == cs.text, f"device text, pass {p}"
        assert (buf[nbytes:] == FILL).all(), f"pass {p}: bytes behind the text were written"
    _set_pass(monkeypatch, None)
    if host_forms:
        rc, counts, got = _table_raw(g, n + 5, nu + 2, device=False)  # capacities above the need
        assert rc == 0 and counts == (n, nu, ncirc), _err(g)
        _same_table(got, want, n, nu, "host table")
        rc, counts, got = _table_raw(g, 0, 0, device=True, arrays=False)  # null only: counts
        assert rc == 0 and counts == (n, nu, ncirc)
        t = g.unitig_table_np()
        assert um.same_table(t, want) and t["unitig"].dtype == np.uint32 and t["flags"].dtype == np.uint8
        assert g.unitig_counts() == (n, nu, ncirc)
        assert g.unitigs_text_np().tobytes() == cs.text
        assert g.unitigs_text_device() == (len(cs.text), nu)
    assert g.serialize() == blob and g.validate() == 0  # observers: nothing is modified or sorted


def _round_trip(cs, g):
    """The k-mers of the device's text lines, inserted into a fresh index with the same parameters, give the same count() and checksum()."""
    lines = g.unitigs_text_np().tobytes().split(b"\n")[:-1]
    assert all(len(ln) >= cs.k for ln in lines)
    f = cbl_amd.CBL(cs.k, cs.pb, canonical=False)
    if lines:
        f.insert_seqs(*nm.Graph.arrays(lines))
    assert f.count() == g.count() == cs.n and f.checksum() == g.checksum()
    f.close()


@pytest.mark.parametrize("k,pb,canonical", TABLE_CONFIGS)
def test_table_and_text_of_the_neighbour_graph(k, pb, canonical, monkeypatch):
    _need_gpu()
    cs = _graph_case(k, pb, canonical)
    assert cs.table["n_circular"] >= 6  # the input still exercises the cycle path
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    _round_trip(cs, g)
    assert list(g.unitigs()) == cs.text.decode().split("\n")[:-1]
    g.close()


@pytest.mark.parametrize("k", [31, 33])
def test_path_length_edges_and_cycles(k, monkeypatch):
    _need_gpu()
    cs = _named_case(f"edges{k}")
    lengths = cs.table["length"].tolist()
    assert all(ln in lengths for ln in um.PATH_LENGTHS) and sorted(cs.table["length"][cs.table["flags"] == 1].tolist()) == sorted(um.CYCLE_LENGTHS)
    assert 200 in lengths  # the cycle with a read running into it came out linear
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    _round_trip(cs, g)
    g.close()


def test_one_path_of_70000_kmers(monkeypatch):
    _need_gpu()
    cs = _named_case("long")
    assert cs.n == 70000 and len(cs.table["head"]) == 1
    g = cs.index()
    _check_index(cs, g, monkeypatch, passes=(None, 256))
    _check_index(cs, g, monkeypatch, passes=(7,), host_forms=False)
    _round_trip(cs, g)
    g.close()


def test_dense_graph_of_tries(monkeypatch):
    _need_gpu()
    cs = _named_case("dense")
    assert cs.n > 30000 and len(cs.table["head"]) > 10000
    g = cs.index()
    _, length, kind = g.bucket_table_np()
    # Tries hold nearly every k-mer: necklaces begin with their smallest rotation, so the few k-mers of the high prefixes stay in Vec buckets
    assert int((kind == 1).sum()) >= 4 and (length[kind == 1] > THRESHOLD).all() and int(length[kind == 1].sum()) > 0.95 * cs.n
    _check_index(cs, g, monkeypatch, passes=(None, 256))
    _check_index(cs, g, monkeypatch, passes=(7,), host_forms=False)
    _round_trip(cs, g)
    g.close()


@pytest.mark.parametrize("k", [15, 31, 33])
def test_edge_cases(k, monkeypatch):
    _need_gpu()
    pb = {15: 6, 31: 24, 33: 16}[k]
    # the empty index: U = 0, nothing written, an empty file
    e = cbl_amd.CBL(k, pb)
    for device in (True, False):
        rc, counts, got = _table_raw(e, 4, 4, device=device)
        assert rc == 0 and counts == (0, 0, 0)
        assert all((a == (FILL if name == "flags" else FILL32)).all() for name, a in got.items())
    rc, nbytes, u, buf = _text_device_raw(e, 8)
    assert rc == 0 and (nbytes, u) == (0, 0) and (buf == FILL).all()
    assert len(e.unitigs_text_np()) == 0 and list(e.unitigs()) == [] and e.unitig_table_np()["n_circular"] == 0 and len(e.unitig_table_np()["head"]) == 0
    e.close()
    # one k-mer; poly-A alone (a circular unitig of length 1); a branch read inserted in a second flush into the middle of a path
    lone = nm._rand(random.Random(k), k).encode()
    for key, batches in ((f"lone{k}", [[lone]]), (f"polyA{k}", [[b"A" * k]])):
        if key not in _cases:
            _cases[key] = Case(k, pb, False, batches)
        cs = _cases[key]
        assert cs.n == 1 and len(cs.text) == k + 1 and cs.table["n_circular"] == (1 if key.startswith("polyA") else 0)
        g = cs.index()
        _check_index(cs, g, monkeypatch)
        _round_trip(cs, g)
        g.close()
    cs = _named_case(f"branch{k}")
    assert sorted(cs.table["length"].tolist()) == [21, 149, 151]
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    _round_trip(cs, g)
    g.close()


# ---- refusals, files, the command line ---------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(tmp_path):
    _need_gpu()
    k, pb = 31, 24
    cs = _graph_case(k, pb, False)
    n, nu, ncirc = cs.n, len(cs.table["head"]), cs.table["n_circular"]
    g = cs.index()
    for device in (True, False):
        for cap_k, cap_u in ((n - 1, nu), (n, nu - 1), (0, 0)):
            rc, counts, got = _table_raw(g, cap_k, cap_u, device=device)
            assert rc == cbl_amd.ERANGE and counts == (n, nu, ncirc), (device, cap_k, cap_u)  # the need is reported
            assert all((a == (FILL if name == "flags" else FILL32)).all() for name, a in got.items()), "a refused call wrote"
    rc, nbytes, u, buf = _text_device_raw(g, len(cs.text) - 1)
    assert rc == cbl_amd.ERANGE and (nbytes, u) == (len(cs.text), nu) and (buf == FILL).all()
    # a descriptor that cannot be written to: the rule of list_to_fd
    fd = os.open(tmp_path / "ro.txt", os.O_RDONLY | os.O_CREAT, 0o644)
    try:
        with pytest.raises(cbl_amd.CblxError) as e:
            g.unitigs_to_fd(fd, 100)
    finally:
        os.close(fd)
    assert e.value.code == cbl_amd.EINVAL and "Failed to write the unitigs" in str(e.value)
    # a closed descriptor: a number far above the ones in use, so that nothing opened meanwhile can take it
    closed = 500
    fd_source = os.open(tmp_path / "ro.txt", os.O_RDONLY)
    os.dup2(fd_source, closed)
    os.close(fd_source)
    os.close(closed)
    with pytest.raises(cbl_amd.CblxError) as e:
        g.unitigs_to_fd(closed, 100)
    assert e.value.code == cbl_amd.EINVAL and "Failed to write the unitigs" in str(e.value)
    with pytest.raises(cbl_amd.CblxError) as e:
        g.unitigs_to_fd(-1)
    assert e.value.code == cbl_amd.EINVAL
    with pytest.raises(cbl_amd.CblxError):
        g.unitigs_to_file(tmp_path / "no" / "such" / "dir.txt")
    assert g.unitigs_text_np().tobytes() == cs.text and g.serialize() == cs.blob  # the index still answers
    g.close()
    # a canonical index: bidirected unitigs are not built
    cc = _graph_case(k, pb, True)
    c = cc.index()
    for device in (True, False):
        rc, counts, got = _table_raw(c, cc.n, cc.n, device=device)
        assert rc == cbl_amd.EINVAL and b"canonical" in _err(c) and counts == (12345, 12345, 12345)
        assert all((a == (FILL if name == "flags" else FILL32)).all() for name, a in got.items())
    rc, nbytes, u, buf = _text_device_raw(c, 64)
    assert rc == cbl_amd.EINVAL and (buf == FILL).all()
    with pytest.raises(cbl_amd.CblxError) as e:
        c.unitigs_to_file(tmp_path / "canonical.txt")
    assert e.value.code == cbl_amd.EINVAL
    assert not (tmp_path / "canonical.txt").exists()  # the refusal comes before the file is created ...
    (tmp_path / "kept.txt").write_bytes(b"kept\n")
    with pytest.raises(cbl_amd.CblxError) as e:
        c.unitigs_to_file(tmp_path / "kept.txt")
    assert e.value.code == cbl_amd.EINVAL and b"canonical" in _err(c)
    assert (tmp_path / "kept.txt").read_bytes() == b"kept\n"  # ... or truncated
    assert c.serialize() == cc.blob
    c.close()


@pytest.mark.parametrize("name", ["graph", "edges31"])
def test_unitigs_to_file_and_fd(name, tmp_path):
    _need_gpu()
    cs = _graph_case(33, 16, False) if name == "graph" else _named_case(name)
    g = cs.index()
    nu = len(cs.table["head"])
    for chunk in (5, 0):  # a chunk smaller than one line; the default
        path = tmp_path / f"unitigs-{chunk}.txt"
        assert g.unitigs_to_file(path, chunk) == (nu, len(cs.text))
        data = path.read_bytes()
        assert data == cs.text and data == g.unitigs_text_np().tobytes()
    r, w = os.pipe()
    got = []

    def reader():
        with os.fdopen(r, "rb") as f:
            got.append(f.read())

    t = threading.Thread(target=reader)
    t.start()
    try:
        res = g.unitigs_to_fd(w, 1000)
    finally:
        os.close(w)
        t.join()
    assert res == (nu, len(cs.text)) and got[0] == cs.text
    assert g.serialize() == cs.blob
    g.close()


def test_cli_unitigs(tmp_path):
    _need_gpu()
    k, pb = 31, 24
    cs = _graph_case(k, pb, False)
    path = tmp_path / "index.cbl"
    path.write_bytes(cs.blob)
    base = [sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb), "unitigs", str(path)]
    r = subprocess.run(base, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == cs.text
    out = tmp_path / "unitigs.txt"
    r = subprocess.run(base + ["-o", str(out)], env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == cs.text
    lines, human = unitigs_report(um.summary_model(cs.table["length"], cs.table["flags"], k))
    r = subprocess.run(base + ["--stats"], env=dict(os.environ), capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == lines and all(h in r.stderr for h in human)
