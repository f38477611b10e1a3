"""Bidirected unitigs on the GPU: the compaction table with `reversed` (host and device arrays), the text (device buffer, file, descriptor, generator) and
the `unitigs` command on a canonical index. Every expectation comes from the CPU: the oracle's iteration order through tests/biunitigs_model.py (the
sequential walk over oriented k-mers that states the definition), never from the GPU path; every output is pre-filled with 0xA5 and carries pad elements
that must keep the fill, so an element that is not written, or one written too many, shows."""
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

import biunitigs_model as bm  # noqa: E402  (tests/)
import neighbors_model as nm  # noqa: E402
import unitigs_model as um  # noqa: E402

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
PASS_ENV = "CBLX_NEIGHBOR_PASS"
PASSES = (None, 64, 1000)  # the default (one pass); several passes with a ragged last one
FILL, PAD = 0xA5, 3
FILL32 = 0xA5A5A5A5
ARRAYS = (("unitig", "k", np.uint32), ("offset", "k", np.uint32), ("reversed", "k", np.uint8), ("head", "u", np.uint32), ("length", "u", np.uint32), ("flags", "u", np.uint8))


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


def _fill(dt):
    return FILL if dt == np.uint8 else FILL32


# ---- the resident sets and their expectations, once per process ------------------------------------------------------------------------------
_cases = {}


class Case:
    """A canonical index of `batches` (lists of reads, one flush each): the oracle's iteration order, the model's table and text."""

    def __init__(self, k, pb, batches, canonical=True):
        self.k, self.pb, self.batches, self.canonical = k, pb, batches, canonical
        self.oracle = Oracle(k, pb, canonical)
        for batch in batches:
            self.oracle.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = self.oracle.serialize()
        self.resident = nm.oracle_kmers(self.oracle)
        self.n = len(self.resident)
        if canonical:
            self.table = bm.walk_model(self.resident, k)
            bm.check_identities(self.table, self.n)
            self.text = bm.text_model(self.resident, self.table, k)

    def index(self):
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        for batch in self.batches:
            g.insert_seqs(*nm.Graph.arrays(batch))
            g.flush()
        assert g.serialize() == self.blob
        return g


def _case(name):
    if name not in _cases:
        if name == "long":
            _cases[name] = Case(31, 24, [um.long_path_reads(31)])
        elif name.startswith("lone"):
            k = int(name[4:])
            _cases[name] = Case(k, {15: 6, 31: 24, 33: 16}[k], [[nm._rand(random.Random(k), k).encode()]])
        else:
            _cases[name] = Case(*bm.crafted(name))
    return _cases[name]


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------------------
def _table_raw(g, cap_k, cap_u, device, arrays=True):
    """cblx_biunitig_table(_device) through the raw ABI on outputs of cap + PAD filled elements: (status, (n, U, circular), dict of the six arrays)."""
    L = cbl_amd.lib()
    counts = [C.c_uint64(12345) for _ in range(3)]
    host = {name: np.full((cap_k if per == "k" else cap_u) + PAD, _fill(dt), dtype=dt) for name, per, dt in ARRAYS}
    if device:
        dev = {name: torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda() for name, a in host.items()}
        ptr = {name: t.data_ptr() for name, t in dev.items()}
        fn = L.cblx_biunitig_table_device
    else:
        ptr = {name: a.ctypes.data for name, a in host.items()}
        fn = L.cblx_biunitig_table
    if not arrays:
        ptr = {name: None for name in ptr}
    rc = fn(g._h, ptr["unitig"], ptr["offset"], ptr["reversed"], cap_k, ptr["head"], ptr["length"], ptr["flags"], cap_u, *[C.byref(c) for c in counts])
    if device:
        host = {name: (t.cpu().numpy().view(np.uint32) if host[name].dtype == np.uint32 else t.cpu().numpy()) for name, t in dev.items()}
    return rc, tuple(c.value for c in counts), host


def _untouched(got):
    return all((a == _fill(a.dtype)).all() for a in got.values())


def _same_table(got, want, n, nu, what):
    for name, per, dt in ARRAYS:
        m = n if per == "k" else nu
        a, w = got[name], want[name]
        bad = np.flatnonzero(a[:m] != w[:m])
        assert not len(bad), f"{what}: {name} wrong at (index, got, expected) {[(int(i), int(a[i]), int(w[i])) for i in bad[:8]]}"
        assert len(a) >= m + PAD and (a[m:] == _fill(dt)).all(), f"{what}: elements behind {name} were written"


def _text_device_raw(g, cap):
    d_buf = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    nbytes, nu = C.c_uint64(12345), C.c_uint64(12345)
    rc = cbl_amd.lib().cblx_biunitigs_text_device(g._h, d_buf.data_ptr(), cap, C.byref(nbytes), C.byref(nu))
    return rc, nbytes.value, nu.value, d_buf.cpu().numpy()


def _check_index(cs, g, monkeypatch, passes=PASSES):
    """Table, `reversed` and text of g byte-equal to the model of cs at every pass size, host and device forms, the identities on what the device gave,
    and serialize() unchanged afterwards."""
    n, want, k = cs.n, cs.table, cs.k
    nu, ncirc = len(want["head"]), want["n_circular"]
    for p in passes:
        _set_pass(monkeypatch, p)
        rc, counts, got = _table_raw(g, n, nu, device=True)
        assert rc == 0, _err(g)
        assert counts == (n, nu, ncirc), (p, counts)
        _same_table(got, want, n, nu, f"device table, pass {p}")
        trimmed = {name: got[name][: (n if per == "k" else nu)] for name, per, _ in ARRAYS}
        trimmed["n_circular"] = counts[2]
        bm.check_identities(trimmed, n, n_simple=want["n_simple"])
        rc, nbytes, u, buf = _text_device_raw(g, len(cs.text))
        assert rc == 0, _err(g)
        assert (nbytes, u) == (len(cs.text), nu) and nbytes == n + nu * k
        assert buf[:nbytes].tobytes() == cs.text, f"device text, pass {p}"
        assert (buf[nbytes:] == FILL).all(), f"pass {p}: bytes behind the text were written"
    _set_pass(monkeypatch, None)
    rc, counts, got = _table_raw(g, n + 5, nu + 2, device=False)  # capacities above the need
    assert rc == 0 and counts == (n, nu, ncirc), _err(g)
    _same_table(got, want, n, nu, "host table")
    for device in (True, False):
        rc, counts, got = _table_raw(g, 0, 0, device=device, arrays=False)  # null only: counts
        assert rc == 0 and counts == (n, nu, ncirc)
    t = g.biunitig_table_np()
    assert bm.same_table(t, want) and t["unitig"].dtype == np.uint32 and t["reversed"].dtype == np.uint8 and t["flags"].dtype == np.uint8
    d = g.biunitig_table_device()
    assert all(d[name].is_cuda for name, _, _ in ARRAYS) and d["n_circular"] == ncirc
    assert all(np.array_equal(d[name].cpu().numpy().view(dt), want[name]) for name, _, dt in ARRAYS)
    assert g.biunitig_counts() == (n, nu, ncirc)
    assert g.biunitigs_text_np().tobytes() == cs.text
    assert g.biunitigs_text_device() == (len(cs.text), nu)
    assert list(g.biunitigs()) == cs.text.decode().split("\n")[:-1]
    assert cbl_amd.CBL.unitig_summary(t["length"], t["flags"], k) == um.summary_model(want["length"], want["flags"], k)
    assert g.serialize() == cs.blob and g.validate() == 0  # observers: nothing is modified or sorted


def _round_trip(cs, g):
    """The lines of the device's text, inserted into a fresh canonical index with the same parameters, give the same count() and checksum()."""
    lines = g.biunitigs_text_np().tobytes().split(b"\n")[:-1]
    assert all(len(ln) >= cs.k for ln in lines)
    f = cbl_amd.CBL(cs.k, cs.pb, canonical=True)
    if lines:
        f.insert_seqs(*nm.Graph.arrays(lines))
    assert f.count() == g.count() == cs.n and f.checksum() == g.checksum()
    f.close()


# ---- table and text ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bm.CRAFTED)
def test_table_reversed_and_text(name, monkeypatch):
    _need_gpu()
    cs = _case(name)
    if name.startswith("graph"):
        assert 3000 < cs.n < 4500 and cs.table["n_circular"] >= 2  # the rotation ring and the dinucleotide pair stay circular; the homopolymers do not
    if name.startswith("edges"):
        lengths = cs.table["length"].tolist()
        assert all(ln in lengths for ln in um.PATH_LENGTHS) and sorted(cs.table["length"][cs.table["flags"] == 1].tolist()) == sorted(um.CYCLE_LENGTHS)
        assert 200 in lengths  # the cycle with a read running into it came out linear
    if name == "dense":
        assert cs.n > 30000 and len(cs.table["head"]) > 10000
    if name == "overlap":
        assert len(cs.table["head"]) == 1 and 0 < int(cs.table["reversed"].sum()) < cs.n
    if name in ("homopolymers", "at"):
        assert cs.table["n_circular"] == 0 and (cs.table["length"] == 1).all()
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    _round_trip(cs, g)
    g.close()


def test_one_path_of_70000_kmers(monkeypatch):
    _need_gpu()
    cs = _case("long")
    assert cs.n == 70000 and len(cs.table["head"]) == 1
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    _round_trip(cs, g)
    g.close()


@pytest.mark.parametrize("k", [15, 31, 33])
def test_empty_index_and_one_kmer(k, monkeypatch):
    _need_gpu()
    pb = {15: 6, 31: 24, 33: 16}[k]
    e = cbl_amd.CBL(k, pb, canonical=True)
    for device in (True, False):
        rc, counts, got = _table_raw(e, 4, 4, device=device)
        assert rc == 0 and counts == (0, 0, 0) and _untouched(got)
    rc, nbytes, u, buf = _text_device_raw(e, 8)
    assert rc == 0 and (nbytes, u) == (0, 0) and (buf == FILL).all()
    t = e.biunitig_table_np()
    assert len(e.biunitigs_text_np()) == 0 and list(e.biunitigs()) == [] and t["n_circular"] == 0 and len(t["head"]) == 0 and len(t["reversed"]) == 0
    e.close()
    cs = _case(f"lone{k}")
    assert cs.n == 1 and len(cs.text) == k + 1 and cs.table["reversed"].tolist() == [0]
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    _round_trip(cs, g)
    g.close()


# ---- refusals, files, the command line ---------------------------------------------------------------------------------------------------------
def test_refusals_write_nothing(tmp_path):
    _need_gpu()
    cs = _case("graph31")
    n, nu, ncirc = cs.n, len(cs.table["head"]), cs.table["n_circular"]
    g = cs.index()
    for device in (True, False):
        for cap_k, cap_u in ((n - 1, nu), (n, nu - 1), (0, 0)):
            rc, counts, got = _table_raw(g, cap_k, cap_u, device=device)
            assert rc == cbl_amd.ERANGE and counts == (n, nu, ncirc), (device, cap_k, cap_u)  # the need is reported
            assert _untouched(got), "a refused call wrote"
    rc, nbytes, u, buf = _text_device_raw(g, len(cs.text) - 1)
    assert rc == cbl_amd.ERANGE and (nbytes, u) == (len(cs.text), nu) and (buf == FILL).all()
    # a descriptor that cannot be written to: the rule of list_to_fd
    fd = os.open(tmp_path / "ro.txt", os.O_RDONLY | os.O_CREAT, 0o644)
    try:
        with pytest.raises(cbl_amd.CblxError) as e:
            g.biunitigs_to_fd(fd, 100)
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
        g.biunitigs_to_fd(closed, 100)
    assert e.value.code == cbl_amd.EINVAL and "Failed to write the unitigs" in str(e.value)
    with pytest.raises(cbl_amd.CblxError) as e:
        g.biunitigs_to_fd(-1)
    assert e.value.code == cbl_amd.EINVAL
    with pytest.raises(cbl_amd.CblxError):
        g.biunitigs_to_file(tmp_path / "no" / "such" / "dir.txt")
    assert g.biunitigs_text_np().tobytes() == cs.text and g.serialize() == cs.blob  # the index still answers
    g.close()
    # a non-canonical index: it has cblx_unitig_table, and the message says so
    key = "plain31"
    if key not in _cases:
        graph = nm.Graph(31)
        _cases[key] = Case(31, 24, [graph.batch1, graph.batch2], canonical=False)
    pc = _cases[key]
    p = pc.index()
    for device in (True, False):
        rc, counts, got = _table_raw(p, pc.n, pc.n, device=device)
        assert rc == cbl_amd.EINVAL and b"cblx_unitig_table" in _err(p) and counts == (12345, 12345, 12345) and _untouched(got)
    rc, nbytes, u, buf = _text_device_raw(p, 64)
    assert rc == cbl_amd.EINVAL and (buf == FILL).all() and (nbytes, u) == (12345, 12345)
    target = tmp_path / "plain.txt"
    with pytest.raises(cbl_amd.CblxError) as e:
        p.biunitigs_to_file(target)
    assert e.value.code == cbl_amd.EINVAL and not target.exists()
    assert p.serialize() == pc.blob
    p.close()


@pytest.mark.parametrize("name", ["graph33", "edges31"])
def test_biunitigs_to_file_and_fd(name, tmp_path):
    _need_gpu()
    cs = _case(name)
    g = cs.index()
    nu = len(cs.table["head"])
    for chunk in (5, 0):  # a chunk smaller than one line; the default
        path = tmp_path / f"unitigs-{chunk}.txt"
        assert g.biunitigs_to_file(path, chunk) == (nu, len(cs.text))
        assert path.read_bytes() == cs.text
    r, w = os.pipe()
    got = []

    def reader():
        with os.fdopen(r, "rb") as f:
            got.append(f.read())

    t = threading.Thread(target=reader)
    t.start()
    try:
        res = g.biunitigs_to_fd(w, 1000)
    finally:
        os.close(w)
        t.join()
    assert res == (nu, len(cs.text)) and got[0] == cs.text
    assert g.serialize() == cs.blob
    g.close()


def test_cli_unitigs_of_a_canonical_index(tmp_path):
    _need_gpu()
    cs = _case("graph31")
    path = tmp_path / "index.cbl"
    path.write_bytes(cs.blob)
    base = [sys.executable, "-m", "cbl_amd", "-k", str(cs.k), "--prefix-bits", str(cs.pb), "unitigs", str(path)]
    r = subprocess.run(base, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == cs.text
    out = tmp_path / "unitigs.txt"
    r = subprocess.run(base + ["-o", str(out)], env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == cs.text
    lines, human = unitigs_report(um.summary_model(cs.table["length"], cs.table["flags"], cs.k))
    r = subprocess.run(base + ["--stats"], env=dict(os.environ), capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == lines and all(h in r.stderr for h in human)
