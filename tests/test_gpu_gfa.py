"""Links between unitigs and the GFA text on the GPU, in both forms: the link table (host and device arrays), the text (device buffer, file, descriptor)
and `unitigs --gfa`. Every expectation comes from the CPU: the oracle's iteration order through tests/gfa_model.py (every edge of the set, classified
against the sequential walk's table), never from the GPU path; every output is pre-filled with 0xA5 and carries pad elements that must keep the fill, so
an element that is not written, or one written too many, shows."""
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
from oracle import Oracle  # noqa: E402

import biunitigs_model as bm  # noqa: E402  (tests/)
import gfa_model as gm  # noqa: E402
import neighbors_model as nm  # noqa: E402
import unitigs_model as um  # noqa: E402

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
PASS_ENV = "CBLX_NEIGHBOR_PASS"
PASSES = (None, 64, 1000)  # the default (one pass); several passes with a ragged last one
FORMS = (True, False)  # canonical: bidirected unitigs; non-canonical: plain unitigs
FILL, PAD = 0xA5, 3
ARRAYS = (("link_start", np.uint64), ("link_to", np.uint32), ("link_rev", np.uint8))
PB = {15: 6, 31: 24, 33: 16}


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
    return np.frombuffer(bytes([FILL]) * 8, dtype=dt)[0]


# ---- the resident sets and their expectations, once per process ------------------------------------------------------------------------------
_cases = {}


class Case:
    """An index of `batches` (lists of reads, one flush each): the oracle's iteration order, the walk's table, the links by definition, the GFA text."""

    def __init__(self, k, pb, batches, canonical):
        self.k, self.pb, self.batches, self.canonical = k, pb, batches, canonical
        self.oracle = Oracle(k, pb, canonical)
        for batch in batches:
            self.oracle.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = self.oracle.serialize()
        self.resident = nm.oracle_kmers(self.oracle)
        self.n = len(self.resident)
        self.table = gm.walk_model(self.resident, k, canonical)
        self.nu = len(self.table["head"])
        self.links = gm.definition_model(self.resident, k, canonical, self.table)
        self.nl = self.links["n_links"]
        self.lines = gm.n_l_lines(self.links, canonical)
        self.unitig_text = gm.text_model(self.resident, self.table, k, canonical)
        self.text = gm.gfa_model(self.resident, k, canonical, self.table, self.links)

    def index(self):
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        for batch in self.batches:
            g.insert_seqs(*nm.Graph.arrays(batch))
            g.flush()
        assert g.serialize() == self.blob
        return g


def _case(name, canonical):
    key = (name, canonical)
    if key not in _cases:
        if name.startswith("lone"):
            k = int(name[4:])
            _cases[key] = Case(k, PB[k], [[nm._rand(random.Random(k), k).encode()]], canonical)
        else:
            _cases[key] = Case(*bm.crafted(name), canonical)
    return _cases[key]


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------------------
def _links_raw(g, cap_s, cap_l, device, arrays=True):
    """cblx_gfa_links(_device) through the raw ABI on outputs of cap + PAD filled elements: (status, (U, L), dict of the three arrays)."""
    L = cbl_amd.lib()
    counts = [C.c_uint64(12345) for _ in range(2)]
    host = {name: np.full((cap_s if name == "link_start" else cap_l) + PAD, _fill(dt), dtype=dt) for name, dt in ARRAYS}
    signed = {np.uint64: np.int64, np.uint32: np.int32, np.uint8: np.uint8}
    if device:
        dev = {name: torch.from_numpy(host[name].view(signed[dt])).cuda() for name, dt in ARRAYS}
        ptr = {name: t.data_ptr() for name, t in dev.items()}
        fn = L.cblx_gfa_links_device
    else:
        ptr = {name: a.ctypes.data for name, a in host.items()}
        fn = L.cblx_gfa_links
    if not arrays:
        ptr = {name: None for name in ptr}
    rc = fn(g._h, ptr["link_start"], cap_s, ptr["link_to"], ptr["link_rev"], cap_l, *[C.byref(c) for c in counts])
    if device:
        host = {name: dev[name].cpu().numpy().view(dt) for name, dt in ARRAYS}
    return rc, tuple(c.value for c in counts), host


def _untouched(got):
    return all((a == _fill(a.dtype.type)).all() for a in got.values())


def _same_links(got, cs, what):
    for name, dt in ARRAYS:
        m = 2 * cs.nu + 1 if name == "link_start" else cs.nl
        a, w = got[name], cs.links[name]
        bad = np.flatnonzero(a[:m] != w[:m])
        assert not len(bad), f"{what}: {name} wrong at (index, got, expected) {[(int(i), int(a[i]), int(w[i])) for i in bad[:8]]}"
        assert len(a) >= m + PAD and (a[m:] == _fill(dt)).all(), f"{what}: elements behind {name} were written"


def _text_device_raw(g, cap):
    d_buf = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    out = [C.c_uint64(12345) for _ in range(3)]
    rc = cbl_amd.lib().cblx_gfa_text_device(g._h, d_buf.data_ptr(), cap, *[C.byref(c) for c in out])
    return rc, tuple(c.value for c in out), d_buf.cpu().numpy()  # (bytes, unitigs, L lines)


def _check_index(cs, g, monkeypatch, passes=PASSES):
    """Link table and GFA bytes of g equal to the model of cs at every pass size, host and device forms; the numbering is the table calls'; L agrees with
    the degree table; serialize() unchanged afterwards."""
    nu, nl = cs.nu, cs.nl
    for p in passes:
        _set_pass(monkeypatch, p)
        rc, counts, got = _links_raw(g, 2 * nu + 1, nl, device=True)
        assert rc == 0, _err(g)
        assert counts == (nu, nl), (p, counts)
        _same_links(got, cs, f"device links, pass {p}")
        rc, sizes, buf = _text_device_raw(g, len(cs.text))
        assert rc == 0, _err(g)
        assert sizes == (len(cs.text), nu, cs.lines), (p, sizes)
        assert buf[: len(cs.text)].tobytes() == cs.text, f"device text, pass {p}"
        assert (buf[len(cs.text):] == FILL).all(), f"pass {p}: bytes behind the text were written"
    _set_pass(monkeypatch, None)
    rc, counts, got = _links_raw(g, 2 * nu + 6, nl + 2, device=False)  # capacities above the need
    assert rc == 0 and counts == (nu, nl), _err(g)
    _same_links(got, cs, "host links")
    for device in (True, False):
        rc, counts, got = _links_raw(g, 0, 0, device=device, arrays=False)  # null only: counts
        assert rc == 0 and counts == (nu, nl) and _untouched(got)
    t = g.biunitig_table_np() if cs.canonical else g.unitig_table_np()  # the numbering the links speak of is the table calls'
    assert (bm if cs.canonical else um).same_table(t, cs.table)
    lt = g.gfa_links_np()
    assert gm.same_links(lt, cs.links) and lt["link_start"].dtype == np.uint64 and lt["link_to"].dtype == np.uint32 and lt["link_rev"].dtype == np.uint8
    d = g.gfa_links_device()
    assert all(d[name].is_cuda for name, _ in ARRAYS) and (d["n_unitigs"], d["n_links"]) == (nu, nl)
    assert all(np.array_equal(d[name].cpu().numpy().view(dt), cs.links[name]) for name, dt in ARRAYS)
    assert g.gfa_counts() == (nu, nl)
    deg = g.degree_table().astype(np.int64)
    e_out, e_in = int((deg.sum(axis=1) * np.arange(5)).sum()), int((deg.sum(axis=0) * np.arange(5)).sum())
    assert nl == (e_out + e_in - 2 * cs.n + 2 * nu if cs.canonical else e_out - cs.n + nu)
    assert g.gfa_text_np().tobytes() == cs.text
    assert g.gfa_text_device() == (len(cs.text), nu, cs.lines)
    # the unitig text is what it was
    assert (g.biunitigs_text_np() if cs.canonical else g.unitigs_text_np()).tobytes() == cs.unitig_text
    assert g.serialize() == cs.blob and g.validate() == 0  # observers: nothing is modified or sorted


# ---- links and text ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", bm.CRAFTED)
def test_links_and_gfa_text(name, canonical, monkeypatch):
    _need_gpu()
    cs = _case(name, canonical)
    if name == "dense":
        assert (cs.n, cs.nu, cs.nl) == ((36292, 24551, 103027) if canonical else (39344, 16927, 32406))
    if name == "hairpin" and canonical:
        assert cs.nl == 1 and cs.lines == 1
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("k", [15, 31, 33])
def test_empty_index_and_one_kmer(k, canonical, monkeypatch):
    _need_gpu()
    e = cbl_amd.CBL(k, PB[k], canonical=canonical)
    for device in (True, False):
        rc, counts, got = _links_raw(e, 4, 4, device=device)
        assert rc == 0 and counts == (0, 0)
        assert got["link_start"][0] == 0 and (got["link_start"][1:] == _fill(np.uint64)).all() and _untouched({k2: got[k2] for k2 in ("link_to", "link_rev")})
        rc, counts, got = _links_raw(e, 0, 0, device=device)  # link_start needs one element even then
        assert rc == cbl_amd.ERANGE and counts == (0, 0) and _untouched(got)
    rc, sizes, buf = _text_device_raw(e, 16)
    assert rc == 0 and sizes == (11, 0, 0) and buf[:11].tobytes() == gm.HEADER and (buf[11:] == FILL).all()
    assert e.gfa_text_np().tobytes() == gm.HEADER and e.gfa_counts() == (0, 0)
    lt = e.gfa_links_np()
    assert lt["link_start"].tolist() == [0] and len(lt["link_to"]) == 0 and len(lt["link_rev"]) == 0
    e.close()
    cs = _case(f"lone{k}", canonical)
    assert cs.n == 1 and cs.nu == 1 and cs.nl == 0 and cs.text == gm.HEADER + b"S\t0\t" + cs.unitig_text
    g = cs.index()
    _check_index(cs, g, monkeypatch)
    g.close()


# ---- refusals, files, the command line ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
def test_refusals_write_nothing(canonical, tmp_path):
    _need_gpu()
    cs = _case("graph31", canonical)
    nu, nl = cs.nu, cs.nl
    assert nl > 0
    g = cs.index()
    for device in (True, False):
        for cap_s, cap_l in ((2 * nu, nl), (2 * nu + 1, nl - 1), (0, 0)):
            rc, counts, got = _links_raw(g, cap_s, cap_l, device=device)
            assert rc == cbl_amd.ERANGE and counts == (nu, nl), (device, cap_s, cap_l)  # the need is reported
            assert _untouched(got), "a refused call wrote"
    rc, sizes, buf = _text_device_raw(g, len(cs.text) - 1)
    assert rc == cbl_amd.ERANGE and sizes == (len(cs.text), nu, cs.lines) and (buf == FILL).all()
    fd = os.open(tmp_path / "ro.txt", os.O_RDONLY | os.O_CREAT, 0o644)  # a descriptor that cannot be written to: the rule of list_to_fd
    try:
        with pytest.raises(cbl_amd.CblxError) as e:
            g.gfa_to_fd(fd, 100)
    finally:
        os.close(fd)
    assert e.value.code == cbl_amd.EINVAL and "Failed to write the GFA" in str(e.value)
    with pytest.raises(cbl_amd.CblxError) as e:
        g.gfa_to_fd(-1)
    assert e.value.code == cbl_amd.EINVAL
    target = tmp_path / "no" / "such" / "graph.gfa"
    with pytest.raises(cbl_amd.CblxError):
        g.gfa_to_file(target)
    assert not target.exists() and not target.parent.exists()  # a refused call leaves no file
    assert g.gfa_text_np().tobytes() == cs.text and g.serialize() == cs.blob  # the index still answers
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["graph33", "cycles"])
def test_gfa_to_file_and_fd(name, canonical, tmp_path):
    _need_gpu()
    cs = _case(name, canonical)
    g = cs.index()
    for chunk in (5, 997, 0):  # chunks that split lines (one smaller than any line); the default
        path = tmp_path / f"graph-{chunk}.gfa"
        assert g.gfa_to_file(path, chunk) == (cs.nu, cs.lines, len(cs.text))
        assert path.read_bytes() == cs.text
    r, w = os.pipe()
    got = []

    def reader():
        with os.fdopen(r, "rb") as f:
            got.append(f.read())

    t = threading.Thread(target=reader)
    t.start()
    try:
        res = g.gfa_to_fd(w, 1000)
    finally:
        os.close(w)
        t.join()
    assert res == (cs.nu, cs.lines, len(cs.text)) and got[0] == cs.text
    assert g.serialize() == cs.blob
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_cli_unitigs_gfa(canonical, tmp_path):
    _need_gpu()
    cs = _case("graph31", canonical)
    path = tmp_path / "index.cbl"
    path.write_bytes(cs.blob)
    base = [sys.executable, "-m", "cbl_amd", "-k", str(cs.k), "--prefix-bits", str(cs.pb), "unitigs", str(path)]
    r = subprocess.run(base + ["--gfa"], env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == cs.text
    out = tmp_path / "graph.gfa"
    r = subprocess.run(base + ["--gfa", "-o", str(out)], env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0 and r.stdout == b"" and out.read_bytes() == cs.text
    # without the flag: the unitig text, byte for byte
    g = cs.index()
    plain = (g.biunitigs_text_np() if canonical else g.unitigs_text_np()).tobytes()
    g.close()
    r = subprocess.run(base, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == plain == cs.unitig_text
