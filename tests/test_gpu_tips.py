"""Tip clipping on the GPU, in both forms: the degrees at the unitig ends, the marks (host and device arrays), clip_tips and `cbl clip`. Every expectation
comes from the CPU — the oracle's iteration order through tests/tips_model.py: the walk's table, the masks of the set, removal_model.remove_batch — never
from the GPU path; every output is pre-filled with 0xA5 and carries pad elements that must keep the fill."""
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
from oracle import Oracle  # noqa: E402

import biunitigs_model as bm  # noqa: E402  (tests/)
import neighbors_model as nm  # noqa: E402
import removal_model as rm  # noqa: E402
import setops_model as sm  # noqa: E402
import tips_model as tm  # noqa: E402

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
PASS_ENV = "CBLX_NEIGHBOR_PASS"
PASSES = (None, 64, 1000)  # the default (one pass); several passes with a ragged last one
FORMS = (True, False)  # canonical: bidirected unitigs; non-canonical: plain unitigs
FILL, PAD = 0xA5, 3
OLD = ["dense", "branch", "graph15", "cycles", "hairpin", "homopolymers", "at"]  # of biunitigs_model.crafted, at max_kmers = K - 1


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


# ---- the resident sets and their expectations, once per process ------------------------------------------------------------------------------
_cases = {}


class Case:
    """An index of `batches` (lists of reads, one flush each): the oracle's bytes, the model index, the marks of its first round."""

    def __init__(self, k, pb, batches, mk, canonical):
        self.k, self.pb, self.batches, self.mk, self.canonical = k, pb, batches, mk, canonical
        o = Oracle(k, pb, canonical)
        for batch in batches:
            o.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = o.serialize()
        self.model = tm.model_of_words(k, pb, canonical, o.iter_words())
        assert self.model.serialize() == self.blob
        self.kmers = nm.oracle_kmers(o)
        self.n = len(self.kmers)
        self.marks = tm.marks_of_set(self.kmers, k, canonical, mk)
        self.nu = len(self.marks["kind"])
        self._clipped = {}

    def index(self, blob=None):
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        g.load(self.blob if blob is None else blob)
        return g

    def clipped(self, isolated, rounds, model=None):
        """(bytes, stats, the model index) of clip_model on a copy of the model index (or of `model`)."""
        key = (isolated, rounds)
        if model is not None or key not in self._clipped:
            m = rm.copy_cbl(self.model if model is None else model)
            st = tm.clip_model(m, self.mk, isolated, rounds)
            if model is not None:
                return m.serialize(), st, m
            self._clipped[key] = (m.serialize(), st, m)
        return self._clipped[key]


def _case(name, canonical):
    key = (name, canonical)
    if key not in _cases:
        if name in tm.CRAFTED:
            _cases[key] = Case(*tm.crafted(name), canonical)
        else:
            k, pb, flushes = bm.crafted(name)
            _cases[key] = Case(k, pb, flushes, k - 1, canonical)
    return _cases[key]


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------------------
def _bytes_out(cap, device):
    host = np.full(cap + PAD, FILL, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda() if device else None
    return host, dev, (dev.data_ptr() if device else host.ctypes.data)


def _ends_raw(g, cap, device, arrays=(True, True)):
    """cblx_unitig_ends(_device) on outputs of cap + PAD filled bytes: (status, U, left, right)."""
    L = cbl_amd.lib()
    u = C.c_uint64(12345)
    outs = [_bytes_out(cap, device) for _ in range(2)]
    ptrs = [o[2] if on else None for o, on in zip(outs, arrays)]
    rc = (L.cblx_unitig_ends_device if device else L.cblx_unitig_ends)(g._h, ptrs[0], ptrs[1], cap, C.byref(u))
    return (rc, u.value) + tuple(o[1].cpu().numpy() if device else o[0] for o in outs)


def _mark_raw(g, mk, cap, device, array=True):
    """cblx_tips_mark(_device): (status, U, counts, kind)."""
    L = cbl_amd.lib()
    u, counts = C.c_uint64(12345), (C.c_uint64 * 4)(7, 7, 7, 7)
    host, dev, ptr = _bytes_out(cap, device)
    rc = (L.cblx_tips_mark_device if device else L.cblx_tips_mark)(g._h, mk, ptr if array else None, cap, C.byref(u), counts)
    return rc, u.value, tuple(int(v) for v in counts), (dev.cpu().numpy() if device else host)


def _same(got, want, what):
    m = len(want)
    bad = np.flatnonzero(got[:m] != want)
    assert not len(bad), f"{what}: wrong at (index, got, expected) {[(int(i), int(got[i]), int(want[i])) for i in bad[:8]]}"
    assert len(got) >= m + PAD and (got[m:] == FILL).all(), f"{what}: elements behind the output were written"


def _check_observers(cs, g, monkeypatch, passes=PASSES):
    nu, mk = cs.nu, cs.mk
    left, right, kind, counts = cs.marks["left"], cs.marks["right"], cs.marks["kind"], cs.marks["counts"]
    for p in passes:
        _set_pass(monkeypatch, p)
        for device in (True, False):
            rc, u, got_l, got_r = _ends_raw(g, nu, device)
            assert rc == 0 and u == nu, (_err(g), p, device)
            _same(got_l, left, f"left, pass {p}, device {device}")
            _same(got_r, right, f"right, pass {p}, device {device}")
            rc, u, got_c, got_k = _mark_raw(g, mk, nu + 2, device)  # a capacity above the need
            assert rc == 0 and u == nu and got_c == counts, (_err(g), p, device, got_c, counts)
            _same(got_k, kind, f"kind, pass {p}, device {device}")
    _set_pass(monkeypatch, None)
    for device in (True, False):
        rc, u, got_l, got_r = _ends_raw(g, nu, device, arrays=(False, True))  # one array alone
        assert rc == 0 and u == nu and (got_l == FILL).all()
        _same(got_r, right, "right alone")
        rc, u, got_l, got_r = _ends_raw(g, 0, device, arrays=(False, False))  # null only: the count
        assert rc == 0 and u == nu and (got_l == FILL).all() and (got_r == FILL).all()
        rc, u, got_c, got_k = _mark_raw(g, mk, 0, device, array=False)
        assert rc == 0 and u == nu and got_c == counts and (got_k == FILL).all()
    e = g.unitig_ends_np()
    assert e["n_unitigs"] == nu and e["left"].dtype == np.uint8 and np.array_equal(e["left"], left) and np.array_equal(e["right"], right)
    d = g.unitig_ends_device()
    assert d["left"].is_cuda and np.array_equal(d["left"].cpu().numpy(), left) and np.array_equal(d["right"].cpu().numpy(), right)
    t = g.tips_np(mk)
    names = cbl_amd.TIP_COUNTS
    assert np.array_equal(t["kind"], kind) and tuple(t[key] for key in names) == counts and t["n_unitigs"] == nu
    assert tuple(g.tip_counts(mk)[key] for key in names) == counts
    if mk == cs.k - 1:
        assert np.array_equal(g.tips_np()["kind"], kind)  # the default: unitigs shorter than K k-mers
    table = g.biunitig_table_np() if cs.canonical else g.unitig_table_np()  # the numbering is the table calls'; the rule restated on the host
    assert np.array_equal(cbl_amd.CBL.tip_kinds(table["length"], table["flags"], e["left"], e["right"], mk), kind)
    assert g.serialize() == cs.blob and g.validate() == 0  # observers: nothing is modified or sorted


def _check_clip(cs, blob, monkeypatch, model=None, passes=PASSES, what=""):
    """clip_tips on an index loaded from blob, for rounds = 1, 2, 0 with isolated off and on: the bytes and the stats of clip_model."""
    g = cs.index(blob)
    for isolated in (False, True):
        for rounds in (1, 2, 0):
            want, st, m = cs.clipped(isolated, rounds, model)
            for p in passes:
                _set_pass(monkeypatch, p)
                g.load(blob)
                got = g.clip_tips(cs.mk, isolated=isolated, rounds=rounds)
                assert got == st, (what, isolated, rounds, p, got, st)
                assert g.serialize() == want, (what, isolated, rounds, p)
                assert g.count() == m.count() and g.num_buckets() == len(m.buckets) and g.is_empty() == (m.count() == 0) and g.validate(False) == 0
    _set_pass(monkeypatch, None)
    g.close()


# ---- the observers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", tm.CRAFTED + OLD)
def test_ends_and_marks(name, canonical, monkeypatch):
    _need_gpu()
    cs = _case(name, canonical)
    g = cs.index()
    _check_observers(cs, g, monkeypatch)
    g.close()


# ---- clip_tips ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", tm.CRAFTED + ["graph15", "branch", "homopolymers"])
def test_clip_tips(name, canonical, monkeypatch):
    """Key widths: edge15 (no hi array), edge (a byte-wide hi), edge33 and edge59 (a wide k-mer)."""
    _need_gpu()
    cs = _case(name, canonical)
    _check_clip(cs, cs.blob, monkeypatch, what=name)
    if name == "fork":
        g = cs.index()
        st = g.clip_tips(cs.mk)
        assert g.is_empty() and st["kmers_left"] == 0 and g.serialize() == cbl_amd.CBL(cs.k, cs.pb, canonical=canonical).serialize()
        assert g.clip_tips(cs.mk, rounds=0) == dict.fromkeys(tm.STATS, 0) | {"rounds": 1, "fixpoint": 1}  # an empty index
        g.close()
    if name == "cascade":
        assert [(cs.clipped(False, r)[1]["rounds"], cs.clipped(False, r)[1]["fixpoint"]) for r in (1, 2, 0)] == [(1, 0), (2, 0), (3, 1)]
        assert cs.clipped(False, 1)[0] != cs.clipped(False, 2)[0]


@pytest.mark.parametrize("canonical", FORMS)
def test_clip_tips_dense(canonical, monkeypatch):
    """16 buckets of thousands of words (Tries), two removing rounds in the plain form."""
    _need_gpu()
    cs = _case("dense", canonical)
    want, st, m = cs.clipped(False, 0)
    assert (cs.n, st["rounds"], st["kmers_left"]) == ((36292, 2, 36064) if canonical else (39344, 3, 38662))
    g = cs.index()
    for p in (None, 1000):
        _set_pass(monkeypatch, p)
        g.load(cs.blob)
        assert g.clip_tips(rounds=0) == st and g.serialize() == want and g.validate(False) == 0
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_bucket_kinds(canonical, monkeypatch):
    """The same set in three layouts: as built; every bucket declared a Trie (a visited one comes out as an ascending Vec, an unvisited one stays a
    Trie); every Vec shuffled (swap_remove shows the order)."""
    _need_gpu()
    cs = _case("deep", canonical)
    built = {p: (kind, list(items)) for p, (kind, items) in cs.model.buckets.items()}
    rng = random.Random(5)
    layouts = {"built": built, "tries": {p: ("trie", sorted(items)) for p, (_, items) in built.items()},
               "shuffled": {p: (kind, rng.sample(items, len(items)) if kind == "vec" else items) for p, (kind, items) in built.items()}}
    blobs = {}
    for what, buckets in layouts.items():
        model = sm.from_buckets(cs.k, cs.pb, canonical, buckets)
        want, st, after = cs.clipped(True, 1, model)
        blobs[what] = want
        sel = tm.selected(cs.marks, True)
        gone = {w for w, f in zip(tm.iteration_words(cs.model), sel.tolist()) if f}  # the same k-mers in every layout: the set decides
        sb = model.P["SB"]
        visited = {w >> sb for w in gone}
        assert sm.words(after) == sm.words(model) - gone
        emptied = [p for p in buckets if p not in after.buckets]
        assert emptied and set(emptied) <= visited  # a bucket that empties
        if what == "tries":
            assert any(after.buckets[p][0] == "vec" and after.buckets[p][1] == sorted(after.buckets[p][1]) and len(after.buckets[p][1]) > 1 for p in visited - set(emptied))
            assert any(after.buckets[p][0] == "trie" for p in set(buckets) - visited)  # an unvisited Trie stays one
        else:  # a Vec that loses a word that is not its last one
            lost = {p: [((p << sb) | s) in gone for s in items] for p, (kind, items) in buckets.items() if kind == "vec"}
            assert any(True in f and False in f[f.index(True):] for f in lost.values())
        _check_clip(cs, model.serialize(), monkeypatch, model=model, passes=(None, 64), what=what)
    assert len(set(blobs.values())) == 3


# ---- refusals, the command line ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
def test_refusals_write_and_remove_nothing(canonical):
    _need_gpu()
    cs = _case("edge", canonical)
    nu = cs.nu
    g = cs.index()
    L = cbl_amd.lib()
    for device in (True, False):
        for cap in (nu - 1, 0):  # a short capacity: the need is reported, the fill stays
            rc, u, got_l, got_r = _ends_raw(g, cap, device)
            assert rc == cbl_amd.ERANGE and u == nu and (got_l == FILL).all() and (got_r == FILL).all(), (device, cap)
            rc, u, got_c, got_k = _mark_raw(g, cs.mk, cap, device)
            assert rc == cbl_amd.ERANGE and u == nu and (got_k == FILL).all(), (device, cap)
        rc, u, got_c, got_k = _mark_raw(g, 0, nu, device)  # max_kmers = 0
        assert rc == cbl_amd.EINVAL and (got_k == FILL).all()
    st = cbl_amd.ClipStats(*([77] * 7))
    assert L.cblx_clip_tips(g._h, 0, 0, 1, C.byref(st)) == cbl_amd.EINVAL  # max_kmers = 0
    assert L.cblx_clip_tips(g._h, cs.mk, 2, 1, C.byref(st)) == cbl_amd.EINVAL and L.cblx_clip_tips(g._h, cs.mk, 0x80000001, 0, C.byref(st)) == cbl_amd.EINVAL  # unknown flag bits
    assert all(getattr(st, name) == 77 for name in tm.STATS)
    with pytest.raises(cbl_amd.CblxError) as e:
        g.clip_tips(0)
    assert e.value.code == cbl_amd.EINVAL
    assert g.serialize() == cs.blob and g.count() == cs.n
    assert L.cblx_clip_tips(g._h, cs.mk, 0, 1, None) == 0 and g.serialize() == cs.clipped(False, 1)[0]  # stats may be null
    g.close()
    # An even K is refused where the index is created (K must be odd), in either form: no index of an even K exists for the form's own refusal to meet
    for canon in FORMS:
        with pytest.raises(cbl_amd.CblxError) as e:
            cbl_amd.CBL(30, 24, canonical=canon)
        assert e.value.code == cbl_amd.EINVAL


@pytest.mark.parametrize("canonical", FORMS)
def test_empty_index(canonical):
    _need_gpu()
    g = cbl_amd.CBL(31, 24, canonical=canonical)
    for device in (True, False):
        rc, u, got_l, got_r = _ends_raw(g, 4, device)
        assert rc == 0 and u == 0 and (got_l == FILL).all() and (got_r == FILL).all()
        rc, u, got_c, got_k = _mark_raw(g, 5, 0, device)
        assert rc == 0 and u == 0 and got_c == (0, 0, 0, 0) and (got_k == FILL).all()
    for rounds in (0, 1, 3):
        assert g.clip_tips(rounds=rounds, isolated=True) == dict.fromkeys(tm.STATS, 0) | {"rounds": 1, "fixpoint": 1}
    assert g.tips_np()["kind"].tolist() == [] and g.unitig_ends_np()["left"].tolist() == []
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_cli_clip(canonical, tmp_path):
    _need_gpu()
    cs = _case("cascade", canonical)
    path, out = tmp_path / "index.cbl", tmp_path / "clipped.cbl"
    path.write_bytes(cs.blob)
    base = [sys.executable, "-m", "cbl_amd", "-k", str(cs.k), "--prefix-bits", str(cs.pb), "clip", str(path), "-o", str(out), "--max-kmers", str(cs.mk)]
    for extra, isolated, rounds in (([], False, 1), (["--rounds", "0", "--isolated"], True, 0)):
        r = subprocess.run(base + extra, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
        assert r.returncode == 0, r.stderr
        want, st, _ = cs.clipped(isolated, rounds)
        g = cs.index()
        assert g.clip_tips(cs.mk, isolated=isolated, rounds=rounds) == st
        assert out.read_bytes() == g.serialize() == want  # the round trip equals the method's bytes
        g.close()
        assert r.stdout.decode() == "".join(f"{key}\t{st[key]}\n" for key in tm.STATS)
    assert path.read_bytes() == cs.blob
