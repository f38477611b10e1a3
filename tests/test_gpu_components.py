"""Connected components on the GPU, in both forms: the table (host and device arrays), the counts with `rounds`, components_filter and `cbl components`.
Every expectation comes from the CPU — the oracle's iteration order through tests/components_model.py: the walk's table, the link table of the definition, the
hook / compress rule in numpy, removal_model.remove_batch — never from the GPU path; every output is pre-filled with 0xA5 and carries pad elements that must
keep the fill."""
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

import components_model as cm  # noqa: E402  (tests/)
import removal_model as rm  # noqa: E402
import setops_model as sm  # noqa: E402

C = cbl_amd.C
ROOT = Path(__file__).resolve().parent.parent
PASS_ENV = "CBLX_NEIGHBOR_PASS"
PASSES = (None, 64, 1000)  # the default (one pass); several passes with a ragged last one
FORMS = (True, False)  # canonical: bidirected unitigs; non-canonical: plain unitigs
FILL, PAD = 0xA5, 3
WIDE = ["graph15", "graph33", "graph59"]  # of biunitigs_model.crafted: no hi array, and the wide k-mers
LARGE = ("comb", "dense")  # thousands of k-mers: not at 64 k-mers per pass
DTYPES = {"component": np.uint32, "kmer_component": np.uint32, "first": np.uint32, "unitigs": np.uint32, "kmers": np.uint64}


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
    """An index of `flushes` (lists of reads, one insert each): the oracle's bytes, the model index, the model's table."""

    def __init__(self, k, pb, flushes, canonical):
        self.k, self.pb, self.canonical = k, pb, canonical
        self.blob, self.model, self.kmers = cm.build_case(k, pb, canonical, flushes)
        self.n = len(self.kmers)
        self.table = cm.route_model(self.kmers, k, canonical)
        self.counts = cm.counts_of(self.table)
        self.nu, self.nc = self.table["unitigs_n"], self.table["components"]
        self._filtered = {}

    def index(self, blob=None):
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        g.load(self.blob if blob is None else blob)
        return g

    def filtered(self, min_kmers, largest, model=None):
        """(bytes, stats, the model index) of filter_model on a copy of the model index (or of `model`, another layout of the same set: its own table)."""
        key = (min_kmers, largest)
        if model is not None or key not in self._filtered:
            m = rm.copy_cbl(self.model if model is None else model)
            st = cm.filter_model(m, min_kmers, largest, table=self.table if model is None else None)
            if model is not None:
                return m.serialize(), st, m
            self._filtered[key] = (m.serialize(), st, m)
        return self._filtered[key]


def _case(name, canonical):
    key = (name, canonical)
    if key not in _cases:
        _cases[key] = Case(*cm.crafted(name), canonical)
    return _cases[key]


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------------------
def _out(cap, dtype, device):
    host = np.full((cap + PAD) * np.dtype(dtype).itemsize, FILL, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda() if device else None
    return host, dev, (dev.data_ptr() if device else host.ctypes.data)


def _raw(g, caps, device, arrays=cm.ARRAYS):
    """cblx_components(_device) on outputs of cap + PAD filled elements; caps = (unitigs, kmers, components). Returns (status, counts, {name: array})."""
    L = cbl_amd.lib()
    counts = (C.c_uint64 * 6)(*([12345] * 6))
    cap_of = {"component": caps[0], "kmer_component": caps[1], "first": caps[2], "unitigs": caps[2], "kmers": caps[2]}
    outs = {name: _out(cap_of[name], DTYPES[name], device) for name in cm.ARRAYS}
    p = {name: outs[name][2] if name in arrays else None for name in cm.ARRAYS}
    rc = (L.cblx_components_device if device else L.cblx_components)(g._h, p["component"], caps[0], p["kmer_component"], caps[1], p["first"], p["unitigs"], p["kmers"],
                                                                       caps[2], counts)
    got = {name: (o[1].cpu().numpy() if device else o[0]).view(DTYPES[name]) for name, o in outs.items()}
    return rc, tuple(int(v) for v in counts), got


def _same(got, want, what):
    m = len(want)
    fill = np.frombuffer(bytes([FILL]) * got.dtype.itemsize, dtype=got.dtype)[0]
    bad = np.flatnonzero(got[:m] != want)
    assert not len(bad), f"{what}: wrong at (index, got, expected) {[(int(i), int(got[i]), int(want[i])) for i in bad[:8]]}"
    assert len(got) >= m + PAD and (got[m:] == fill).all(), f"{what}: elements behind the output were written"


def _untouched(got, names=cm.ARRAYS):
    return all((got[name].view(np.uint8) == FILL).all() for name in names)


def _check_table(cs, g, monkeypatch, passes):
    t = cs.table
    for p in passes:
        _set_pass(monkeypatch, p)
        for device in (True, False):
            rc, counts, got = _raw(g, (cs.nu + 2, cs.n, cs.nc), device)  # one capacity above the need
            assert rc == 0 and counts == cs.counts, (_err(g), p, device, counts, cs.counts)  # `rounds` among them
            for name in cm.ARRAYS:
                _same(got[name], t[name], f"{name}, pass {p}, device {device}")
    _set_pass(monkeypatch, None)
    for device in (True, False):
        rc, counts, got = _raw(g, (cs.nu, 0, cs.nc), device, arrays=("component", "kmers"))  # some arrays alone
        assert rc == 0 and counts == cs.counts and _untouched(got, ("kmer_component", "first", "unitigs"))
        _same(got["component"], t["component"], "component alone")
        _same(got["kmers"], t["kmers"], "kmers alone")
        rc, counts, got = _raw(g, (0, 0, 0), device, arrays=())  # null only: the counts
        assert rc == 0 and counts == cs.counts and _untouched(got)
    assert g.component_counts() == dict(zip(cm.COUNTS, cs.counts))
    for per_kmer in (False, True):
        h, d = g.components_np(per_kmer), g.components_device(per_kmer)
        assert ("kmer_component" in h) == ("kmer_component" in d) == per_kmer
        for name in cm.ARRAYS:
            if name == "kmer_component" and not per_kmer:
                continue
            assert h[name].dtype == DTYPES[name] and np.array_equal(h[name], t[name]), name
            assert d[name].is_cuda and np.array_equal(d[name].cpu().numpy().view(DTYPES[name]), t[name]), name
        assert (h["n_kmers"], h["n_unitigs"], h["n_links"], h["n_components"], h["largest_kmers"], h["rounds"]) == cs.counts
    # the numbering is the table calls', the links are the link table's
    table = g.biunitig_table_np() if cs.canonical else g.unitig_table_np()
    assert np.array_equal(np.bincount(t["component"], weights=table["length"], minlength=cs.nc).astype(np.uint64), t["kmers"])
    lt = g.gfa_links_np()
    frm, to = cm.link_pairs(lt)
    assert lt["n_links"] == cs.counts[2] and np.array_equal(t["component"][frm], t["component"][to])
    assert g.serialize() == cs.blob and g.validate() == 0  # observers: nothing is modified or sorted


# ---- the table -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", cm.CRAFTED + cm.OLD + WIDE)
def test_component_table(name, canonical, monkeypatch):
    _need_gpu()
    cs = _case(name, canonical)
    g = cs.index()
    _check_table(cs, g, monkeypatch, (None, 1000) if name in LARGE else PASSES)
    g.close()


# ---- components_filter -----------------------------------------------------------------------------------------------------------------------------
def _rules(cs, name):
    """(min_kmers, largest): at, below and above every edge, the identity, everything, and `largest`."""
    sizes = sorted(set(cs.table["kmers"].tolist()))
    edges = sorted({v for s in sizes for v in (s - 1, s, s + 1) if v >= 1}) if len(sizes) <= 6 else sorted({1, sizes[0], sizes[0] + 1, sizes[-1], sizes[-1] + 1})
    if name in cm.MIN_KMERS:
        mk = cm.MIN_KMERS[name]
        assert {mk - 1, mk, mk + 1, mk + 2} <= set(edges)
    return [(v, False) for v in edges] + [(None, True)]


def _check_filter(cs, blob, monkeypatch, rules, model=None, passes=PASSES, what=""):
    g = cs.index(blob)
    for min_kmers, largest in rules:
        want, st, m = cs.filtered(min_kmers, largest, model)
        for p in passes:
            _set_pass(monkeypatch, p)
            g.load(blob)
            got = g.components_filter(min_kmers, largest=largest)
            assert got == st, (what, min_kmers, largest, p, got, st)
            assert g.serialize() == want, (what, min_kmers, largest, p)
            assert g.count() == m.count() and g.num_buckets() == len(m.buckets) and g.is_empty() == (m.count() == 0) and g.validate(False) == 0
    _set_pass(monkeypatch, None)
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["arch15", "arch31", "strands", "islands", "branch", "cycles", "one", "graph33", "graph59"])
def test_components_filter(name, canonical, monkeypatch):
    """Key widths: arch15 (no hi array), arch31 (a byte-wide hi), graph33 and graph59 (a wide k-mer)."""
    _need_gpu()
    cs = _case(name, canonical)
    rules = _rules(cs, name)
    _check_filter(cs, cs.blob, monkeypatch, rules, passes=(None, 64) if name.startswith("arch") else (None,), what=name)
    assert cs.filtered(1, False)[0] == cs.blob and cs.filtered(cs.table["largest_kmers"] + 1, False)[2].count() == 0  # the identity; nothing left
    empty = cbl_amd.CBL(cs.k, cs.pb, canonical=canonical)
    assert cs.filtered(cs.table["largest_kmers"] + 1, False)[0] == empty.serialize()
    empty.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_bucket_kinds(canonical, monkeypatch):
    """The same set in three layouts: as built; every bucket declared a Trie (a visited one comes out as an ascending Vec, an unvisited one stays a
    Trie); every Vec shuffled (swap_remove shows the order). The iteration order, and with it the unitig and component numbers, differ between them."""
    _need_gpu()
    cs = _case("arch15", canonical)
    mk = cm.MIN_KMERS["arch15"]
    built = {p: (kind, list(items)) for p, (kind, items) in cs.model.buckets.items()}
    rng = random.Random(5)
    layouts = {"built": built, "tries": {p: ("trie", sorted(items)) for p, (_, items) in built.items()},
               "shuffled": {p: (kind, rng.sample(items, len(items)) if kind == "vec" else items) for p, (kind, items) in built.items()}}
    blobs = {}
    for what, buckets in layouts.items():
        model = sm.from_buckets(cs.k, cs.pb, canonical, buckets)
        want, st, after = cs.filtered(mk, False, model)
        blobs[what] = want
        assert st["removed_kmers"] > 0 and len(after.buckets) < len(model.buckets)  # a bucket that the filter empties
        assert sm.words(after) < sm.words(model)
        _check_filter(cs, model.serialize(), monkeypatch, [(mk, False), (mk + 1, False), (None, True)], model=model, passes=(None, 64), what=what)
    assert len(set(blobs.values())) == 3


# ---- refusals, the empty index, the command line -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
def test_refusals_write_and_remove_nothing(canonical):
    _need_gpu()
    cs = _case("arch31", canonical)
    g = cs.index()
    L = cbl_amd.lib()
    full = (cs.nu, cs.n, cs.nc)
    for device in (True, False):
        for short in range(3):  # one capacity short, the others exact: the need is reported, every fill stays
            for cap in (full[short] - 1, 0):
                caps = tuple(cap if j == short else full[j] for j in range(3))
                rc, counts, got = _raw(g, caps, device)
                assert rc == cbl_amd.ERANGE and counts == cs.counts and _untouched(got), (device, short, cap)
        rc, counts, got = _raw(g, (cs.nu, 0, 0), device, arrays=("component",))  # a capacity of 0 behind a null array is no refusal
        assert rc == 0 and counts == cs.counts
    st = cbl_amd.ComponentStats(*([77] * 6))
    mk = cm.MIN_KMERS["arch31"]
    for min_kmers, flags in ((0, 0), (mk, 1), (mk, 2), (0, 3), (mk, 0x80000000)):  # no rule; both rules; unknown flag bits
        assert L.cblx_components_filter(g._h, min_kmers, flags, C.byref(st)) == cbl_amd.EINVAL, (min_kmers, flags)
    assert all(getattr(st, name) == 77 for name in cm.STATS)
    for kw in ({}, {"min_kmers": 0}, {"min_kmers": mk, "largest": True}):
        with pytest.raises(cbl_amd.CblxError) as e:
            g.components_filter(**kw)
        assert e.value.code == cbl_amd.EINVAL
    assert g.serialize() == cs.blob and g.count() == cs.n
    assert L.cblx_components_filter(g._h, mk, 0, None) == 0 and g.serialize() == cs.filtered(mk, False)[0]  # stats may be null
    again = g.components_filter(mk)  # one call is the fixpoint
    assert again["removed_kmers"] == 0 and again["components"] == cs.nc - cs.filtered(mk, False)[1]["removed_components"] and g.serialize() == cs.filtered(mk, False)[0]
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_empty_index(canonical):
    _need_gpu()
    g = cbl_amd.CBL(31, 24, canonical=canonical)
    for device in (True, False):
        rc, counts, got = _raw(g, (4, 4, 4), device)
        assert rc == 0 and counts == (0, 0, 0, 0, 0, 0) and _untouched(got)
    assert g.components_filter(5) == dict.fromkeys(cm.STATS, 0) and g.components_filter(largest=True) == dict.fromkeys(cm.STATS, 0)
    t = g.components_np(per_kmer=True)
    assert all(t[name].tolist() == [] for name in cm.ARRAYS) and t["n_components"] == 0
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_cli_components(canonical, tmp_path):
    _need_gpu()
    cs = _case("arch31", canonical)
    mk, t = cm.MIN_KMERS["arch31"], cs.table
    path, out = tmp_path / "index.cbl", tmp_path / "filtered.cbl"
    path.write_bytes(cs.blob)
    base = [sys.executable, "-m", "cbl_amd", "-k", str(cs.k), "--prefix-bits", str(cs.pb), "components", str(path)]
    r = subprocess.run(base + ["--sizes"], env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    summary = cbl_amd.CBL.component_summary(t["kmers"], t["unitigs"])
    assert summary["components"] == cs.nc and summary["largest"] == t["largest_kmers"] and summary["singletons"] == int((t["unitigs"] == 1).sum())
    head = (f"kmers\t{cs.n}\nunitigs\t{cs.nu}\nlinks\t{cs.counts[2]}\ncomponents\t{cs.nc}\nlargest\t{t['largest_kmers']}\nsingletons\t{summary['singletons']}\n"
            f"largest_fraction\t{t['largest_kmers'] / cs.n:.6f}\n")
    assert r.stdout.decode() == head + "".join(f"{c}\t{k}\t{u}\n" for c, (k, u) in enumerate(zip(t["kmers"].tolist(), t["unitigs"].tolist())))
    for extra, rule in ((["--min-kmers", str(mk)], (mk, False)), (["--largest"], (None, True))):
        r = subprocess.run(base + ["-o", str(out)] + extra, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
        assert r.returncode == 0, r.stderr
        want, st, _ = cs.filtered(*rule)
        assert out.read_bytes() == want
        assert r.stdout.decode() == "".join(f"{key}\t{st[key]}\n" for key in cm.STATS)
    assert path.read_bytes() == cs.blob
