"""Bubble popping on the GPU, in both forms: the marks (host and device arrays, with and without counts), pop_bubbles with the carried counts, and
`cbl pop`. Every expectation comes from the CPU — the oracle's iteration order through tests/bubbles_model.py: the walk's table, the link table of the
definition, removal_model.remove_batch — never from the GPU path; every output is pre-filled with 0xA5 and carries pad elements that must keep the fill."""
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

import bubbles_model as bb  # noqa: E402  (tests/)
import gfa_model as gm  # noqa: E402
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
FILL32 = 0xA5A5A5A5


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


def _dev_counts(counts, pad=PAD):
    """A device array of the counts with `pad` filled elements behind them: (tensor of len + pad int32, pointer or None)."""
    host = np.concatenate([np.asarray(counts, dtype=np.uint32), np.full(pad, FILL32, dtype=np.uint32)])
    t = torch.from_numpy(host.view(np.int32).copy()).cuda()
    return t, t.data_ptr()


def _host(t):
    return t.cpu().numpy().view(np.uint32)


# ---- the resident sets and their expectations, once per process ------------------------------------------------------------------------------
_cases = {}


class Case:
    """An index of the flushes of a crafted case: the oracle's bytes, the model index, the counts of its tally, the marks of its first round."""

    def __init__(self, name, canonical):
        self.k, self.pb, batches, self.mk, self.tally = bb.crafted(name)
        self.canonical = canonical
        o = Oracle(self.k, self.pb, canonical)
        for batch in batches:
            o.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = o.serialize()
        self.model = tm.model_of_words(self.k, self.pb, canonical, o.iter_words())
        assert self.model.serialize() == self.blob
        self.kmers = nm.oracle_kmers(o)
        self.n = len(self.kmers)
        self.table = gm.walk_model(self.kmers, self.k, canonical)
        self.counts = bb.counts_of_case(self.model, self.kmers, self.table, self.tally)
        self.reads = None if callable(self.tally) else self.tally
        self.marks = {False: bb.marks_of_set(self.kmers, self.k, canonical, self.mk), True: bb.marks_of_set(self.kmers, self.k, canonical, self.mk, self.counts)}
        self.nu = len(self.table["head"])
        self._popped = {}

    def index(self, blob=None):
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        g.load(self.blob if blob is None else blob)
        return g

    def counts_for(self, model):
        """The case's counts in the iteration order of another layout of the same set."""
        by_word = dict(zip(tm.iteration_words(self.model), self.counts.tolist()))
        return np.array([by_word[w] for w in tm.iteration_words(model)], dtype=np.uint32)

    def popped(self, counted, rounds, model=None):
        """(bytes, stats, counts after or None, the model index) of pop_model on a copy of the model index (or of `model`)."""
        key = (counted, rounds)
        if model is not None or key not in self._popped:
            m = rm.copy_cbl(self.model if model is None else model)
            cnt = None if not counted else self.counts if model is None else self.counts_for(model)
            st, after = bb.pop_model(m, self.mk, cnt, rounds)
            if model is not None:
                return m.serialize(), st, after, m
            self._popped[key] = (m.serialize(), st, after, m)
        return self._popped[key]


def _case(name, canonical):
    key = (name, canonical)
    if key not in _cases:
        _cases[key] = Case(name, canonical)
    return _cases[key]


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------------------
def _bytes_out(cap, device):
    host = np.full(cap + PAD, FILL, dtype=np.uint8)
    dev = torch.from_numpy(host).cuda() if device else None
    return host, dev, (dev.data_ptr() if device else host.ctypes.data)


def _mark_raw(g, mk, cap, device, d_counts=None, n_counts=0, array=True):
    """cblx_bubbles_mark(_device): (status, U, counts, kind)."""
    L = cbl_amd.lib()
    u, counts = C.c_uint64(12345), (C.c_uint64 * 3)(7, 7, 7)
    host, dev, ptr = _bytes_out(cap, device)
    rc = (L.cblx_bubbles_mark_device if device else L.cblx_bubbles_mark)(g._h, mk, d_counts, n_counts, ptr if array else None, cap, C.byref(u), counts)
    return rc, u.value, tuple(int(v) for v in counts), (dev.cpu().numpy() if device else host)


def _pop_raw(g, mk, d_counts, n_counts, rounds, flags=0, stats=True):
    st = cbl_amd.BubbleStats(*([77] * 6))
    rc = cbl_amd.lib().cblx_pop_bubbles(g._h, mk, d_counts, n_counts, flags, rounds, C.byref(st) if stats else None)
    return rc, {name: int(getattr(st, name)) for name in bb.STATS}


def _same(got, want, what):
    m = len(want)
    bad = np.flatnonzero(got[:m] != want)
    assert not len(bad), f"{what}: wrong at (index, got, expected) {[(int(i), int(got[i]), int(want[i])) for i in bad[:8]]}"
    assert len(got) >= m + PAD and (got[m:] == FILL).all(), f"{what}: elements behind the output were written"


def _check_observers(cs, g, monkeypatch, passes=PASSES):
    nu, mk = cs.nu, cs.mk
    t_counts, p_counts = _dev_counts(cs.counts)
    for counted in (False, True):
        kind, counts = cs.marks[counted]["kind"], cs.marks[counted]["counts"]
        args = (p_counts if cs.n else None, cs.n) if counted else (None, 0)
        for p in passes:
            _set_pass(monkeypatch, p)
            for device in (True, False):
                rc, u, got_c, got_k = _mark_raw(g, mk, nu + 2, device, *args)  # a capacity above the need
                assert rc == 0 and u == nu and got_c == counts, (_err(g), p, device, counted, got_c, counts)
                _same(got_k, kind, f"kind, pass {p}, device {device}, counted {counted}")
        _set_pass(monkeypatch, None)
        for device in (True, False):
            rc, u, got_c, got_k = _mark_raw(g, mk, 0, device, *args, array=False)  # null: the counts alone
            assert rc == 0 and u == nu and got_c == counts and (got_k == FILL).all()
        cnt = t_counts[: cs.n] if counted else None
        got_kind, got = g.bubbles_np(mk, cnt)
        assert got_kind.dtype == np.uint8 and np.array_equal(got_kind, kind) and tuple(got[key] for key in cbl_amd.BUBBLE_COUNTS) == counts and got["n_unitigs"] == nu
        assert g.bubble_counts(mk, cnt) == got
        d_kind = torch.full((nu + PAD,), FILL, dtype=torch.uint8, device="cuda")
        assert g.bubbles_mark_device(mk, cnt, d_kind, nu) == got
        _same(d_kind.cpu().numpy(), kind, "bubbles_mark_device")
        # the rule restated on the host, on the arrays of the other observers: the numbering is the table calls'
        lt = g.gfa_links_np()
        table = g.biunitig_table_np() if cs.canonical else g.unitig_table_np()
        left = None if cs.canonical else g.unitig_ends_np()["left"]
        kc = g.unitig_coverage_np(cnt) if counted else None
        assert np.array_equal(cbl_amd.CBL.bubble_kinds(lt["link_start"], lt["link_to"], lt["link_rev"], table["length"], left, kc, mk), kind)
    assert np.array_equal(_host(t_counts), np.concatenate([cs.counts, np.full(PAD, FILL32, dtype=np.uint32)]))  # the observers only read the counts
    assert g.serialize() == cs.blob and g.validate() == 0  # observers: nothing is modified or sorted


def _check_pop(cs, blob, monkeypatch, model=None, passes=(None, 64), what=""):
    """pop_bubbles on an index loaded from blob, for rounds = 1, 2, 0 with and without counts: the bytes, the stats and the carried array of pop_model."""
    g = cs.index(blob)
    start = cs.counts if model is None else cs.counts_for(model)
    for counted in (False, True):
        for rounds in (1, 2, 0):
            want, st, after, m = cs.popped(counted, rounds, model)
            for p in passes:
                _set_pass(monkeypatch, p)
                g.load(blob)
                t, ptr = _dev_counts(start)
                rc, got = _pop_raw(g, cs.mk, ptr if counted and cs.n else None, cs.n if counted else 0, rounds)
                assert rc == 0 and got == st, (what, counted, rounds, p, _err(g), got, st)
                assert g.serialize() == want, (what, counted, rounds, p)
                assert g.count() == m.count() and g.num_buckets() == len(m.buckets) and g.validate(False) == 0
                carried = _host(t)
                assert (carried[cs.n:] == FILL32).all()  # the pads behind the array
                if counted:  # the survivors' counts by their new ordinals, then zeros (after == start when nothing was removed)
                    assert np.array_equal(carried[: cs.n], after), (what, rounds, p)
                    assert not carried[m.count(): cs.n].any() or st["popped"] == 0
                else:
                    assert np.array_equal(carried[: cs.n], start)
    _set_pass(monkeypatch, None)
    g.close()


# ---- the observers -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", bb.CRAFTED)
def test_marks(name, canonical, monkeypatch):
    """Key widths: snp15 (no hi array), snp31 (a byte-wide hi), snp33 and snp59 (a wide k-mer)."""
    _need_gpu()
    cs = _case(name, canonical)
    g = cs.index()
    _check_observers(cs, g, monkeypatch)
    g.close()


# ---- pop_bubbles -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", bb.CRAFTED)
def test_pop_bubbles(name, canonical, monkeypatch):
    _need_gpu()
    cs = _case(name, canonical)
    _check_pop(cs, cs.blob, monkeypatch, what=name)
    if name == "nested":
        for counted in (False, True):
            assert [(cs.popped(counted, r)[1]["rounds"], cs.popped(counted, r)[1]["fixpoint"]) for r in (1, 2, 0)] == [(1, 0), (2, 0), (3, 1)]
        assert cs.popped(False, 1)[0] != cs.popped(False, 2)[0]
    if name in ("split", "shared", "snp31-short", "mirror1"):  # nothing is popped: the bytes stay
        assert cs.popped(True, 0)[0] == cs.blob and cs.popped(True, 0)[1]["rounds"] == 1


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["snp15", "snp33", "indel", "quad", "nested", "strands", "deep", "sized257"])
def test_python_surface_and_fresh_tally(name, canonical):
    """pop_bubbles through the method, with the counts the GPU tallied itself; the carried view equals a fresh tally of the same reads on the popped index."""
    _need_gpu()
    cs = _case(name, canonical)
    g = cs.index()
    counts, total, found = g.abundance_seqs(*nm.Graph.arrays(cs.reads))
    assert np.array_equal(_host(counts), cs.counts)
    for rounds in (1, 0):
        g.load(cs.blob)
        mine = counts.clone()
        want, st, after, m = cs.popped(True, rounds)
        got, view = g.pop_bubbles(cs.mk, mine, rounds=rounds)
        assert got == st and g.serialize() == want
        assert view.data_ptr() == mine.data_ptr() and view.numel() == st["kmers_left"]  # a view of the caller's tensor
        assert np.array_equal(_host(mine), after)
        fresh, _, _ = g.abundance_seqs(*nm.Graph.arrays(cs.reads))
        assert fresh.numel() == st["kmers_left"] and torch.equal(fresh, view)
        g.load(cs.blob)
        assert g.pop_bubbles(cs.mk, rounds=rounds) == cs.popped(False, rounds)[1]  # without counts: the stats alone
        assert g.serialize() == cs.popped(False, rounds)[0]
    if cs.mk == 2 * cs.k:  # the default: arms of at most 2 K k-mers
        g.load(cs.blob)
        assert g.pop_bubbles() == cs.popped(False, 1)[1] and g.bubble_counts()["popped"] == 0
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_bucket_kinds(canonical, monkeypatch):
    """The same set in three layouts: as built; every bucket declared a Trie; every Vec shuffled (swap_remove shows the order, and the ordinals move)."""
    _need_gpu()
    cs = _case("deep", canonical)
    built = {p: (kind, list(items)) for p, (kind, items) in cs.model.buckets.items()}
    rng = random.Random(5)
    layouts = {"built": built, "tries": {p: ("trie", sorted(items)) for p, (_, items) in built.items()},
               "shuffled": {p: (kind, rng.sample(items, len(items)) if kind == "vec" else items) for p, (kind, items) in built.items()}}
    blobs = {}
    for what, buckets in layouts.items():
        model = sm.from_buckets(cs.k, cs.pb, canonical, buckets)
        blobs[what] = cs.popped(True, 1, model)[0]
        _check_pop(cs, model.serialize(), monkeypatch, model=model, passes=(None, 64), what=what)
    assert len(set(blobs.values())) == 3


# ---- refusals, the empty index, tips first, the command line ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
def test_refusals_write_and_remove_nothing(canonical):
    _need_gpu()
    cs = _case("chain", canonical)
    nu, n, mk = cs.nu, cs.n, cs.mk
    g = cs.index()
    t, ptr = _dev_counts(cs.counts)
    untouched = _host(t).copy()
    for device in (True, False):
        for cap in (nu - 1, 0):  # a short capacity: the need is reported, the fill stays
            rc, u, got_c, got_k = _mark_raw(g, mk, cap, device, ptr, n)
            assert rc == cbl_amd.ERANGE and u == nu and (got_k == FILL).all(), (device, cap)
        for args in ((0, ptr, n), (mk, None, n), (mk, ptr, n - 1), (mk, ptr, n + 1), (mk, ptr, 0)):  # max_kmers = 0; null counts; a length that is not count()
            rc, u, got_c, got_k = _mark_raw(g, args[0], nu, device, args[1], args[2])
            assert rc == cbl_amd.EINVAL and (got_k == FILL).all(), (device, args)
    for args in ((0, ptr, n, 0), (mk, ptr, n, 1), (mk, ptr, n, 0x80000000), (mk, None, n, 0), (mk, ptr, n - 1, 0), (mk, ptr, n + 1, 0)):
        rc, st = _pop_raw(g, args[0], args[1], args[2], 1, flags=args[3])
        assert rc == cbl_amd.EINVAL and all(v == 77 for v in st.values()), args
    with pytest.raises(cbl_amd.CblxError) as e:
        g.pop_bubbles(0)
    assert e.value.code == cbl_amd.EINVAL
    assert g.serialize() == cs.blob and g.count() == n and np.array_equal(_host(t), untouched)
    # a stale array: the one from before another removal no longer has count() elements
    g.remove_seq(cs.reads[0][: cs.k + 2])
    after_removal = g.serialize()
    assert g.count() == n - 3
    rc, st = _pop_raw(g, mk, ptr, n, 1)
    assert rc == cbl_amd.EINVAL and g.serialize() == after_removal and np.array_equal(_host(t), untouched)
    g.load(cs.blob)
    rc, _ = _pop_raw(g, mk, ptr, n, 1, stats=False)  # stats may be null
    assert rc == 0 and g.serialize() == cs.popped(True, 1)[0]
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_empty_index(canonical):
    _need_gpu()
    g = cbl_amd.CBL(31, 24, canonical=canonical)
    t, ptr = _dev_counts(np.zeros(0, dtype=np.uint32))
    for device in (True, False):
        for args in ((None, 0), (ptr, 0)):
            rc, u, got_c, got_k = _mark_raw(g, 5, 0, device, *args)
            assert rc == 0 and u == 0 and got_c == (0, 0, 0) and (got_k == FILL).all()
    for rounds in (0, 1, 3):
        assert g.pop_bubbles(rounds=rounds) == dict.fromkeys(bb.STATS, 0) | {"rounds": 1, "fixpoint": 1}
        rc, st = _pop_raw(g, 5, ptr, 0, rounds)
        assert rc == 0 and st == dict.fromkeys(bb.STATS, 0) | {"rounds": 1, "fixpoint": 1}
    assert (_host(t) == FILL32).all()
    kind, counts = g.bubbles_np()
    assert kind.tolist() == [] and counts == {"bubbles": 0, "popped": 0, "popped_kmers": 0, "n_unitigs": 0}
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_tipped_before_and_after_clip(canonical):
    _need_gpu()
    cs = _case("tipped", canonical)
    g = cs.index()
    assert g.bubble_counts(cs.mk)["bubbles"] == 0 and g.pop_bubbles(cs.mk)["popped"] == 0 and g.serialize() == cs.blob
    m = rm.copy_cbl(cs.model)
    assert g.clip_tips(4) == tm.clip_model(m, 4, False, 1) and g.serialize() == m.serialize()
    st, _ = bb.pop_model(m, cs.mk, None, 0)
    assert st["popped"] == 1 and g.pop_bubbles(cs.mk, rounds=0) == st and g.serialize() == m.serialize()
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_cli_pop(canonical, tmp_path):
    _need_gpu()
    cs = _case("nested", canonical)
    path, out, reads = tmp_path / "index.cbl", tmp_path / "popped.cbl", tmp_path / "reads.fa"
    path.write_bytes(cs.blob)
    reads.write_bytes(b"".join(b">r%d\n%s\n" % (j, r) for j, r in enumerate(cs.reads)))
    base = [sys.executable, "-m", "cbl_amd", "-k", str(cs.k), "--prefix-bits", str(cs.pb), "pop", str(path)]
    for extra, counted, rounds in (([], False, 1), ([str(reads), "--rounds", "0"], True, 0)):
        r = subprocess.run(base + extra + ["-o", str(out), "--max-kmers", str(cs.mk)], env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
        assert r.returncode == 0, r.stderr
        want, st, _, _ = cs.popped(counted, rounds)
        assert out.read_bytes() == want
        assert r.stdout.decode() == "".join(f"{key}\t{st[key]}\n" for key in bb.STATS)
    assert path.read_bytes() == cs.blob
