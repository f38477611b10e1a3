"""K-mer abundances on the GPU, in both forms: the tally (host and device reads), the spectrum, the unitig coverage, the tagged GFA text (device buffer,
file, descriptor), the filter under both rules and `cbl abundance`. Every expectation comes from the CPU — the oracle's enumeration of the batch and its
iteration order through tests/abundance_model.py, gfa_model's table and text, removal_model.remove_batch — never from the GPU path; every output is
pre-filled with 0xA5 and carries pad elements that must keep the fill."""
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

import abundance_model as am  # noqa: E402  (tests/)
import biunitigs_model as bm  # noqa: E402
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
FILL32, FILL64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
EDGES = (7, 8, 9, 31, 32, 33, 255, 256, 257)  # k-mers in a batch: the group, wave and workgroup edges of a QL = 8 kernel with 256 threads


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
    """An index of `flushes` (lists of reads, one flush each): the oracle's bytes and iteration order, the model index, the table and the GFA text."""

    def __init__(self, k, pb, flushes, canonical):
        self.k, self.pb, self.flushes, self.canonical = k, pb, flushes, canonical
        self.reads = [r for batch in flushes for r in batch]
        self.oracle = Oracle(k, pb, canonical)
        for batch in flushes:
            self.oracle.insert_seqs(*nm.Graph.arrays(batch))
        self.blob = self.oracle.serialize()
        self.order = self.oracle.iter_words()
        self.model = tm.model_of_words(k, pb, canonical, self.order)
        assert self.model.serialize() == self.blob
        self.kmers = nm.oracle_kmers(self.oracle)
        self.n = len(self.kmers)
        self._graph = None

    def graph(self):
        """(table, text, L lines) of the compacted graph, made when first asked for."""
        if self._graph is None:
            t = gm.walk_model(self.kmers, self.k, self.canonical)
            lt = gm.definition_model(self.kmers, self.k, self.canonical, t)
            self._graph = (t, gm.gfa_model(self.kmers, self.k, self.canonical, t, lt), gm.n_l_lines(lt, self.canonical))
        return self._graph

    def index(self, blob=None):
        g = cbl_amd.CBL(self.k, self.pb, canonical=self.canonical)
        g.load(self.blob if blob is None else blob)
        return g


def _case(name, canonical):
    key = (name, canonical)
    if key not in _cases:
        if name == "long":
            _cases[key] = Case(31, 24, [am.long_unitig_reads(31)], canonical)
        elif name in tm.CRAFTED:
            _cases[key] = Case(*tm.crafted(name)[:3], canonical)
        else:
            _cases[key] = Case(*bm.crafted(name), canonical)
    return _cases[key]


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------------------
def _dev32(values, pad=PAD):
    """A device array of the uint32 `values` and `pad` filled elements behind them (a torch int32 tensor)."""
    host = np.concatenate([np.asarray(values, dtype=np.uint32), np.full(pad, FILL32, dtype=np.uint32)])
    return torch.from_numpy(host.view(np.int32)).cuda()


def _back32(t):
    return t.cpu().numpy().view(np.uint32)


def _tally_raw(g, seqs, d_counts, n_counts, device):
    """cblx_abundance_seqs(_device) on the reads `seqs`: (status, total, found)."""
    L = cbl_amd.lib()
    bases, offsets = nm.Graph.arrays(seqs)
    tot, found = C.c_uint64(12345), C.c_uint64(12345)
    p = d_counts.data_ptr() if d_counts is not None else None
    if device:
        d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, dtype=np.uint8)])).cuda()
        d_o = torch.from_numpy(offsets.view(np.int64)).cuda()
        rc = L.cblx_abundance_seqs_device(g._h, d_b.data_ptr(), d_o.data_ptr(), len(seqs), p, n_counts, C.byref(tot), C.byref(found))
    else:
        rc = L.cblx_abundance_seqs(g._h, bases.ctypes.data, offsets.ctypes.data, len(seqs), p, n_counts, C.byref(tot), C.byref(found))
    return rc, tot.value, found.value


def _same32(got, want, what):
    m = len(want)
    bad = np.flatnonzero(got[:m] != want)
    assert not len(bad), f"{what}: wrong at (index, got, expected) {[(int(i), int(got[i]), int(want[i])) for i in bad[:8]]}"
    assert len(got) == m + PAD and (got[m:] == FILL32).all(), f"{what}: elements behind the counts were written"


def _check_tally(cs, g, order, batches, what=""):
    """Every batch through the host and the device entry into one running array each: the counts, the totals and the pad after every call."""
    enum = cs.oracle  # the enumeration does not depend on what the oracle holds
    n = len(order)
    for device in (True, False):
        want = np.zeros(n, dtype=np.uint32)
        d = _dev32(want)
        for name, batch in batches:
            want, total, found = am.tally_model(enum, batch, want, order)
            rc, t, f = _tally_raw(g, batch, d, n, device)
            assert rc == 0, (what, name, device, _err(g))
            assert (t, f) == (total, found), (what, name, device, t, f, total, found)
            _same32(_back32(d), want, f"{what} {name}, device {device}")
    return want


def _tally_batches(cs):
    named = am.tally_reads(cs.k, cs.reads)
    batches = [(name, named[name]) for name in ("far-apart", "both-strands", "dirty", "short", "only-short", "none", "miss", "poly-a")]
    # short and empty sequences between long ones of many lengths, at the head and at the tail: the compaction of the kept bases, over several workgroups
    src, mixed = max(cs.reads, key=len), [b"", b"AC"]
    for j in range(120):
        mixed += [src[j % 7: j % 7 + cs.k + j % 40], src[: j % cs.k], b""][: 1 + j % 3]
    batches.append(("interleaved", mixed + [src[: cs.k - 1]]))
    return batches + [(f"exact-{nk}", am.exact_batch(cs.k, cs.reads, nk)) for nk in EDGES]


# ---- the tally -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["edge15", "edge", "edge33", "edge59"])
def test_tally_equals_model(name, canonical):
    """Key widths: edge15 (no hi array), edge (a byte-wide hi), edge33 and edge59 (a wide k-mer)."""
    _need_gpu()
    cs = _case(name, canonical)
    g = cs.index()
    batches = _tally_batches(cs)
    for nk in EDGES:
        assert sum(len(am.enumerate_words(cs.oracle, s)) for s in dict(batches)[f"exact-{nk}"]) == nk
    want = _check_tally(cs, g, cs.order, batches, name)
    assert int(want.max()) >= 3 and int((want == 0).sum()) > 0  # repeats and k-mers never seen
    # two calls compared with one call on the concatenation
    a, b = dict(batches)["far-apart"], dict(batches)["dirty"]
    one, two = _dev32(np.zeros(cs.n)), _dev32(np.zeros(cs.n))
    r1 = _tally_raw(g, a + b, one, cs.n, True)
    r2a, r2b = _tally_raw(g, a, two, cs.n, True), _tally_raw(g, b, two, cs.n, False)
    assert r1[0] == r2a[0] == r2b[0] == 0 and r1[1:] == (r2a[1] + r2b[1], r2a[2] + r2b[2])
    assert np.array_equal(_back32(one), _back32(two))
    # the Python surface: a tensor made here, then accumulated into
    bases, offsets = nm.Graph.arrays(a)
    counts, t, f = g.abundance_seqs(bases, offsets)
    w1, t1, f1 = am.tally_model(cs.oracle, a, None, cs.order)
    assert counts.is_cuda and counts.dtype == torch.int32 and (t, f) == (t1, f1) and np.array_equal(_back32(counts), w1)
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros(16, dtype=np.uint8)])).cuda()
    same, t, f = g.abundance_seqs_device(d_b, torch.from_numpy(offsets.view(np.int64)).cuda(), len(a), counts)
    assert same is counts and (t, f) == (t1, f1) and np.array_equal(_back32(counts), 2 * w1)
    assert np.array_equal(g.abundance_histogram(counts), am.spectrum(2 * w1))
    assert g.serialize() == cs.blob and g.validate() == 0  # observers: nothing is modified or sorted
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_tally_follows_the_stored_order(canonical):
    """The deep index (PREFIX_BITS = 6) as built, with every bucket declared a Trie, and with every Vec shuffled: ordinals follow the stored order."""
    _need_gpu()
    cs = _case("deep", canonical)
    built = {p: (kind, list(items)) for p, (kind, items) in cs.model.buckets.items()}
    rng = random.Random(5)
    layouts = {"built": built, "tries": {p: ("trie", sorted(items)) for p, (_, items) in built.items()},
               "shuffled": {p: (kind, rng.sample(items, len(items)) if kind == "vec" else items) for p, (kind, items) in built.items()}}
    batches = _tally_batches(cs)
    seen = {}
    for what, buckets in layouts.items():
        model = sm.from_buckets(cs.k, cs.pb, canonical, buckets)
        order = tm.iteration_words(model)
        g = cs.index(model.serialize())
        want = _check_tally(cs, g, order, batches, what)
        assert g.serialize() == model.serialize()
        seen[what] = (tuple(order), want.tolist())
        g.close()
    assert len({o for o, _ in seen.values()}) == 3 and len({tuple(w) for _, w in seen.values()}) == 3  # three orders, three arrays
    assert len({tuple(sorted(zip(o, w))) for o, w in seen.values()}) == 1  # ... of the same count per word


@pytest.mark.parametrize("canonical", FORMS)
def test_saturation(canonical):
    _need_gpu()
    cs = _case("edge", canonical)
    g = cs.index()
    read = cs.reads[0][: cs.k + 2]  # three k-mers of the index, five times
    rank = am.ordinals(cs.order)
    hit = sorted({rank[w] for w in am.enumerate_words(cs.oracle, read)})
    assert len(hit) == 3
    before = np.full(cs.n, 7, dtype=np.uint32)
    before[hit[0]], before[hit[1]], before[hit[2]] = am.MAX - 2, am.MAX, am.MAX - 5
    want, total, found = am.tally_model(cs.oracle, [read] * 5, before, cs.order)
    assert want[hit[0]] == want[hit[1]] == want[hit[2]] == am.MAX and total == found == 15
    assert all(want[i] == 7 for i in range(cs.n) if i not in hit)  # the neighbours are exact
    for device in (True, False):
        d = _dev32(before)
        assert _tally_raw(g, [read] * 5, d, cs.n, device) == (0, total, found)
        _same32(_back32(d), want, f"saturation, device {device}")
    g.close()
    g = cbl_amd.CBL(31, 24, canonical=canonical)  # a poly-A index: one ordinal, every wave's leaders on it, from 2^32 - 3, from 0 and up to the ceiling exactly
    g.insert_seq(b"A" * 31)
    g.flush()
    for start, end in ((am.MAX - 2, am.MAX), (0, 270), (am.MAX - 270, am.MAX)):
        d = _dev32([start])
        assert _tally_raw(g, [b"A" * 300], d, 1, True) == (0, 270, 270)
        assert _back32(d).tolist() == [end] + [FILL32] * PAD
    g.close()


# ---- the spectrum ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257, 70000])
def test_spectrum(n):
    _need_gpu()
    rng = random.Random(n)
    g = cbl_amd.CBL(31, 24, canonical=False)
    g.insert_seq(nm._rand(rng, n + 30).encode())
    g.flush()
    assert g.count() == n
    vals = np.array([0, 1, 254, 255, 256, am.MAX], dtype=np.uint32)
    L = cbl_amd.lib()
    for counts in (vals[np.arange(n) % 6], vals[np.array([rng.randrange(6) for _ in range(n)])], np.full(n, 255, dtype=np.uint32), np.zeros(n, dtype=np.uint32)):
        d = _dev32(counts)
        hist = np.full(256 + PAD, FILL64, dtype=np.uint64)
        assert L.cblx_abundance_histogram(g._h, d.data_ptr(), n, hist.ctypes.data_as(C.POINTER(C.c_uint64))) == 0, _err(g)
        assert np.array_equal(hist[:256], am.spectrum(counts)) and (hist[256:] == FILL64).all() and int(hist[:256].sum()) == n
        _same32(_back32(d), counts, "the spectrum reads only")
    g.close()


# ---- coverage and the tagged text ------------------------------------------------------------------------------------------------------------------
def _kc_raw(g, d_counts, n_counts, cap, device, array=True):
    """cblx_unitig_coverage(_device) on an output of cap + PAD filled words: (status, U, kc)."""
    L = cbl_amd.lib()
    u = C.c_uint64(12345)
    host = np.full(cap + PAD, FILL64, dtype=np.uint64)
    dev = torch.from_numpy(host.view(np.int64)).cuda() if device else None
    ptr = (dev.data_ptr() if device else host.ctypes.data) if array else None
    p = d_counts.data_ptr() if d_counts is not None else None
    rc = (L.cblx_unitig_coverage_device if device else L.cblx_unitig_coverage)(g._h, p, n_counts, ptr, cap, C.byref(u))
    return rc, u.value, (dev.cpu().numpy().view(np.uint64) if device else host)


def _tagged_raw(g, d_counts, n_counts, cap):
    d_buf = torch.full((cap + PAD,), FILL, dtype=torch.uint8, device="cuda")
    out = [C.c_uint64(12345) for _ in range(3)]
    p = d_counts.data_ptr() if d_counts is not None else None
    rc = cbl_amd.lib().cblx_gfa_tagged_text_device(g._h, p, n_counts, d_buf.data_ptr(), cap, *[C.byref(c) for c in out])
    return rc, tuple(c.value for c in out), d_buf.cpu().numpy()  # (bytes, unitigs, L lines)


def _check_coverage_and_text(cs, g, counts, monkeypatch, passes=PASSES):
    table, text, lines = cs.graph()
    nu = len(table["head"])
    kc = am.kc_model(table, counts)
    want_kc = np.array(kc, dtype=np.uint64)
    tagged, ln_only = am.tagged_text(text, table, cs.k, kc), am.tagged_text(text, table, cs.k, None)
    assert am.untag(tagged)[0] == am.untag(ln_only)[0] == text
    d = _dev32(counts)
    plain_before = g.gfa_text_np().tobytes()
    assert plain_before == text
    for p in passes:
        _set_pass(monkeypatch, p)
        for device in (True, False):
            rc, u, got = _kc_raw(g, d, cs.n, nu, device)
            assert rc == 0 and u == nu, (_err(g), p, device)
            assert np.array_equal(got[:nu], want_kc) and (got[nu:] == FILL64).all(), (p, device)
        for want, dc, m in ((tagged, d, cs.n), (ln_only, None, 0)):
            rc, sizes, buf = _tagged_raw(g, dc, m, len(want))
            assert rc == 0, _err(g)
            assert sizes == (len(want), nu, lines), (p, sizes)
            assert buf[: len(want)].tobytes() == want, f"tagged text, pass {p}, counts {dc is not None}"
            assert (buf[len(want):] == FILL).all(), f"pass {p}: bytes behind the text were written"
    _set_pass(monkeypatch, None)
    for device in (True, False):
        rc, u, got = _kc_raw(g, d, cs.n, 0, device, array=False)  # null only: the count
        assert rc == 0 and u == nu and (got == FILL64).all()
        rc, u, got = _kc_raw(g, d, cs.n, nu + 2, device)  # a capacity above the need
        assert rc == 0 and u == nu and np.array_equal(got[:nu], want_kc) and (got[nu:] == FILL64).all()
    t = d[: cs.n]
    assert np.array_equal(g.unitig_coverage_np(t), want_kc) and g.unitig_coverage_np(t).dtype == np.uint64
    dk = g.unitig_coverage_device(t)
    assert dk.is_cuda and dk.dtype == torch.int64 and np.array_equal(dk.cpu().numpy().view(np.uint64), want_kc)
    assert g.gfa_tagged_text_np(t).tobytes() == tagged and g.gfa_tagged_text_np().tobytes() == ln_only
    assert g.gfa_tagged_text_device(t) == (len(tagged), nu, lines) and g.gfa_tagged_text_device() == (len(ln_only), nu, lines)
    _same32(_back32(d), counts, "the counts are only read")
    assert g.gfa_text_np().tobytes() == plain_before  # the untagged text is byte-identical before and after
    assert g.serialize() == cs.blob and g.validate() == 0
    return tagged, ln_only


@pytest.mark.parametrize("canonical", FORMS)
def test_coverage_and_tagged_text_digits(canonical, monkeypatch, tmp_path):
    """Counts preset so that kc hits 9, 10, 99, 100, ... 10^12 - 1, 10^12 on chosen unitigs, 300 k-mers at 2^32 - 1 (13 digits), and unitigs of one k-mer."""
    _need_gpu()
    cs = _case("long", canonical)
    table = cs.graph()[0]
    counts, kc = am.digit_counts(table)
    assert set(am.DIGIT_TARGETS) <= set(kc) and max(kc) == 300 * am.MAX and 1 in table["length"].tolist() and 0 in kc
    g = cs.index()
    tagged, ln_only = _check_coverage_and_text(cs, g, counts, monkeypatch)
    assert b"\tKC:i:1288490188500\n" in tagged and b"\tKC:i:1000000000000\n" in tagged and b"\tKC:i:9\n" in tagged and b"KC" not in ln_only
    # files and descriptors
    d = _dev32(counts)[: cs.n]
    nu, lines = len(kc), cs.graph()[2]
    for chunk in (5, 997, 0):  # chunks that split lines (one smaller than any line); the default
        path = tmp_path / f"graph-{chunk}.gfa"
        assert g.gfa_tagged_to_file(path, d, chunk) == (nu, lines, len(tagged))
        assert path.read_bytes() == tagged
    assert g.gfa_tagged_to_file(tmp_path / "ln.gfa") == (nu, lines, len(ln_only)) and (tmp_path / "ln.gfa").read_bytes() == ln_only
    r, w = os.pipe()
    got = []

    def reader():
        with os.fdopen(r, "rb") as f:
            got.append(f.read())

    t = threading.Thread(target=reader)
    t.start()
    try:
        res = g.gfa_tagged_to_fd(w, d, 1000)
    finally:
        os.close(w)
        t.join()
    assert res == (nu, lines, len(tagged)) and got[0] == tagged
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["dense", "cycles", "hairpin", "at"])
def test_coverage_and_tagged_text_crafted(name, canonical, monkeypatch):
    _need_gpu()
    cs = _case(name, canonical)
    rng = random.Random(len(name))
    vals = [0, 0, 1, 2, 9, 10, 255, 65536, am.MAX]
    counts = np.array([vals[rng.randrange(len(vals))] for _ in range(cs.n)], dtype=np.uint32)
    g = cs.index()
    _check_coverage_and_text(cs, g, counts, monkeypatch, passes=(None, 1000) if name == "dense" else PASSES)
    g.close()


# ---- the filter ------------------------------------------------------------------------------------------------------------------------------------
def _check_filter(cs, blob, model, counts, mc, unitigs, monkeypatch, passes=(None, 64), what=""):
    m = rm.copy_cbl(model)
    st = am.filter_model(m, counts, mc, unitigs)
    want = m.serialize()
    g = cs.index(blob)
    for p in passes:
        _set_pass(monkeypatch, p)
        g.load(blob)
        d = _dev32(counts)
        got = g.abundance_filter(d[: len(counts)], mc, unitigs=unitigs)
        assert got == st, (what, unitigs, mc, p, got, st)
        assert g.serialize() == want, (what, unitigs, mc, p)
        assert g.count() == m.count() and g.num_buckets() == len(m.buckets) and g.is_empty() == (m.count() == 0) and g.validate(False) == 0
        _same32(_back32(d), counts, "the filter reads only")
    _set_pass(monkeypatch, None)
    g.close()
    return st, m


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["edge15", "edge", "edge33", "edge59", "islands"])
def test_filter(name, canonical, monkeypatch):
    """Bytes and stats equal to the model: counts at min_count - 1 and min_count; kc at min_count * length - 1 and exactly min_count * length."""
    _need_gpu()
    cs = _case(name, canonical)
    table = cs.graph()[0]
    for mc in (1, 3):
        kcounts, ucounts = am.kmer_edge_counts(cs.n, mc), am.unitig_edge_counts(table, mc)
        for counts in (kcounts, ucounts):
            for unitigs in (False, True):
                st, m = _check_filter(cs, cs.blob, cs.model, counts, mc, unitigs, monkeypatch, what=name)
                if mc == 3 and (counts is ucounts) == unitigs:
                    assert 0 < st["removed_kmers"] < cs.n
        ln, kc = table["length"].tolist(), am.kc_model(table, ucounts)
        sel, gone = am.select_model(ucounts, mc, table)
        kept = sorted(set(range(len(ln))) - set(gone))
        assert gone and kept and all(kc[u] in (mc * ln[u] - 1, 0) for u in gone) and all(kc[u] == mc * ln[u] for u in kept)  # one below the bound, and on it
    # an index that empties, under either rule
    for unitigs in (False, True):
        st, m = _check_filter(cs, cs.blob, cs.model, np.full(cs.n, 4, dtype=np.uint32), 5, unitigs, monkeypatch, passes=(None,), what="empties")
        assert st["kmers_left"] == 0 and m.serialize() == cbl_amd.CBL(cs.k, cs.pb, canonical=canonical).serialize()


@pytest.mark.parametrize("canonical", FORMS)
def test_filter_bucket_kinds(canonical, monkeypatch):
    """The three load forms of `deep`: a bucket that empties, Tries that shrink into Vecs, Vecs that lose by swap_remove."""
    _need_gpu()
    cs = _case("deep", canonical)
    built = {p: (kind, list(items)) for p, (kind, items) in cs.model.buckets.items()}
    rng = random.Random(5)
    layouts = {"built": built, "tries": {p: ("trie", sorted(items)) for p, (_, items) in built.items()},
               "shuffled": {p: (kind, rng.sample(items, len(items)) if kind == "vec" else items) for p, (kind, items) in built.items()}}
    blobs = set()
    for what, buckets in layouts.items():
        model = sm.from_buckets(cs.k, cs.pb, canonical, buckets)
        table = am.table_of(model)
        order = tm.iteration_words(model)
        sb = model.P["SB"]
        # the k-mer rule: everything in one bucket goes, and of the other buckets some words that are not the last of their Vec
        first = min(model.buckets)
        counts = np.array([0 if (w >> sb) == first or i % 5 == 1 else 2 for i, w in enumerate(order)], dtype=np.uint32)
        st, m = _check_filter(cs, model.serialize(), model, counts, 2, False, monkeypatch, what=what)
        assert first not in m.buckets and st["removed_kmers"] > len(model.buckets[first][1])  # a bucket that empties
        blobs.add(m.serialize())
        st, m = _check_filter(cs, model.serialize(), model, am.unitig_edge_counts(table, 2), 2, True, monkeypatch, what=what)
        assert 0 < st["removed_unitigs"] < st["unitigs"]
    assert len(blobs) == 3


# ---- refusals, the empty index, the command line ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("canonical", FORMS)
def test_refusals_write_and_remove_nothing(canonical, tmp_path):
    _need_gpu()
    cs = _case("edge", canonical)
    nu = len(cs.graph()[0]["head"])
    g = cs.index()
    L = cbl_amd.lib()
    counts = np.full(cs.n, 2, dtype=np.uint32)
    batch = [cs.reads[0]]
    for off in (-1, 1):  # n_counts off by one, in every call
        m = cs.n + off
        d = _dev32(counts, pad=PAD + 1)  # (the allocation covers n + 1)
        for device in (True, False):
            assert _tally_raw(g, batch, d, m, device) == (cbl_amd.EINVAL, 0, 0)
            rc, u, got = _kc_raw(g, d, m, nu, device)
            assert rc == cbl_amd.EINVAL and (got == FILL64).all()
        hist = np.full(256, FILL64, dtype=np.uint64)
        assert L.cblx_abundance_histogram(g._h, d.data_ptr(), m, hist.ctypes.data_as(C.POINTER(C.c_uint64))) == cbl_amd.EINVAL and (hist == FILL64).all()
        rc, sizes, buf = _tagged_raw(g, d, m, 1 << 16)
        assert rc == cbl_amd.EINVAL and (buf == FILL).all()
        r, w = os.pipe()  # the descriptor form: refused before a byte is written
        try:
            with pytest.raises(cbl_amd.CblxError) as e:
                g._gfa_sizes("gfa_tagged_to_fd", d.data_ptr(), m, w, 0)
        finally:
            os.close(w)
        with os.fdopen(r, "rb") as f:
            assert e.value.code == cbl_amd.EINVAL and f.read() == b""
        target = tmp_path / f"refused{off}.gfa"
        with pytest.raises(cbl_amd.CblxError) as e:
            g._gfa_sizes("gfa_tagged_to_file", d.data_ptr(), m, os.fsencode(target), 0)
        assert e.value.code == cbl_amd.EINVAL and not target.exists()  # a refused call does not create the file
        st = cbl_amd.AbundanceStats(*([77] * 6))
        for flags in (0, cbl_amd.ABUNDANCE_UNITIGS):
            assert L.cblx_abundance_filter(g._h, d.data_ptr(), m, 3, flags, C.byref(st)) == cbl_amd.EINVAL
        assert all(getattr(st, name) == 77 for name in am.STATS)
        assert _back32(d)[: cs.n].tolist() == counts.tolist()
    d = _dev32(counts)
    st = cbl_amd.AbundanceStats(*([77] * 6))
    assert L.cblx_abundance_filter(g._h, d.data_ptr(), cs.n, 0, 0, C.byref(st)) == cbl_amd.EINVAL  # min_count = 0
    assert L.cblx_abundance_filter(g._h, d.data_ptr(), cs.n, 3, 2, C.byref(st)) == cbl_amd.EINVAL  # unknown flag bits
    assert L.cblx_abundance_filter(g._h, d.data_ptr(), cs.n, 3, 0x80000001, C.byref(st)) == cbl_amd.EINVAL
    assert all(getattr(st, name) == 77 for name in am.STATS)
    with pytest.raises(cbl_amd.CblxError) as e:
        g.abundance_filter(d[: cs.n], 0)
    assert e.value.code == cbl_amd.EINVAL
    for device in (True, False):
        for cap in (nu - 1, 0):  # a short capacity: the need is reported, the fill stays
            rc, u, got = _kc_raw(g, d, cs.n, cap, device)
            assert rc == cbl_amd.ERANGE and u == nu and (got == FILL64).all(), (device, cap)
    text = am.tagged_text(cs.graph()[1], cs.graph()[0], cs.k, am.kc_model(cs.graph()[0], counts))
    rc, sizes, buf = _tagged_raw(g, d, cs.n, len(text) - 1)
    assert rc == cbl_amd.ERANGE and sizes == (len(text), nu, cs.graph()[2]) and (buf == FILL).all()
    with pytest.raises(cbl_amd.CblxError) as e:
        g.gfa_tagged_to_fd(-1, d[: cs.n])
    assert e.value.code == cbl_amd.EINVAL
    target = tmp_path / "no" / "such" / "graph.gfa"
    with pytest.raises(cbl_amd.CblxError):
        g.gfa_tagged_to_file(target, d[: cs.n])
    assert not target.exists() and not target.parent.exists()
    assert g.serialize() == cs.blob and g.count() == cs.n  # nothing was removed
    assert L.cblx_abundance_filter(g._h, d.data_ptr(), cs.n, 3, 0, None) == 0 and g.count() == 0  # stats may be null (every count is 2)
    g.close()
    # An even K is refused where the index is created (K must be odd), in either form: no index of an even K exists for the unitig rule's own refusal to
    # meet; the k-mer rule runs on a canonical index of every crafted case above
    for canon in FORMS:
        with pytest.raises(cbl_amd.CblxError) as e:
            cbl_amd.CBL(30, 24, canonical=canon)
        assert e.value.code == cbl_amd.EINVAL


@pytest.mark.parametrize("canonical", FORMS)
def test_a_stale_array_is_refused_after_a_removal(canonical):
    _need_gpu()
    cs = _case("edge", canonical)
    g = cs.index()
    counts = am.kmer_edge_counts(cs.n, 3)
    d = _dev32(counts)
    st = g.abundance_filter(d[: cs.n], 3)
    assert 0 < st["removed_kmers"] < cs.n
    with pytest.raises(cbl_amd.CblxError) as e:
        g.abundance_filter(d[: cs.n], 3)
    assert e.value.code == cbl_amd.EINVAL and g.count() == st["kmers_left"]
    g.insert_seq(nm._rand(random.Random(1), 40).encode())  # pending inserts are applied first: the guard sees them
    assert _tally_raw(g, [cs.reads[0]], _dev32(np.zeros(st["kmers_left"])), st["kmers_left"], True)[0] == cbl_amd.EINVAL
    g.close()


@pytest.mark.parametrize("canonical", FORMS)
def test_empty_index(canonical):
    _need_gpu()
    g = cbl_amd.CBL(31, 24, canonical=canonical)
    read = nm._rand(random.Random(2), 100).encode()
    for device in (True, False):
        assert _tally_raw(g, [read, b"ACG"], None, 0, device) == (0, 70, 0)  # tallies nothing: found = 0
        assert _tally_raw(g, [], None, 0, device) == (0, 0, 0)
        assert _tally_raw(g, [read], _dev32([]), 1, device)[0] == cbl_amd.EINVAL
        rc, u, got = _kc_raw(g, None, 0, 4, device)
        assert rc == 0 and u == 0 and (got == FILL64).all()
    counts, t, f = g.abundance_seqs(*nm.Graph.arrays([read]))
    assert counts.numel() == 0 and (t, f) == (70, 0)
    assert g.abundance_histogram(counts).tolist() == [0] * 256
    assert g.unitig_coverage_np(counts).tolist() == [] and g.gfa_tagged_text_np(counts).tobytes() == gm.HEADER == g.gfa_tagged_text_np().tobytes()
    for unitigs in (False, True):
        assert g.abundance_filter(counts, 3, unitigs=unitigs) == dict.fromkeys(am.STATS, 0)
    g.close()


def _fasta(path, reads):
    path.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(reads)))


@pytest.mark.parametrize("canonical", FORMS)
def test_cli_abundance(canonical, tmp_path):
    _need_gpu()
    cs = _case("cascade", canonical)
    index, out, gfa = tmp_path / "index.cbl", tmp_path / "solid.cbl", tmp_path / "graph.gfa"
    index.write_bytes(cs.blob)
    rng = random.Random(11)
    files = [cs.reads + cs.reads[:2] + [nm._rand(rng, 60).encode()], [r[3:] for r in cs.reads[:2]] + [bytes(cs.reads[0]).lower()]]
    for j, reads in enumerate(files):
        _fasta(tmp_path / f"reads{j}.fa", reads)
    counts, total, found = None, 0, 0
    for reads in files:
        counts, t, f = am.tally_model(cs.oracle, reads, counts, cs.order)
        total, found = total + t, found + f
    from cbl_amd.__main__ import abundance_report

    hist = am.spectrum(counts)
    head = "".join(line + "\n" for line in abundance_report(total, found, hist)[0])
    base = [sys.executable, "-m", "cbl_amd", "-k", str(cs.k), "--prefix-bits", str(cs.pb), "abundance", str(index)] + [str(tmp_path / f"reads{j}.fa") for j in range(2)]
    r = subprocess.run(base, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == head and f"total\t{total}\nfound\t{found}\n" in head
    table, text, _ = cs.graph()
    mc = 3
    for unitigs in (False, True):
        extra = ["--hist", "--gfa", str(gfa), "--min-count", str(mc), "-o", str(out)] + (["--unitigs"] if unitigs else [])
        r = subprocess.run(base + extra, env=dict(os.environ), capture_output=True, cwd=str(ROOT), timeout=300)
        assert r.returncode == 0, r.stderr
        m = rm.copy_cbl(cs.model)
        st = am.filter_model(m, counts, mc, unitigs)
        assert 0 < st["removed_kmers"] < cs.n
        want = head + "".join(f"{j}\t{v}\n" for j, v in enumerate(hist.tolist())) + "".join(f"{key}\t{st[key]}\n" for key in am.STATS)
        assert r.stdout.decode() == want
        assert out.read_bytes() == m.serialize()
        assert gfa.read_bytes() == am.tagged_text(text, table, cs.k, am.kc_model(table, counts))  # the index as loaded
    assert index.read_bytes() == cs.blob
