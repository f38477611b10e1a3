"""Per-sequence query tallies on the GPU: contains_seqs_counts, contains_seqs_counts_device, query_fastx_file_counts, matching_seqs
and `query --per-record`, on the batches of tests/query_counts_shapes.py (tests/test_query_counts_model.py shows on the CPU what they
hold). Every expectation comes from the CPU oracle or the shapes module, never from the GPU path; every output array is pre-filled
with 0xA5A5A5A5, so an entry that is not written shows."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

import query_counts_shapes as qc  # noqa: E402  (tests/)
import query_shapes as qs  # noqa: E402  (tests/)

ROOT = Path(__file__).resolve().parent.parent
JOIN_ENV = "CBLX_QUERY_JOIN_MIN"
FILL = 0xA5A5A5A5
M64 = (1 << 64) - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _routes(monkeypatch):
    """The per-query kernel (small batches), then the join forced for every batch."""
    for join in (None, "1"):
        if join is None:
            monkeypatch.delenv(JOIN_ENV, raising=False)
        else:
            monkeypatch.setenv(JOIN_ENV, join)
        yield "join" if join else "per query"
    monkeypatch.delenv(JOIN_ENV, raising=False)


def _device_batch(bases, offsets):
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros((-len(bases)) % 16 + 16, np.uint8)])).cuda()
    d_o = torch.from_numpy(np.asarray(offsets, dtype=np.uint64).astype(np.int64)).cuda()
    return d_b, d_o


def _filled(n):
    return torch.full((n,), FILL - (1 << 32), dtype=torch.int32, device="cuda")


def _u32(t):
    return t.cpu().numpy().view(np.uint32)


def _same(got, want, names, what):
    got = np.asarray(got)
    assert got.dtype == np.uint32 and got.shape == want.shape, (what, got.dtype, got.shape)
    bad = np.flatnonzero(got != want)
    if len(bad):
        pytest.fail(f"{what}: {len(bad)} wrong of {len(want)}; (sequence, name, got, expected): "
                    f"{[(int(i), names[i] if names else None, int(got[i]), int(want[i])) for i in bad[:8]]}")


def _host_counts(g, bases, offsets):
    """contains_seqs_counts through the raw ABI into pre-filled arrays."""
    n = len(offsets) - 1
    total, positive = np.full(n, FILL, dtype=np.uint32), np.full(n, FILL, dtype=np.uint32)
    tot, pos = cbl_amd.C.c_uint64(0), cbl_amd.C.c_uint64(0)
    g._chk(g._L.cblx_contains_seqs_counts(g._h, bases.ctypes.data, offsets.ctypes.data, n, total.ctypes.data, positive.ctypes.data,
                                          cbl_amd.C.byref(tot), cbl_amd.C.byref(pos)))
    return total, positive, tot.value, pos.value


def _gpu_index(b, k, pb, canonical):
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    g.insert_seqs(*qc.as_arrays(qc.resident_seqs(b)))
    return g


# ---- 1. every shape batch, every word class, both flag routes -----------------------------------------------------------------
@pytest.mark.parametrize("k,pb,canonical", qc.CONFIGS)
def test_counts_of_every_shape(k, pb, canonical, monkeypatch):
    _need_gpu()
    b, o, want = qc.case(k, pb, canonical)
    g = _gpu_index(b, k, pb, canonical)
    blob = g.serialize()
    assert blob == o.serialize()
    d_b, d_o = _device_batch(b.bases, b.offsets)
    n = len(b.seqs)
    for how in _routes(monkeypatch):
        total, positive, tot, pos = _host_counts(g, b.bases, b.offsets)
        _same(total, want.total, b.names, f"contains_seqs_counts total, {how}")
        _same(positive, want.positive, b.names, f"contains_seqs_counts positive, {how}")
        tallies = g.contains_seqs(b.bases, b.offsets, flags=False)[1:]
        assert (tot, pos) == tallies == (int(total.sum(dtype=np.uint64)), int(positive.sum(dtype=np.uint64))), how
        t2, p2 = g.contains_seqs_counts(b.bases, b.offsets)
        assert np.array_equal(t2, want.total) and np.array_equal(p2, want.positive), how
        d_t, d_p = g.contains_seqs_counts_device(d_b, d_o, n, _filled(n), _filled(n))
        _same(_u32(d_t), want.total, b.names, f"contains_seqs_counts_device total, {how}")
        _same(_u32(d_p), want.positive, b.names, f"contains_seqs_counts_device positive, {how}")
    assert g.serialize() == blob and g.validate() == 0  # a query changes nothing
    g.close()


# ---- 2. resident buckets on both sides of the join's classes, cut into reads --------------------------------------------------
def test_counts_of_reads_at_the_join_class_edges(monkeypatch):
    """The "15-6" edge shape of tests/query_shapes.py (buckets of JOIN_FULL_MAX - 1 .. + 1 and JOIN_TAB_MAX - 1 .. + 2 words among others),
    its genome cut into reads of K + 20 bases: k-mer j of read r is k-mer 35 r + j of the genome (clean bases, not canonical)."""
    _need_gpu()
    s = qs.shape(qs.EDGE_SHAPES["15-6"])
    lengths = {bk.length for bk in s.buckets.values()}
    assert {qs.JOIN_FULL_MAX, qs.JOIN_FULL_MAX + 1, qs.JOIN_TAB_MAX, qs.JOIN_TAB_MAX + 1} <= lengths
    L = s.k + 20
    nreads = len(s.genome) // L
    assert nreads > 3000
    bases = np.frombuffer(s.genome, dtype=np.uint8)[: nreads * L].copy()
    offsets = np.arange(nreads + 1, dtype=np.uint64) * L
    per = L - s.k + 1
    exp = s.expected.astype(np.uint32)
    want_pos = np.array([exp[r * L: r * L + per].sum() for r in range(nreads)], dtype=np.uint32)
    want_tot = np.full(nreads, per, dtype=np.uint32)
    assert 0 < int(want_pos.sum()) < int(want_tot.sum())
    g, o = cbl_amd.CBL(s.k, s.pb), Oracle(s.k, s.pb)
    lo = torch.from_numpy(np.array([w & M64 for w in s.resident], dtype=np.uint64).view(np.int64)).cuda()
    assert g.consts()["hi_bytes"] == 0
    g.insert_words_device(lo, None, len(s.resident))
    o.insert_words(s.resident)
    assert g.serialize() == o.serialize()
    d_b, d_o = _device_batch(bases, offsets)
    for how in _routes(monkeypatch):
        total, positive, tot, pos = _host_counts(g, bases, offsets)
        _same(total, want_tot, None, f"total, {how}")
        _same(positive, want_pos, None, f"positive, {how}")
        assert (tot, pos) == (nreads * per, int(want_pos.sum(dtype=np.uint64))), how
        d_t, d_p = g.contains_seqs_counts_device(d_b, d_o, nreads, _filled(nreads), _filled(nreads))
        _same(_u32(d_t), want_tot, None, f"device total, {how}")
        _same(_u32(d_p), want_pos, None, f"device positive, {how}")
    g.close()


# ---- 3. the contract ---------------------------------------------------------------------------------------------------------
def test_contract_cases(monkeypatch):
    _need_gpu()
    k, pb = 31, 24
    b, o, want = qc.case(k, pb, False)
    n = len(b.seqs)
    d_b, d_o = _device_batch(b.bases, b.offsets)
    # an empty index: the totals are right, nothing is found
    e = cbl_amd.CBL(k, pb)
    for how in _routes(monkeypatch):
        total, positive, tot, pos = _host_counts(e, b.bases, b.offsets)
        _same(total, want.total, b.names, f"empty index total, {how}")
        assert not positive.any() and (tot, pos) == (int(want.total.sum(dtype=np.uint64)), 0), how
        d_t, d_p = e.contains_seqs_counts_device(d_b, d_o, n, _filled(n), _filled(n))
        _same(_u32(d_t), want.total, b.names, f"empty index device total, {how}")
        assert not _u32(d_p).any(), how
    e.close()
    g = _gpu_index(b, k, pb, False)
    # n == 0: a no-op
    t0, p0 = g.contains_seqs_counts(b.bases[:0], np.zeros(1, dtype=np.uint64))
    assert len(t0) == len(p0) == 0
    d_t, d_p = _filled(4), _filled(4)
    g.contains_seqs_counts_device(d_b, d_o, 0, d_t, d_p)
    assert (_u32(d_t) == FILL).all() and (_u32(d_p) == FILL).all()
    # one sequence of K - 1 bases: ESHORT, nothing is queried, the outputs are untouched (host and device)
    short_seqs = b.seqs[:3] + [b.seqs[3][: k - 1]] + b.seqs[4:8]
    sb, so = qc.as_arrays(short_seqs)
    with pytest.raises(cbl_amd.CblxError) as ei:
        _host_counts(g, sb, so)
    assert ei.value.code == cbl_amd.ESHORT and "smaller than K" in str(ei.value)
    total, positive = np.full(8, FILL, dtype=np.uint32), np.full(8, FILL, dtype=np.uint32)
    rc = g._L.cblx_contains_seqs_counts(g._h, sb.ctypes.data, so.ctypes.data, 8, total.ctypes.data, positive.ctypes.data, None, None)
    assert rc == cbl_amd.ESHORT and (total == FILL).all() and (positive == FILL).all()
    sd_b, sd_o = _device_batch(sb, so)
    d_t, d_p = _filled(8), _filled(8)
    with pytest.raises(cbl_amd.CblxError) as ei:
        g.contains_seqs_counts_device(sd_b, sd_o, 8, d_t, d_p)
    assert ei.value.code == cbl_amd.ESHORT and (_u32(d_t) == FILL).all() and (_u32(d_p) == FILL).all()
    # a slice of a larger buffer: offsets[0] > 0 (and not 16-byte aligned), on the host and on the device
    a, z = next(i for i in range(3, 12) if int(b.offsets[i]) % 16), 40
    for how in _routes(monkeypatch):
        total, positive, tot, pos = _host_counts(g, b.bases, b.offsets[a: z + 1].copy())
        _same(total, want.total[a:z], b.names[a:z], f"slice total, {how}")
        _same(positive, want.positive[a:z], b.names[a:z], f"slice positive, {how}")
        d_t, d_p = g.contains_seqs_counts_device(d_b, d_o[a: z + 1].clone(), z - a, _filled(z - a), _filled(z - a))
        _same(_u32(d_t), want.total[a:z], b.names[a:z], f"device slice total, {how}")
        _same(_u32(d_p), want.positive[a:z], b.names[a:z], f"device slice positive, {how}")
        # tensors the call allocates itself, and a flag tensor as well: the flags are those of contains_seqs
        d_t, d_p = g.contains_seqs_counts_device(d_b, d_o, n)
        assert d_t.shape == d_p.shape == (n,) and d_t.is_cuda
        _same(_u32(d_p), want.positive, b.names, f"allocated tensors, {how}")
        nk = len(want.flags)
        d_f = torch.full((nk + 5,), 0xA5, dtype=torch.uint8, device="cuda")
        d_t, d_p = g.contains_seqs_counts_device(d_b, d_o, n, _filled(n), _filled(n), d_flags=d_f)
        _same(_u32(d_t), want.total, b.names, f"with flags total, {how}")
        _same(_u32(d_p), want.positive, b.names, f"with flags positive, {how}")
        flags = d_f.cpu().numpy()
        assert (flags[nk:] == 0xA5).all() and int(flags[:nk].max()) <= 1, how
        host_flags = g.contains_seqs(b.bases, b.offsets)[0]
        assert np.array_equal(flags[:nk].astype(bool), host_flags) and np.array_equal(host_flags, want.flags), how
    # only one of the two arrays
    total = np.full(n, FILL, dtype=np.uint32)
    g._chk(g._L.cblx_contains_seqs_counts(g._h, b.bases.ctypes.data, b.offsets.ctypes.data, n, total.ctypes.data, None, None, None))
    assert np.array_equal(total, want.total)
    positive = np.full(n, FILL, dtype=np.uint32)
    g._chk(g._L.cblx_contains_seqs_counts(g._h, b.bases.ctypes.data, b.offsets.ctypes.data, n, None, positive.ctypes.data, None, None))
    assert np.array_equal(positive, want.positive)
    g.close()


# ---- 4. the file path ----------------------------------------------------------------------------------------------------------
def _write_fasta(path, seqs, width=70):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b">r%d some text\n" % i)
            for a in range(0, len(s), width):
                f.write(s[a: a + width] + b"\n")


def _write_fastq(path, seqs):
    with open(path, "wb") as f:
        for i, s in enumerate(seqs):
            f.write(b"@r%d\n" % i + s + b"\n+\n" + b"I" * len(s) + b"\n")


FLUSH_BYTES = 30_000  # of ~180 000 bases: the records reach the device in six flushes or more, the long sequence in one of its own

_FILE_CHILD = r"""
import sys
sys.path.insert(0, %(root)r)
import numpy as np
import cbl_amd
C = cbl_amd.C
want = np.load(%(want)r)
g = cbl_amd.CBL.load_from_file(%(index)r, %(k)d, %(pb)d)
blob = g.serialize()
for path in (%(fa)r, %(fq)r):
    assert g.count_fastx_records(path) == want.shape[1]
    total, positive = g.query_fastx_file_counts(path)
    assert total.dtype == positive.dtype == np.uint32
    assert np.array_equal(total, want[0]) and np.array_equal(positive, want[1]), (path, np.flatnonzero(total != want[0])[:8], np.flatnonzero(positive != want[1])[:8])
    assert g.query_fastx_file(path) == (want.shape[1], int(want[0].sum()), int(want[1].sum()))
    # a capacity that is too small: ERANGE, the record count comes back, nothing is written past the capacity
    cap = want.shape[1] - 7
    rt, rp = np.full(want.shape[1], 0xA5A5A5A5, dtype=np.uint32), np.full(want.shape[1], 0xA5A5A5A5, dtype=np.uint32)
    nrec, tot, pos = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = g._L.cblx_query_fastx_file_counts(g._h, path.encode(), rt.ctypes.data, rp.ctypes.data, cap, C.byref(nrec), C.byref(tot), C.byref(pos))
    assert rc == cbl_amd.ERANGE and nrec.value == want.shape[1], (rc, nrec.value)
    assert (rt[cap:] == 0xA5A5A5A5).all() and (rp[cap:] == 0xA5A5A5A5).all()
    # both arrays NULL: cblx_query_fastx_file
    rc = g._L.cblx_query_fastx_file_counts(g._h, path.encode(), None, None, 0, C.byref(nrec), C.byref(tot), C.byref(pos))
    assert (rc, nrec.value, tot.value, pos.value) == (0, want.shape[1], int(want[0].sum()), int(want[1].sum()))
assert g.serialize() == blob and g.validate() == 0
print("ok")
"""


@pytest.fixture(scope="module")
def file_case(tmp_path_factory):
    k, pb = 31, 24
    b, o, want = qc.case(k, pb, False)
    d = tmp_path_factory.mktemp("query_counts")
    fa, fq, index, npy = d / "batch.fa", d / "batch.fq", d / "index.cbl", d / "want.npy"
    _write_fasta(fa, b.seqs)
    _write_fastq(fq, b.seqs)
    with open(index, "wb") as f:
        f.write(o.serialize())
    np.save(npy, np.stack([want.total, want.positive]))
    assert len(b.bases) >= 3 * FLUSH_BYTES
    return dict(k=k, pb=pb, fa=str(fa), fq=str(fq), index=str(index), want=str(npy), root=str(ROOT), dir=d, expect=want)


def test_file_counts_across_flushes(file_case):
    """A multi-line FASTA and a FASTQ of the shape batch, read with a queue bound that takes the records to the device in many
    flushes (a fresh process: the bound is read once)."""
    _need_gpu()
    code = _FILE_CHILD % file_case
    env = dict(os.environ, CBLX_INGEST_FLUSH_BYTES=str(FLUSH_BYTES))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_cli_per_record(file_case):
    """`query --per-record OUT`: one line per record, `ordinal<TAB>queried<TAB>positive`; stderr and the summary line as without it."""
    _need_gpu()
    want = file_case["expect"]
    out = file_case["dir"] / "per_record.tsv"
    env = dict(os.environ, CBLX_INGEST_FLUSH_BYTES=str(FLUSH_BYTES))
    base = [sys.executable, "-m", "cbl_amd", "-k", str(file_case["k"]), "--prefix-bits", str(file_case["pb"]), "query", file_case["index"], file_case["fa"]]
    plain = subprocess.run(base, env=env, capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    per = subprocess.run(base + ["--per-record", str(out)], env=env, capture_output=True, text=True, cwd=str(ROOT), timeout=300)
    assert plain.returncode == 0 and per.returncode == 0, plain.stderr + per.stderr
    assert per.stderr == plain.stderr and per.stdout == plain.stdout
    assert plain.stdout.split() == [str(int(want.total.sum())), str(int(want.positive.sum()))]
    assert f"# queries: {int(want.total.sum())}" in plain.stderr and "# positive queries: %d (" % int(want.positive.sum()) in plain.stderr
    lines = out.read_text().splitlines()
    assert lines == [f"{i}\t{t}\t{p}" for i, (t, p) in enumerate(zip(want.total.tolist(), want.positive.tolist()))]


# ---- 5. screening -------------------------------------------------------------------------------------------------------------
def test_matching_seqs_thresholds():
    _need_gpu()
    import math

    k, pb = 31, 24
    b, o, want = qc.case(k, pb, False)
    g = _gpu_index(b, k, pb, False)
    t, p = want.total.tolist(), want.positive.tolist()
    for frac, hits in ((0.5, 0), (1.0, 0), (0.0, 0), (0.0, 1), (0.0, 11), (0.3, 2049), (1e-4, 0)):
        mask = g.matching_seqs(b.bases, b.offsets, min_fraction=frac, min_hits=hits)
        assert mask.dtype == bool and mask.tolist() == [ti > 0 and pi >= max(hits, math.ceil(frac * ti)) for ti, pi in zip(t, p)], (frac, hits)
    half = g.matching_seqs(b.bases, b.offsets, min_fraction=0.5)
    assert half[::2].all() and half.sum() < len(half)  # the resident sequences match, not everything does
    # a record without a k-mer never matches, whatever the thresholds
    assert cbl_amd.CBL.matching(np.array([0, 0, 3]), np.array([0, 0, 0]), min_fraction=0.0, min_hits=0).tolist() == [False, False, True]
    g.close()
