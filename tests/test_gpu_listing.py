"""Reading an index out of the GPU: k_export_range behind cblx_export_kmers_range / cblx_list_range (host and device outputs), the chunked
stream of cblx_list_to_file / cblx_list_to_fd and CBL.iter(chunk), k_bucket_nodes behind buckets_nodes, and the `list` / `repartition`
commands. Every expectation is the CPU oracle's iteration order (Oracle.iter_words + kmer_of_word) turned into text by tests/listing_model.py,
or — after operations the oracle lacks — the stored order of g.buckets() through the same word -> k-mer -> text; never the GPU's own list."""

import os
import subprocess
import sys
import threading
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd import synth  # noqa: E402
from oracle import Oracle, pyref  # noqa: E402

import listing_model as lm  # noqa: E402  (tests/)
import query_shapes as qs  # noqa: E402  (tests/)

ROOT = Path(__file__).resolve().parents[1]
M64 = (1 << 64) - 1
FILL = 0xA5
FILL64 = int.from_bytes(bytes([FILL]) * 8, "little")

# name -> how it is built. LINE = K + 1: 16, 32, 46 (the crafted buckets of tests/query_shapes.py: Vec and Trie, wide suffixes, k-mers above
# 64 bits) and 10, 60 (reads: many buckets, a Trie longer than one wave takes in k_bucket_nodes).
SHAPES = {"15-6": "edge", "31-3-a": "edge", "45-6": "edge", "9-4-reads": (9, 4, 1500, 100), "59-28-reads": (59, 28, 400, 250)}
NODES_WAVE_MAX = 8192  # kernels_list.hpp: longer Tries go to the workgroup kernel


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _insert_words(g, words):
    lo = torch.from_numpy(np.array([w & M64 for w in words], dtype=np.uint64).view(np.int64)).cuda()
    hb = g.consts()["hi_bytes"]
    hi = None
    if hb:
        a = np.array([w >> 64 for w in words], dtype=np.uint64)
        hi = torch.from_numpy(a.astype(np.uint8) if hb == 1 else a.view(np.int64)).cuda()
    g.insert_words_device(lo, hi, len(words))


class Built:
    """An index on the GPU and what the oracle says it lists, computed once per process and left unchanged by the tests."""

    def __init__(self, name):
        how = SHAPES[name]
        if how == "edge":
            s = qs.shape(qs.EDGE_SHAPES[name])
            self.k, self.pb = s.k, s.pb
            self.g, o = cbl_amd.CBL(s.k, s.pb, canonical=s.canonical), Oracle(s.k, s.pb, s.canonical)
            _insert_words(self.g, s.resident)
            o.insert_words(s.resident)
        else:
            self.k, self.pb, nreads, L = how
            self.g, o = cbl_amd.CBL(self.k, self.pb), Oracle(self.k, self.pb)
            b, off = synth.reads(5, nreads, L)
            self.g.insert_seqs(b, off)
            o.insert_seqs(b, off)
        self.name, self.oracle = name, o
        self.sb = pyref.params(self.k, self.pb)["SB"]
        self.words = o.iter_words()
        self.kmers = [o.kmer_of_word(w) for w in self.words]
        self.count, self.line = len(self.kmers), self.k + 1
        self.lo = np.array([x & M64 for x in self.kmers], dtype=np.uint64)
        self.hi = np.array([x >> 64 for x in self.kmers], dtype=np.uint64)
        self.text = lm.text(self.kmers, self.k)
        self.lines = np.frombuffer(self.text, dtype=np.uint8).reshape(self.count, self.line)
        # element where every bucket begins
        self.starts = [0] + [i for i in range(1, self.count) if self.words[i] >> self.sb != self.words[i - 1] >> self.sb]
        assert self.g.count() == self.count


_built = {}


def built(name) -> Built:
    _need_gpu()
    if name not in _built:
        _built[name] = Built(name)
    return _built[name]


def _ranges(b: Built):
    """(first, n): the empty and the one-element range, the ends, the whole, around three bucket starts with lengths on both sides of a wave
    and of a workgroup, and three whole buckets."""
    c = b.count
    out = [(0, 0), (0, 1), (c, 5), (c - 1, 5), (0, c), (3, 0)]
    st = b.starts
    picked = sorted({st[1], st[len(st) // 2], st[-1]}) if len(st) > 1 else [0]
    for s in picked:
        for first in (s - 1, s, s + 1):
            if 0 <= first <= c:
                out += [(first, n) for n in (1, 2, 63, 64, 65, 255, 256, 257)]
    if len(st) >= 4:
        i = max(0, len(st) // 2 - 1)
        i = min(i, len(st) - 4)
        out.append((st[i], st[i + 3] - st[i]))
    return out


def _written(b: Built, first, n):
    return max(0, min(n, b.count - first))


# ---- ranges ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_ranges_into_host_buffers(name):
    """Every range gives the slice of the oracle's order, packed and as text, and nothing is written behind the returned length."""
    b = built(name)
    g, wide = b.g, b.k > 31
    for first, n in _ranges(b):
        w = _written(b, first, n)
        lo = np.full(n + 3, FILL64, dtype=np.uint64)
        hi = np.full(n + 3, FILL64, dtype=np.uint64)
        assert g.export_kmers_range(first, n, lo, hi) == w, (first, n)
        assert (lo[:w] == b.lo[first : first + w]).all() and (hi[:w] == b.hi[first : first + w]).all(), (first, n)
        assert (lo[w:] == FILL64).all() and (hi[w:] == FILL64).all(), (first, n)
        if not wide:
            lo.fill(FILL64)
            assert g.export_kmers_range(first, n, lo, None) == w and (lo[:w] == b.lo[first : first + w]).all() and (lo[w:] == FILL64).all(), (first, n)
        buf = np.full(n * b.line + 7, FILL, dtype=np.uint8)
        assert g.list_range(first, n, buf) == w * b.line, (first, n)
        assert buf[: w * b.line].tobytes() == b.text[first * b.line : (first + w) * b.line], (first, n)
        assert (buf[w * b.line :] == FILL).all(), (first, n)
        lo2, hi2 = g.kmers_np(first, n)
        assert (lo2 == b.lo[first : first + w]).all() and (hi2 is None) == (not wide), (first, n)
        assert (g.list_np(first, n) == b.lines[first : first + w]).all(), (first, n)


@pytest.mark.parametrize("name", list(SHAPES))
def test_range_errors(name):
    b = built(name)
    g, L = b.g, b.g._L
    lo = np.full(8, FILL64, dtype=np.uint64)
    buf = np.full(8 * b.line, FILL, dtype=np.uint8)
    for call in (lambda: g.export_kmers_range(b.count + 1, 1, lo, lo.copy()), lambda: g.list_range(b.count + 1, 1, buf), lambda: g.kmers_np(b.count + 1, 1),
                 lambda: g.export_kmers_range(b.count + 1, 0, lo, lo.copy())):
        with pytest.raises(cbl_amd.CblxError) as e:
            call()
        assert e.value.code == cbl_amd.EINVAL
    assert (lo == FILL64).all() and (buf == FILL).all()
    # a short buffer: the need is reported, nothing is written
    import ctypes as C

    need = C.c_uint64(0)
    rc = L.cblx_list_range(g._h, 1, 5, buf.ctypes.data, 5 * b.line - 1, C.byref(need))
    assert rc == cbl_amd.ERANGE and need.value == 5 * b.line and (buf == FILL).all()
    d = torch.full((8 * b.line,), FILL, dtype=torch.uint8, device="cuda")
    need = C.c_uint64(0)
    rc = L.cblx_list_range_device(g._h, 1, 5, d.data_ptr(), 5 * b.line - 1, C.byref(need))
    assert rc == cbl_amd.ERANGE and need.value == 5 * b.line and bool((d == FILL).all())
    if b.k > 31:  # k-mers above 64 bits need the hi array
        with pytest.raises(cbl_amd.CblxError) as e:
            g.export_kmers_range(0, 4, lo, None)
        assert e.value.code == cbl_amd.EINVAL and (lo == FILL64).all()
        dl = torch.zeros(8, dtype=torch.int64, device="cuda")
        with pytest.raises(cbl_amd.CblxError) as e:
            g.export_kmers_range_device(0, 4, dl, None)
        assert e.value.code == cbl_amd.EINVAL


@pytest.mark.parametrize("name", list(SHAPES))
def test_ranges_into_device_tensors(name):
    """The device variants write the same elements; the text goes to a 16-byte aligned base and, wherever the line length allows it, ends off a
    16-byte boundary with the bytes behind it untouched."""
    b = built(name)
    g = b.g
    fill64 = FILL64 - (1 << 64)  # as int64
    odd_tail = 0
    for first, n in _ranges(b):
        w = _written(b, first, n)
        d_lo = torch.full((n + 3,), fill64, dtype=torch.int64, device="cuda")
        d_hi = torch.full((n + 3,), fill64, dtype=torch.int64, device="cuda")
        assert g.export_kmers_range_device(first, n, d_lo, d_hi) == w, (first, n)
        lo, hi = d_lo.cpu().numpy().view(np.uint64), d_hi.cpu().numpy().view(np.uint64)
        assert (lo[:w] == b.lo[first : first + w]).all() and (hi[:w] == b.hi[first : first + w]).all(), (first, n)
        assert (lo[w:] == FILL64).all() and (hi[w:] == FILL64).all(), (first, n)
        cap = n * b.line + 40
        d = torch.full((cap,), FILL, dtype=torch.uint8, device="cuda")
        assert d.data_ptr() % 16 == 0
        assert g.list_range_device(first, n, d, cap) == w * b.line, (first, n)
        got = d.cpu().numpy()
        assert got[: w * b.line].tobytes() == b.text[first * b.line : (first + w) * b.line], (first, n)
        assert (got[w * b.line :] == FILL).all(), (first, n)
        odd_tail += (w * b.line) % 16 != 0
    assert odd_tail or b.line % 16 == 0


# ---- streaming ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["31-3-a", "45-6"])
@pytest.mark.parametrize("chunk", ["1", "7", "255", "256", "257", "4097", "count", "count+1", "0"])
def test_list_to_file_at_every_chunk_seam(name, chunk, tmp_path):
    b = built(name)
    c = {"count": b.count, "count+1": b.count + 1}.get(chunk)
    c = int(chunk) if c is None else c
    out = tmp_path / "list.txt"
    out.write_bytes(b"stale content that must go")
    assert b.g.list_to_file(out, c) == b.count
    assert out.read_bytes() == b.text


@pytest.mark.parametrize("chunk", [1, 0])
def test_list_of_an_empty_index(chunk, tmp_path):
    _need_gpu()
    g = cbl_amd.CBL(31, 24)
    out = tmp_path / "empty.txt"
    out.write_bytes(b"stale")
    assert g.list_to_file(out, chunk) == 0 and out.read_bytes() == b""
    assert g.list_np().shape == (0, 32) and list(g.iter()) == [] and g.buckets_nodes() == [] and g.buckets_node_count() == {}
    lo, hi = g.kmers_np(0, 10)
    assert len(lo) == 0 and hi is None
    g.close()


@pytest.mark.parametrize("name,chunk", [("31-3-a", 1000), ("45-6", 0)])
def test_list_to_fd_on_a_pipe(name, chunk):
    b = built(name)
    r, w = os.pipe()
    got = []

    def reader():
        with os.fdopen(r, "rb") as f:
            got.append(f.read())

    t = threading.Thread(target=reader)
    t.start()
    try:
        n = b.g.list_to_fd(w, chunk)
    finally:
        os.close(w)
        t.join()
    assert n == b.count and got[0] == b.text


def test_list_to_fd_reports_a_failed_write(tmp_path):
    b = built("31-3-a")
    fd = os.open(tmp_path / "ro.txt", os.O_RDONLY | os.O_CREAT, 0o644)  # not open for writing: write() fails with EBADF
    try:
        with pytest.raises(cbl_amd.CblxError) as e:
            b.g.list_to_fd(fd, 100)
    finally:
        os.close(fd)
    assert "Failed to write the list" in str(e.value)
    with pytest.raises(cbl_amd.CblxError):
        b.g.list_to_file(tmp_path / "no" / "such" / "dir.txt")
    assert b.g.list_np(0, 2).tobytes() == b.text[: 2 * b.line]  # the index still lists


@pytest.mark.parametrize("name,chunk", [("31-3-a", 1), ("31-3-a", 1000), ("45-6", 1000), ("45-6", 1 << 22)])
def test_iter_in_chunks(name, chunk):
    b = built(name)
    assert list(b.g.iter(chunk=chunk)) == b.kmers
    if chunk == 1000:
        assert list(b.g.iter()) == b.kmers and list(b.g) == b.kmers
        it = b.g.iter(chunk=3)
        assert [next(it) for _ in range(7)] == b.kmers[:7]


@pytest.mark.parametrize("name", list(SHAPES))
def test_kmers_np_without_arguments_is_the_whole_index_export(name):
    import ctypes as C

    b = built(name)
    lo = np.zeros(b.count, dtype=np.uint64)
    hi = np.zeros(b.count, dtype=np.uint64)
    got = C.c_uint64(0)
    assert b.g._L.cblx_export_kmers(b.g._h, lo.ctypes.data, hi.ctypes.data, b.count, C.byref(got)) == 0 and got.value == b.count
    lo2, hi2 = b.g.kmers_np()
    assert (lo2 == lo).all() and (lo == b.lo).all() and (hi == b.hi).all()
    assert (hi2 is None) if b.k <= 31 else (hi2 == hi).all()


# ---- after mutation ---------------------------------------------------------------------------------------------------------
def _stored_text(g, k, pb):
    """The list of an index from its stored buckets: word -> k-mer (the oracle's revert_necklace_pos) -> text."""
    o = Oracle(k, pb)
    sb = pyref.params(k, pb)["SB"]
    kmers = [o.kmer_of_word((p << sb) | s) for p, _, sfx in g.buckets() for s in sfx]
    return kmers, lm.text(kmers, k)


def test_list_after_remove_xor_insert(tmp_path):
    """An index that went through remove_seqs (Tries shrunk to Vecs), `^=` (Vecs grown past 1024 words) and an insert lists exactly its stored
    buckets; the oracle has neither operation, so the stored order comes from g.buckets() and only word -> k-mer -> text is compared."""
    _need_gpu()
    k, pb = 15, 6
    ba, oa = synth.reads(7, 1500, 150)
    bb, ob = synth.reads(8, 1500, 150)
    a, other = cbl_amd.CBL(k, pb), cbl_amd.CBL(k, pb)
    a.insert_seqs(ba, oa)
    other.insert_seqs(bb, ob)
    before = {int(p): (int(n), int(kd)) for p, n, kd in zip(*a.bucket_table_np())}
    cut = 200 * 150
    a.remove_seqs(ba[cut:], oa[200:] - np.uint64(cut))
    shrunk = {int(p): (int(n), int(kd)) for p, n, kd in zip(*a.bucket_table_np())}
    assert any(before[p][1] == lm.TRIE and kd == lm.VEC for p, (n, kd) in shrunk.items()), "no Trie came out of the removal as a Vec"
    a.set_op_assign(other, "xor")
    a.insert_seq(ba[cut : cut + 20].tobytes())  # six k-mers of a removed read: a batch that meets a Vec of more than 1024 words would make it a Trie
    table = {int(p): (int(n), int(kd)) for p, n, kd in zip(*a.bucket_table_np())}
    assert any(kd == lm.VEC and n > 1024 for n, kd in table.values()), "no long Vec"
    assert any(kd == lm.TRIE for n, kd in table.values())
    kmers, text = _stored_text(a, k, pb)
    assert len(kmers) == a.count()
    out = tmp_path / "mut.txt"
    assert a.list_to_file(out, 5000) == len(kmers) and out.read_bytes() == text
    assert list(a.iter(chunk=7777)) == kmers
    mid = len(kmers) // 2
    assert a.list_np(mid - 100, 300).tobytes() == text[(mid - 100) * (k + 1) : (mid + 200) * (k + 1)]
    nbytes = a.consts()["bytes"]
    assert a.buckets_nodes() == [(p, lm.bucket_nodes(kd, sfx, nbytes)) for p, kd, sfx in a.buckets()]
    a.close()
    other.close()


# ---- node statistics ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SHAPES))
def test_buckets_nodes_of_every_bucket(name):
    b = built(name)
    g = b.g
    nbytes = g.consts()["bytes"]
    buckets = g.buckets()
    got = g.buckets_nodes()
    assert [p for p, _ in got] == [p for p, _ in g.buckets_sizes()] == [p for p, _, _ in buckets]
    lengths = [len(s) for _, _, s in buckets]
    named = {1, 1024, 1025, max(lengths)}
    for (p, nodes), (_, kind, sfx) in zip(got, buckets):
        want = lm.bucket_nodes(kind, sfx, nbytes)
        assert nodes == want, f"bucket of prefix {p}, length {len(sfx)}{' (a named length)' if len(sfx) in named else ''}, kind {kind}: {nodes} nodes, the model counts {want}"
        if kind == lm.TRIE and len(sfx) <= 20000:
            assert want == lm.trie_nodes_plain(sfx, nbytes)
    assert sum(n for (_, n), (_, kind, _) in zip(got, buckets) if kind == lm.VEC) == sum(len(s) for _, kind, s in buckets if kind == lm.VEC)
    want_count = {}
    for _, n in got:
        want_count[n] = want_count.get(n, 0) + 1
    assert g.buckets_node_count() == dict(sorted(want_count.items()))
    if name in ("15-6", "45-6"):
        assert {1, 1024, 1025} <= set(lengths)
    if name == "9-4-reads":
        assert any(kind == lm.TRIE and len(s) > NODES_WAVE_MAX for _, kind, s in buckets), "no Trie long enough for the workgroup kernel"


def test_nodes_of_a_trie_of_more_than_2_21_words():
    """One bucket of 2^21 + 5 ascending words at K = 31 / PREFIX_BITS = 24 (six suffix bytes): the workgroup loop of k_bucket_nodes_long. The
    expectation is the closed form in numpy: 6 + the sum of the top differing byte index of neighbours."""
    _need_gpu()
    k, pb, sb = 31, 24, 44
    n = (1 << 21) + 5
    rng = np.random.default_rng(11)
    sfx = np.unique(rng.integers(0, 1 << sb, size=n + 4096, dtype=np.uint64))[:n]
    assert len(sfx) == n
    d = sfx[1:] ^ sfx[:-1]
    want = 6 + int(sum((d >= np.uint64(1 << (8 * j))).sum() for j in range(1, 6)))
    assert want == lm.trie_nodes([int(x) for x in sfx[:3000]], 6) + int(sum((d[2999:] >= np.uint64(1 << (8 * j))).sum() for j in range(1, 6)))
    prefix = 0x123456
    # 68-bit words: the upper four bits of the prefix go to the hi bytes
    lo = torch.from_numpy(((np.uint64(prefix & 0xFFFFF) << np.uint64(sb)) | sfx).view(np.int64)).cuda()
    hi = torch.full((n,), prefix >> 20, dtype=torch.uint8, device="cuda")
    g = cbl_amd.CBL(k, pb)
    assert g.consts()["hi_bytes"] == 1 and g.consts()["bytes"] == 6
    g.insert_words_device(lo, hi, n)
    assert g.buckets_sizes() == [(prefix, n)] and g.bucket_table_np()[2].tolist() == [lm.TRIE]
    assert g.buckets_nodes() == [(prefix, want)]
    g.close()


# ---- the command line -------------------------------------------------------------------------------------------------------
def test_cli_list_and_repartition(tmp_path):
    b = built("45-6")
    idx, out = tmp_path / "a.cbl", tmp_path / "list.txt"
    b.g.save_to_file(idx)
    env = dict(os.environ, PYTHONPATH=str(ROOT) + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = lambda *a: subprocess.run([sys.executable, "-m", "cbl_amd", "-k", str(b.k), "--prefix-bits", str(b.pb)] + [str(x) for x in a], cwd=str(ROOT),  # noqa: E731
                                    env=env, capture_output=True, timeout=300)
    r = run("list", idx, "-o", out)
    assert r.returncode == 0, r.stderr[-2000:]
    assert out.read_bytes() == b.text and r.stdout == b"" and f"Listing {b.k}-mers contained in {idx}".encode() in r.stderr
    r = run("list", idx)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == b.text
    r = run("repartition", idx)
    assert r.returncode == 0, r.stderr[-2000:]
    nbytes = b.g.consts()["bytes"]
    table = [(p, len(s), kind, lm.bucket_nodes(kind, s, nbytes)) for p, kind, s in b.g.buckets()]
    lines, summary = lm.repartition_report(b.pb, table)
    assert r.stderr.decode("utf-8").splitlines()[-len(lines):] == lines
    assert r.stdout.decode().split() == summary.split()
    empty = tmp_path / "empty.cbl"
    g = cbl_amd.CBL(b.k, b.pb)
    g.save_to_file(empty)
    g.close()
    r = run("repartition", empty)
    assert r.returncode == 0, r.stderr[-2000:]
    lines, summary = lm.repartition_report(b.pb, [])
    assert r.stderr.decode("utf-8").splitlines()[-len(lines):] == lines and r.stdout.decode().split() == summary.split()
