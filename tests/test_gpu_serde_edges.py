"""The device serializer (kernels_serde.hpp, serialize_device) at every class, staging and split edge: the crafted bucket tables of
tests/serde_shapes.py are installed with install_buckets_device and every way out of the index — serialized_size, serialize, save_to_file,
serialized_body_size + write_body_at, serialize with the host emitter forced — is compared byte for byte with the closed-form model's bytes, which
tests/test_serde_shapes.py shows to be the C++ oracle's. No tolerance anywhere.

What this cannot show. The serializer has no route counter: that a bucket went through the class, the staging route or the split plan it was
crafted for rests on the restated classify / split_plan / layout of serde_shapes.py, on the constants tests/test_serde_shapes.py reads out of the
sources, and on the blob's base being a hipMalloc'd pool block (so that `mis` is the offset in the blob modulo 16). A failure names the entry the
first wrong byte falls in: prefix, kind, length, class, staged or direct, mis, and for a split Trie its sub-range lengths."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402

import build_shapes as bs  # noqa: E402  (tests/)
import serde_shapes as ss  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _install(s):
    """a fresh CBL holding the shape's table, through install_buckets_device (an index with no entries is the fresh CBL itself)"""
    g = cbl_amd.CBL(s.k, s.pb)
    if s.buckets:
        pr, ct, kd, sf = ss.arrays(s)
        dev = [torch.from_numpy(pr.view(np.int32)).cuda(), torch.from_numpy(ct.view(np.int32)).cuda(), torch.from_numpy(kd).cuda(), torch.from_numpy(sf).cuda()]
        g.install_buckets_device([(len(pr), int(ct.sum(dtype=np.uint64)), *dev)])
    return g


def _equal(got, want, s, what):
    """byte identity, or the first differing offset and the entry it falls in"""
    if got == want:
        return
    n = min(len(got), len(want))
    a, b = np.frombuffer(got, dtype=np.uint8, count=n), np.frombuffer(want, dtype=np.uint8, count=n)
    d = np.flatnonzero(a != b)
    at = int(d[0]) if len(d) else n
    pytest.fail("%s, %s: %d bytes against %d wanted, %d differ, the first at offset %d (got %s, want %s), in %s" % (
        s.name, what, len(got), len(want), len(d), at, got[at: at + 8].hex(), want[at: at + 8].hex(), ss.locate(s, at)))


def _table(g):
    p, l, kd = g.bucket_table_np()
    return {int(a): (int(b), int(c)) for a, b, c in zip(p, l, kd)}


def _check(g, s, want, tmp_path, monkeypatch, reload=True):
    what = s.name
    h = len(ss.header(len(s.buckets)))
    assert g.validate(strict=False) == 0, what
    assert _table(g) == {p: (len(items), 1 if kind == "trie" else 0) for p, (kind, items) in s.buckets.items()}, what
    assert g.serialized_size() == len(want), (what, "serialized_size")
    _equal(g.serialize(), want, s, "serialize")
    path = tmp_path / "whole.cbl"
    g.save_to_file(path)
    _equal(path.read_bytes(), want, s, "save_to_file")
    ne, nbytes = g.serialized_body_size()
    assert (ne, nbytes) == (len(s.buckets), len(want) - h), (what, "serialized_body_size")
    body = tmp_path / "body.cbl"
    with open(body, "wb") as f:
        f.write(want[:h])
        f.truncate(len(want))
    g.write_body_at(body, h)
    _equal(body.read_bytes(), want, s, "write_body_at")
    monkeypatch.setenv("CBLX_HOST_SERDE", "1")
    try:
        _equal(g.serialize(), want, s, "serialize by the host emitter")
    finally:
        monkeypatch.delenv("CBLX_HOST_SERDE")
    if reload:
        g2 = cbl_amd.CBL(s.k, s.pb)
        g2.load(want)
        _equal(g2.serialize(), want, s, "serialize of a second index that loaded the bytes")
        assert g2.checksum() == g.checksum() and g2.count() == g.count(), what
        g2.close()


def _case(case, tmp_path, monkeypatch):
    _need_gpu()
    s = ss.shape(*case)
    g = _install(s)
    assert g.consts()["bytes"] == s.by and g.consts()["suffix_bits"] == s.sb
    _check(g, s, ss.expected(s), tmp_path, monkeypatch)
    g.close()


def _ids(family):
    return [ss.case_id(c) for c in ss.FAMILIES[family]]


@pytest.mark.parametrize("case", ss.FAMILIES["lengths"], ids=_ids("lengths"))
def test_lengths_on_every_class_edge(case, tmp_path, monkeypatch):
    """Vecs and Tries of 1, 2, 31 | 32 | 33, 63 | 64 | 65, 255 | 256 | 257, 1023 | 1024 | 1025, 4095 | 4096 | 4097, 4607 | 4608 | 4609, 8191 | 8192 | 8193 words, each between
    two ordinary neighbours: the one-thread class, the three workgroup classes (a Trie of 32 words is not tiny), a split Trie, a Vec for the host."""
    _case(case, tmp_path, monkeypatch)


@pytest.mark.parametrize("case", ss.FAMILIES["patterns"], ids=_ids("patterns"))
def test_trie_value_patterns(case, tmp_path, monkeypatch):
    """In every workgroup class: consecutive integers (8192 of them: ranks up to 8192 in s_ns), elements that part as high as the width allows,
    suffix 0 and 2^SB - 1, the top byte's bits all set; nodes of exactly 1, 2, 250, 251, 255, 256 children at the root and below it; suffixes that
    differ in one byte only (byte 0, 7, 8, the top one). With BYTES = 1 the root is the leaf level."""
    _case(case, tmp_path, monkeypatch)


@pytest.mark.parametrize("case", ss.FAMILIES["stage"], ids=_ids("stage"))
def test_staging_threshold_at_every_misalignment(case, tmp_path, monkeypatch):
    """For each emitting instance and each mis 0 .. 15 a Vec within 16 bytes below STAGE - mis (staged: first and last 16-byte chunk written
    byte-wise beside the neighbours' bytes) and one within 16 bytes above (direct); for the <256, 4> instance a Trie on either side."""
    _case(case, tmp_path, monkeypatch)


@pytest.mark.parametrize("case", ss.FAMILIES["split"], ids=_ids("split"))
def test_split_tries(case, tmp_path, monkeypatch):
    """Tries cut at the root: sub-ranges of exactly 1, 1024 | 1025, 4096 | 4097, 8192 words in one bucket, top bytes 0 and the last present with a gap between,
    250 | 251 | 256 present top bytes (narrow64), and two buckets the plan finds bad through one sub-range of 8193 words, which the host emits into the
    device's body beside good split buckets and ordinary ones."""
    _case(case, tmp_path, monkeypatch)


@pytest.mark.parametrize("case", ss.FAMILIES["varints"], ids=_ids("varints"))
def test_prefix_varints(case, tmp_path, monkeypatch):
    """Buckets at prefixes 0, 250 | 251, 65535 | 65536 (PREFIX_BITS 24) and 2^PB - 1: a tiny Vec, a workgroup Vec, a workgroup Trie, a split Trie."""
    _case(case, tmp_path, monkeypatch)


@pytest.mark.parametrize("case", ss.FAMILIES["chunks"], ids=_ids("chunks"))
def test_chunk_geometry_in_one_piece(case, tmp_path, monkeypatch):
    """127 | 128 | 129 | 1000 buckets, a chunk without a workgroup entry, every long bucket in chunk 0, an index with no entries — the class lists are
    kept per chunk whether or not the bytes leave in chunks (test_chunked_hand_over sends them out that way)."""
    _case(case, tmp_path, monkeypatch)


def test_tries_on_both_sides_of_split_max(tmp_path, monkeypatch):
    """Tries of 2^21 and 2^21 + 1 words, packed: the first is listed as a split Trie and handed to the host by the plan (4 sub-ranges of 2^19 words),
    the second is listed for the host at once; both are patched into the device body between ordinary neighbours."""
    _need_gpu()
    s = ss.shape(ss.craft_split_max)
    g = _install(s)
    _check(g, s, ss.expected(s), tmp_path, monkeypatch, reload=False)
    g.close()


CHILD = r"""
import sys, ctypes as C
import numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import cbl_amd
import serde_shapes as ss
import test_gpu_serde_edges as t
tmp = %r
n = 0
for family in ("chunks", "stage", "split"):
    for case in ss.FAMILIES[family]:
        s = ss.shape(*case)
        want = ss.expected(s)
        g = t._install(s)
        got = g.serialize()
        assert got == want, (s.name, "serialize", t.first_difference(got, want, s))
        path = tmp + "/chunked.cbl"
        g.save_to_file(path)
        got = open(path, "rb").read()
        assert got == want, (s.name, "save_to_file", t.first_difference(got, want, s))
        small = np.zeros(len(want), dtype=np.uint8)  # a buffer one byte short: refused with the full size
        w = C.c_uint64(0)
        rc = g._L.cblx_serialize(g._h, small.ctypes.data_as(C.POINTER(C.c_uint8)), len(want) - 1, C.byref(w))
        assert rc == cbl_amd.ERANGE and w.value == len(want), (s.name, rc, w.value)
        g.close()
        n += 1
print("ok", n)
"""


def first_difference(got, want, s):
    n = min(len(got), len(want))
    d = np.flatnonzero(np.frombuffer(got, dtype=np.uint8, count=n) != np.frombuffer(want, dtype=np.uint8, count=n))
    at = int(d[0]) if len(d) else n
    return len(got), len(want), at, ss.locate(s, at)


def test_chunked_hand_over(tmp_path):
    """The chunk, staging and split shapes with CBLX_SERDE_CHUNK_MIN=1 (read once per process: a child started fresh, with a time limit): from 128
    buckets on the workgroup entries are emitted group of chunks by group of chunks and handed over piecewise, into a buffer and into a file; into a
    buffer one byte short cblx_serialize returns ERANGE and the full size."""
    _need_gpu()
    code = CHILD % (ROOT, os.path.join(ROOT, "tests"), str(tmp_path))
    env = dict(os.environ, CBLX_SERDE_CHUNK_MIN="1")
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=600)
    want = sum(len(ss.FAMILIES[f]) for f in ("chunks", "stage", "split"))
    assert r.returncode == 0 and "ok %d" % want in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]


def _insert_words(g, words):
    lo = torch.from_numpy(np.array([w & M64 for w in words], dtype=np.uint64).view(np.int64)).cuda()
    hb = g.consts()["hi_bytes"]
    hi = None
    if hb:
        a = np.array([w >> 64 for w in words], dtype=np.uint64)
        hi = torch.from_numpy(a.astype(np.uint8) if hb == 1 else a.view(np.int64)).cuda()
    g.insert_words_device(lo, hi, len(words))


@pytest.mark.parametrize("width", ss.STALE_WIDTHS)
def test_buckets_a_later_batch_did_not_touch(width, tmp_path, monkeypatch):
    """arena_sfx masks every suffix to SB bits because the arena slots of buckets a rebuild did not touch may still carry the full word. Here a
    first batch builds a Vec of 500 words, Tries of 2000, 6000 and 9000 words (c64, c256, c1024, split) and buckets of 1, 1, 1, 2, 17 and 33 words on prefixes whose
    top and bottom bits are set, a second batch touches other prefixes only, and the bytes are compared with the model of insert_batch. That untouched
    slots really still hold prefix bits is read from the code, not observed here: k_classify leaves a single new word "in its slot", where the
    partition put the word whole, and a later batch copies an untouched bucket as it is. The test pins the bytes of such buckets whatever their slots hold."""
    _need_gpu()
    k, pb, sb, by = ss.geom(width)
    first, second, kept = ss.craft_stale(width)
    m = ss.pyref.PyCBL(k, pb)
    g = cbl_amd.CBL(k, pb)
    for words in (first, second):
        bs.insert_batch(m, words)
        _insert_words(g, words)
    s = ss.Shape("stale/" + width, width, k, pb, sb, by, {p: (kind, list(items)) for p, (kind, items) in m.buckets.items()}, {p: "untouched" for p in kept})
    _check(g, s, bs.serialize(m), tmp_path, monkeypatch)
    g.close()


@pytest.mark.parametrize("case", [(ss.craft_patterns, "wide"), (ss.craft_split, "packed"), (ss.craft_chunks, "packed", "129")], ids=ss.case_id)
def test_serialize_again_on_the_same_context(case):
    """Twice on one context, then once more after a query: identical bytes, so the pooled scratch (size table, class lists, staging of the split
    plan, the blob itself) is reused without leftovers."""
    _need_gpu()
    s = ss.shape(*case)
    want = ss.expected(s)
    g = _install(s)
    _equal(g.serialize(), want, s, "first")
    _equal(g.serialize(), want, s, "second")
    rng = random.Random(s.name)
    g.contains_kmers([rng.getrandbits(2 * s.k) for _ in range(3000)])
    assert g.serialized_size() == len(want)
    _equal(g.serialize(), want, s, "after a query")
    g.close()
