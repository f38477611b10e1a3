"""Removal on the MI355X — remove_words_device, remove_seq(s), remove_fastx_file, remove_kmers / remove, `python -m cbl_amd remove` — against the literal
replay of tests/removal_model.py: after every operation the index bytes equal the model's, with count, num_buckets, is_empty and validate."""
import random
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd import synth  # noqa: E402
from oracle import Oracle  # noqa: E402
from oracle.pyref import CHUNK, PyCBL, params  # noqa: E402

import removal_model as rm  # noqa: E402  (tests/)
import setops_model as sm  # noqa: E402  (tests/)

ROOT = Path(__file__).resolve().parent.parent
RM_SMALL, RM_LDS = 64, 2048  # kernels_remove.hpp: table slots (length rounded up to a power of two) one wave / one workgroup keeps in LDS
LENGTHS = (1, 2, 3, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 4096, 4097)
CONFIGS = [(31, 24), (59, 28), (29, 24)]  # 68-bit words with a byte-wide hi array, 125-bit words with 97-bit suffixes, 64-bit words without a hi array
assert all(x in LENGTHS for x in (RM_SMALL, RM_SMALL + 1, RM_LDS, RM_LDS + 1))
M64 = (1 << 64) - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _gpu(m: PyCBL):
    g = cbl_amd.CBL(m.P["K"], m.P["PB"], canonical=m.canonical)
    g.load(m.serialize())
    return g


def _agrees(g, m: PyCBL, what=""):
    assert g.serialize() == m.serialize(), what
    assert g.count() == m.count() and g.num_buckets() == len(m.buckets), what
    assert g.is_empty() == (m.count() == 0), what
    assert g.validate(False) == 0, what


def _remove_words(g, words):
    """one cblx_remove_words_device call = one remove_batch"""
    hb = g.consts()["hi_bytes"]
    lo = torch.from_numpy(np.array([w & M64 for w in words], dtype=np.uint64).view(np.int64)).cuda()
    if hb == 0:
        hi = None
    elif hb == 1:
        hi = torch.from_numpy(np.array([w >> 64 for w in words], dtype=np.uint8)).cuda()
    else:
        hi = torch.from_numpy(np.array([w >> 64 for w in words], dtype=np.uint64).view(np.int64)).cuda()
    g.remove_words_device(lo, hi, len(words))


def _calls(g, m, calls, what=""):
    for i, words in enumerate(calls):
        rm.remove_batch(m, words)
        _remove_words(g, words)
        _agrees(g, m, "%s call %d" % (what, i))


# ---------------------------------------------------------------- 1: the Vec layout
_VEC = {}
KINDS = ("first_last_middle", "all_stored", "all_reverse", "all_ascending", "all_random", "every_second", "thrice_then_again", "absent_only")


def _vec_buckets(k, pb):
    """one shuffled Vec per length, each between two short neighbours that no removal names"""
    if (k, pb) not in _VEC:
        sb = params(k, pb)["SB"]
        rng = random.Random(k * 100 + pb)
        b = {}
        for i, n in enumerate(LENGTHS):
            p = 1000 + 3 * i
            b[p] = ("vec", sm.distinct(rng, n, min(sb, 60)))
            b[p - 1] = ("vec", [5, 6, 7])
            b[p + 1] = ("trie", [8, 9])
        _VEC[(k, pb)] = b
    return _VEC[(k, pb)]


def _removal_lists(kind, items, rng, sb):
    absent = [x for x in range(1, 40) if x not in items][:3]
    if kind == "first_last_middle":
        return [[items[0], items[-1], items[len(items) // 2]]]
    if kind == "all_stored":
        return [list(items)]
    if kind == "all_reverse":
        return [items[::-1]]
    if kind == "all_ascending":
        return [sorted(items)]
    if kind == "all_random":
        return [rng.sample(items, len(items))]
    if kind == "every_second":
        return [items[::2]]
    if kind == "thrice_then_again":
        x = items[len(items) // 3]
        return [[absent[0], x, x, x, absent[1]], [x, items[0]]]
    return [absent]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("k,pb", CONFIGS)
def test_vec_layout(k, pb, kind):
    _need_gpu()
    buckets = _vec_buckets(k, pb)
    sb = params(k, pb)["SB"]
    m = sm.from_buckets(k, pb, False, buckets)
    g = _gpu(m)
    rng = random.Random(7)
    per = {p: _removal_lists(kind, it, rng, sb) for p, (kd, it) in sorted(buckets.items()) if p % 3 == 1}  # the crafted Vecs, not their neighbours
    ncalls = max(len(v) for v in per.values())
    calls = [[(p << sb) | s for p, v in per.items() if c < len(v) for s in v[c]] for c in range(ncalls)]
    _calls(g, m, calls, kind)
    if kind.startswith("all_"):  # every crafted bucket left the directory, the neighbours kept their bytes
        assert set(m.buckets) == {p for p in buckets if p % 3 != 1}
        assert all(m.buckets[p] == [buckets[p][0], list(buckets[p][1])] for p in m.buckets)
    g.close()


@pytest.mark.parametrize("k,pb", CONFIGS)
def test_emptied_index_and_empty_index(k, pb):
    _need_gpu()
    sb = params(k, pb)["SB"]
    rng = random.Random(3)
    buckets = {5: ("vec", sm.distinct(rng, 70, 30)), (1 << pb) - 1: ("trie", sorted(sm.distinct(rng, 1100, 30))), 9: ("trie", [3, 4])}
    m = sm.from_buckets(k, pb, False, buckets)
    g = _gpu(m)
    everything = [(p << sb) | s for p, (_, it) in buckets.items() for s in it]
    rng.shuffle(everything)
    _calls(g, m, [everything[:600], everything[600:]], "emptying")
    assert g.is_empty() and g.serialize() == cbl_amd.CBL(k, pb).serialize()
    _calls(g, m, [everything[:10]], "empty index")
    g.insert_kmers([1, 2, 3])  # and it still takes inserts
    assert g.count() == 3
    g.close()


# ---------------------------------------------------------------- 2: the conversion of a Trie
@pytest.mark.parametrize("k,pb", CONFIGS)
def test_trie_conversion(k, pb):
    _need_gpu()
    sb = params(k, pb)["SB"]
    rng = random.Random(k)
    p, q = 70001, 70005
    W = lambda pp, xs: [(pp << sb) | x for x in xs]  # noqa: E731
    items = sorted(sm.distinct(rng, 1026, min(sb, 60)))
    x1, x2, x3 = items[10], items[500], items[700]
    absent = [x for x in range(1, 40) if x not in items][:2]
    base = {p: ("trie", items), q: ("vec", [1, 2])}
    out = []
    for call in (W(p, [x1, x2]) + W(q, [77]) + W(p, [x3]), W(p, [x1, x2, x3])):
        m = sm.from_buckets(k, pb, False, base)
        g = _gpu(m)
        _calls(g, m, [call], "1026")
        assert m.buckets[p][0] == "vec"
        out.append(g.serialize())
        g.close()
    assert out[0] != out[1]
    cases = [
        (base, [W(p, [x1])], "trie"),  # 1025 left
        ({p: ("trie", items[:1025])}, [W(p, absent)], "trie"),  # only absent words
        ({p: ("trie", items[:1024]), q: ("trie", items[:1024])}, [W(p, absent[:1])], "vec"),  # a short Trie visited by one absent word
        ({p: ("trie", items[:5]), q: ("trie", items[:5])}, [W(p, absent[:1])], "vec"),
        ({p: ("vec", items[::-1])}, [W(p, absent[:1]), W(p, [x1, x2, x3])], "vec"),  # a long Vec stays one and swaps
    ]
    for b, calls, kind in cases:
        m = sm.from_buckets(k, pb, False, b)
        g = _gpu(m)
        _calls(g, m, calls)
        assert m.buckets[p][0] == kind and (q not in b or m.buckets[q] == [b[q][0], list(b[q][1])])
        g.close()


@pytest.mark.parametrize("k,pb", CONFIGS)
def test_trie_of_5000_words(k, pb):
    _need_gpu()
    sb = params(k, pb)["SB"]
    rng = random.Random(pb)
    p, q = 3, 4
    items = sorted(sm.distinct(rng, 5000, min(sb, 60)))
    order = rng.sample(items, len(items))
    W = lambda pp, xs: [(pp << sb) | x for x in xs]  # noqa: E731
    first, then = W(p, order[:3976]), W(p, order[3976:3986])
    res = []
    for calls in ([first + W(q, [0]) + then], [first, then], [W(p, order[:4000])], [W(p, order)], [first + W(q, [0]) + then[:5] + W(q, [0]) + then[5:]]):
        m = sm.from_buckets(k, pb, False, {p: ("trie", items)})
        g = _gpu(m)
        _calls(g, m, calls, "5000")
        res.append(g.serialize())
        g.close()
    assert res[0] == res[1] == res[4] and res[2] != res[0]


# ---------------------------------------------------------------- 3: groups from reads
def _reads(seed, n, length):
    bases, offsets = synth.reads(seed, n, length)
    raw, off = bytes(np.asarray(bases, dtype=np.uint8)), [int(x) for x in np.asarray(offsets)]
    return [raw[off[i]:off[i + 1]] for i in range(n)]


def _batch(seqs):
    return np.frombuffer(b"".join(seqs), dtype=np.uint8), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)


def _seq_batches(o: Oracle, seq: bytes, k):
    """the word lists of remove_seq's remove_batch calls (src/cbl.rs:350-352), by the C++ oracle"""
    return [o.seq_words(seq[s:min(s + CHUNK + k - 1, len(seq))]) for s in range(0, len(seq) - k + 1, CHUNK)]


def _model_of(g, k, pb, canonical):
    """the index as the GPU holds it after a build (compared with the oracle in tests/test_gpu_parity.py), as a model index"""
    return sm.from_buckets(k, pb, canonical, {p: ("trie" if kd else "vec", items) for p, kd, items in g.buckets()})


def _model_remove_seqs(m, o, seqs, k):
    for s in seqs:
        for words in _seq_batches(o, s, k):
            rm.remove_batch(m, words)


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", [(31, 12), (59, 10), (29, 10)])
def test_half_of_the_reads(k, pb, canonical, tmp_path):
    _need_gpu()
    seqs = _reads(21, 2400, 100)
    o = Oracle(k, pb, canonical)
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    g.insert_seqs(*_batch(seqs))
    m = _model_of(g, k, pb, canonical)
    gone = seqs[1200:]
    # the case is about groups: some Trie converts in the middle of the batch and loses words in later groups
    sb = m.P["SB"]
    tagged = rm.groups_of([b for s in gone for b in _seq_batches(o, s, k)], sb)
    per = {}
    for i, (w, grp) in enumerate(tagged):
        per.setdefault(w >> sb, []).append((i, grp, w & ((1 << sb) - 1)))
    late = 0
    for p, (kind, items) in m.buckets.items():
        if kind == "trie" and p in per:
            eff = rm.effective_removals(items, per[p])
            gc = rm.conversion_group(kind, len(items), eff, per[p][0][1])
            late += gc is not None and any(grp > gc for _, grp, _ in eff)
    assert late >= 1
    before = g.serialize()
    _model_remove_seqs(m, o, gone, k)
    g.remove_seqs(*_batch(gone))
    _agrees(g, m, "remove_seqs")
    # the three entry points give the same bytes
    g2 = cbl_amd.CBL(k, pb, canonical=canonical)
    g2.load(before)
    for s in gone[:40]:
        g2.remove_seq(s)
    g2.remove_seqs(*_batch(gone[40:]))
    assert g2.serialize() == m.serialize()
    fa = tmp_path / "gone.fa"
    fa.write_bytes(synth.fasta_bytes(*_batch(gone)))
    g2.load(before)
    assert g2.remove_fastx_file(fa) == len(gone)
    assert g2.serialize() == m.serialize()
    # contains_seq and iter after the removal
    inside = sm.words(m)
    words = [w for s in seqs for w in o.seq_words(s)]
    flags, total, positive = g.contains_seqs(*_batch(seqs))
    want = np.fromiter((w in inside for w in words), dtype=bool, count=len(words))
    assert total == len(words) and np.array_equal(np.asarray(flags).astype(bool), want)
    expect = [o.kmer_of_word((p << sb) | s) for p in sorted(m.buckets) for s in m.buckets[p][1]]
    lo, hi = g.kmers_np()
    assert ([int(x) for x in lo] if hi is None else [int(x) | (int(y) << 64) for x, y in zip(lo, hi)]) == expect
    # the rest goes too: the index is a new index's again (src/cbl.rs:664-683, 726-760)
    g.remove_seqs(*_batch(seqs[:1200]))
    assert g.is_empty() and g.serialize() == cbl_amd.CBL(k, pb, canonical=canonical).serialize()
    g.close()
    g2.close()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", [(31, 6), (59, 8), (29, 6)])
def test_long_and_dirty_reads(k, pb, canonical):
    _need_gpu()
    rng = random.Random(k + pb)
    long_read = bytes(rng.choice(b"ACGT") for _ in range(2 * CHUNK + k + 500))  # prefix runs cross the chunk edges: two groups
    poly_a = b"A" * 3000
    dirty = bytearray(bytes(rng.choice(b"ACGTacgt") for _ in range(700)))
    for i in (5, 6, 300, 650):
        dirty[i] = ord("N")
    other = [bytes(rng.choice(b"ACGT") for _ in range(400)) for _ in range(20)]
    seqs = [long_read, poly_a, bytes(dirty)] + other
    o = Oracle(k, pb, canonical)
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    g.insert_seqs(*_batch(seqs))
    m = _model_of(g, k, pb, canonical)
    for gone in ([poly_a, bytes(dirty)], [long_read] + other[:7], [long_read, poly_a]):
        _model_remove_seqs(m, o, gone, k)
        g.remove_seqs(*_batch(gone))
        _agrees(g, m)
    g.insert_seq(other[0])  # pending inserts are applied before a removal
    g.insert_seq(long_read)
    g.remove_seq(other[0])
    g2 = cbl_amd.CBL(k, pb, canonical=canonical)
    g2.load(m.serialize())
    g2.insert_seqs(*_batch([other[0], long_read]))
    m2 = _model_of(g2, k, pb, canonical)
    _model_remove_seqs(m2, o, [other[0]], k)
    _agrees(g, m2, "insert, insert, remove")
    # insert after remove: Vecs left in swap order grow (and convert) as an index loaded from the model's bytes does
    g.insert_seqs(*_batch(seqs))
    g2.load(m2.serialize())
    g2.insert_seqs(*_batch(seqs))
    assert g.serialize() == g2.serialize()
    g.close()
    g2.close()


# ---------------------------------------------------------------- 4: remove_kmers / remove
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", CONFIGS)
def test_remove_kmers(k, pb, canonical):
    _need_gpu()
    rng = random.Random(k)
    o = Oracle(k, pb, canonical)
    kmers = [rng.getrandbits(2 * k) for _ in range(300)]
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    g.insert_kmers(kmers)
    m = _model_of(g, k, pb, canonical)

    def rc(x):
        r = 0
        for _ in range(k):
            r = (r << 2) | ((x & 3) ^ 2)
            x >>= 2
        return r

    batch = kmers[:50] + kmers[:10] + [rng.getrandbits(2 * k) for _ in range(20)] + [rc(x) for x in kmers[50:80]] + kmers[40:120]
    want = [rm.remove_word(m, o.word_of_kmer(x)) for x in batch]
    got = g.remove_kmers(batch)
    assert [bool(x) for x in got] == want
    _agrees(g, m, "remove_kmers")
    assert g.remove(kmers[200]) is True and g.remove(kmers[200]) is False
    rm.remove_word(m, o.word_of_kmer(kmers[200]))
    _agrees(g, m, "remove")
    before = g.serialize()
    with pytest.raises(cbl_amd.CblxError) as e:
        g.remove_kmers([kmers[201], 1 << (2 * k)])  # bits above 2K
    assert e.value.code == 1 and g.serialize() == before
    g.close()


# ---------------------------------------------------------------- 5: after the set operations
@pytest.mark.parametrize("k,pb", CONFIGS[:2])
def test_after_or_assign_and_xor_assign(k, pb):
    import setops_assign_model as am

    _need_gpu()
    sb = params(k, pb)["SB"]
    rng = random.Random(31)
    x = sm.distinct(rng, 2600, min(sb, 60))
    ba = {7: ("vec", x[:900]), 8: ("trie", sorted(x[:1500])), 9: ("vec", x[:1000])}
    bb = {7: ("vec", x[600:1400]), 8: ("vec", x[200:1490]), 9: ("vec", x[1000:2000])}
    W = lambda pp, xs: [(pp << sb) | s for s in xs]  # noqa: E731
    for how in ("or", "xor"):
        ma, mb = sm.from_buckets(k, pb, False, ba), sm.from_buckets(k, pb, False, bb)
        ga, gb = _gpu(ma), _gpu(mb)
        if how == "or":
            ga |= gb
            ma.merge(mb)
        else:
            ga.set_op_assign(gb, "xor")
            am.set_op_assign(ma, mb, "xor")
        _agrees(ga, ma, how)
        calls = [W(7, x[550:700]) + W(8, x[:3]) + W(9, x[990:1010]), W(8, x[1495:1500] + x[:200]) + W(7, x[:50]) + W(8, x[1400:1500])]
        _calls(ga, ma, calls, "after " + how)
        ga.close()
        gb.close()


# ---------------------------------------------------------------- 5b: the sub-batch route and device inputs
def _dev_batch(seqs):
    """bases (16-byte aligned, padded) and offsets as CUDA tensors"""
    bases, offsets = _batch(seqs)
    pad = np.zeros((-len(bases)) % 16 + 16, dtype=np.uint8)
    return torch.from_numpy(np.concatenate([bases, pad])).cuda(), torch.from_numpy(offsets.astype(np.int64)).cuda()


@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", [(31, 12), (59, 10), (29, 10)])
def test_sub_batches_equal_one_batch(k, pb, canonical, monkeypatch, tmp_path):
    """A removal larger than CBLX_BATCH_MAX_BASES is cut at sequence boundaries into sub-batches, as an insert is: same bytes as one batch and as the
    model, for host, device and file input, with a sequence longer than the cut; a short sequence in a LATER sub-batch removes nothing."""
    _need_gpu()
    rng = random.Random(k)
    seqs = [bytes(rng.choice(b"ACGT") for _ in range(n)) for n in [150] * 120 + [9000, 150, 150, 6000] + [300] * 30]
    o = Oracle(k, pb, canonical)
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    g.insert_seqs(*_batch(seqs))
    before = g.serialize()
    m = _model_of(g, k, pb, canonical)
    gone = seqs[40:140]
    _model_remove_seqs(m, o, gone, k)
    d_b, d_o = _dev_batch(gone)
    g.remove_seqs_device(d_b, d_o, len(gone))  # one batch, device tensors through the public entry
    _agrees(g, m, "one batch, device input")
    fa = tmp_path / "gone.fa"
    fa.write_bytes(synth.fasta_bytes(*_batch(gone)))
    monkeypatch.setenv("CBLX_BATCH_MAX_BASES", "5000")
    for how in ("host", "device", "file"):
        g.load(before)
        if how == "host":
            g.remove_seqs(*_batch(gone))
        elif how == "device":
            g.insert_seq(seqs[0])  # pending inserts are applied first (the read is in the index already)
            g.remove_seqs_device(d_b, d_o, len(gone))
        else:
            assert g.remove_fastx_file(fa) == len(gone)
        _agrees(g, m, "sub-batches, %s input" % how)
    # a slice of a larger batch: offsets that do not start at 0
    g.load(before)
    d_b2, d_o2 = _dev_batch(seqs)
    g.remove_seqs_device(d_b2, d_o2[40:], len(gone))
    _agrees(g, m, "sub-batches, a slice of the offsets")
    # ESHORT in a later sub-batch: nothing is removed
    g.load(before)
    bad = gone[:90] + [b"ACGTACGT"] + gone[90:]
    d_b3, d_o3 = _dev_batch(bad)
    for call in (lambda: g.remove_seqs_device(d_b3, d_o3, len(bad)), lambda: g.remove_seqs(*_batch(bad))):
        with pytest.raises(cbl_amd.CblxError) as e:
            call()
        assert e.value.code == 2 and g.serialize() == before
    g.close()


# ---------------------------------------------------------------- 6: the command line
@pytest.mark.parametrize("canonical", [False, True])
def test_cli(tmp_path, canonical):
    _need_gpu()
    k, pb = 31, 12
    seqs = _reads(5, 60, 90)
    o = Oracle(k, pb, canonical)
    fa, fb, short = tmp_path / "all.fa", tmp_path / "half.fa", tmp_path / "short.fa"
    fa.write_bytes(synth.fasta_bytes(*_batch(seqs)))
    fb.write_bytes(synth.fasta_bytes(*_batch(seqs[30:])))
    short.write_bytes(b">a\nACGT\n")
    idx, out, lst = tmp_path / "a.cbl", tmp_path / "out.cbl", tmp_path / "out.txt"
    run = lambda *a: subprocess.run([sys.executable, "-m", "cbl_amd", "-k", str(k), "--prefix-bits", str(pb)] + [str(x) for x in a], cwd=str(ROOT),  # noqa: E731
                                    capture_output=True, text=True, timeout=120)
    r = run("build", fa, "-o", idx, *(["-c"] if canonical else []))
    assert r.returncode == 0, r.stderr[-2000:]
    g = cbl_amd.CBL(k, pb, canonical=canonical)
    g.load(idx.read_bytes())
    m = _model_of(g, k, pb, canonical)
    g.close()
    _model_remove_seqs(m, o, seqs[30:], k)
    r = run("remove", idx, fb, "-o", out)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "Removing the %s%d-mers contained in %s from the index" % ("canonical " if canonical else "", k, fb) in r.stderr
    assert out.read_bytes() == m.serialize()
    r = run("count", out)
    assert r.returncode == 0 and r.stdout.split()[-1] == str(m.count())
    r = run("list", out, "-o", lst)
    assert r.returncode == 0, r.stderr[-2000:]
    sb = m.P["SB"]
    expect = [o.kmer_of_word((p << sb) | s) for p in sorted(m.buckets) for s in m.buckets[p][1]]  # CBL::iter order
    nucs = "ACTG"
    assert lst.read_text().split() == ["".join(nucs[(x >> (2 * (k - 1 - j))) & 3] for j in range(k)) for x in expect]
    bad_i, bad_r = run("insert", idx, short), run("remove", idx, short)
    assert bad_i.returncode != 0 and bad_r.returncode == bad_i.returncode


# ---------------------------------------------------------------- 7: errors leave the index alone
def test_errors():
    _need_gpu()
    k, pb = 31, 24
    g = cbl_amd.CBL(k, pb)
    seqs = _reads(2, 30, 80)
    g.insert_seqs(*_batch(seqs))
    before = g.serialize()
    L = g._L
    assert L.cblx_remove_seqs(g._h, None, None, 3) == 1
    assert L.cblx_remove_seqs_device(g._h, None, None, 3) == 1
    assert L.cblx_remove_words_device(g._h, None, None, 3) == 1
    assert L.cblx_remove_kmers(g._h, None, None, 3, None) == 1
    assert L.cblx_remove_fastx_file(g._h, None, None) == 1
    assert L.cblx_remove_seq(g._h, None, 40) == 1
    for call in (lambda: g.remove_seq(b"ACGT"), lambda: g.remove_seqs(*_batch([seqs[0], b"ACGTACGT", seqs[1]]))):
        with pytest.raises(cbl_amd.CblxError) as e:
            call()
        assert e.value.code == 2 and "smaller than K" in str(e.value)
    assert g.serialize() == before
    g.remove_seqs(*_batch([]))  # n == 0
    g.remove_kmers([])
    assert g.serialize() == before
    g.close()
