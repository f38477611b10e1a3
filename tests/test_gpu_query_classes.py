"""The read side at every bucket-class edge: k_contains (per query) and k_query_join (the join) against resident buckets of an exact
length and kind, k_export_kmers (CBL::iter) on Tries, long Vecs and wide k-mers. The buckets and their queries come from
tests/query_shapes.py; tests/test_query_shapes.py shows on the CPU that every named length, kind and border is there. Every
expectation is a Python set of words or the CPU oracle, never the GPU path."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import Oracle  # noqa: E402

import query_shapes as qs  # noqa: E402  (tests/)

M64 = (1 << 64) - 1
JOIN_ENV = "CBLX_QUERY_JOIN_MIN"


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


def _pair(s, words):
    g, o = cbl_amd.CBL(s.k, s.pb, canonical=s.canonical), Oracle(s.k, s.pb, s.canonical)
    _insert_words(g, words)
    o.insert_words(words)
    return g, o


def _table(g):
    p, l, kd = g.bucket_table_np()
    return {int(a): (int(b), int(c)) for a, b, c in zip(p, l, kd)}


def _same_flags(s, got, what):
    """got == s.expected, or a message that names the buckets of the first wrong answers: (prefix, length, kind, rank of the key)."""
    got = np.asarray(got).astype(bool)
    assert got.shape == s.expected.shape, (what, got.shape, s.expected.shape)
    bad = np.flatnonzero(got != s.expected)
    if len(bad):
        where = [(int(i), bool(s.expected[i]), qs.bucket_of(s, s.words[i])) for i in bad[:8]]
        pytest.fail(f"{what}: {len(bad)} wrong flags of {len(got)}; (index, expected, (prefix, length, kind, rank)): {where}")


def _query_every_way(g, s, monkeypatch):
    """The genome through contains_seqs (flags, tallies), contains_seqs_device (without and with a flag tensor) and contains_seq, by
    the per-query kernel and by the forced join."""
    want = s.expected
    tot, pos = len(want), int(want.sum())
    bases = np.frombuffer(s.genome, dtype=np.uint8)
    offsets = np.array([0, len(bases)], dtype=np.uint64)
    d_b = torch.from_numpy(np.concatenate([bases, np.zeros((-len(bases)) % 16 + 16, np.uint8)])).cuda()
    d_o = torch.from_numpy(offsets.astype(np.int64)).cuda()
    d_f = torch.empty(len(bases), dtype=torch.uint8, device="cuda")
    for join in (None, "1"):
        if join is None:
            monkeypatch.delenv(JOIN_ENV, raising=False)
        else:
            monkeypatch.setenv(JOIN_ENV, join)
        how = "join" if join else "per query"
        flags, t, p = g.contains_seqs(bases, offsets)
        _same_flags(s, flags, f"contains_seqs flags, {how}")
        assert (t, p) == (tot, pos), how
        assert g.contains_seqs(bases, offsets, flags=False)[1:] == (tot, pos), how
        assert g.contains_seqs_device(d_b, d_o, 1) == (tot, pos), how
        d_f.fill_(0xA5)  # every flag is written, none is left over from an earlier call
        assert g.contains_seqs_device(d_b, d_o, 1, d_f, len(bases)) == (tot, pos), how
        got = d_f[:tot].cpu().numpy()
        assert int(got.max()) <= 1, how
        _same_flags(s, got, f"contains_seqs_device flags, {how}")
    _same_flags(s, g.contains_seq_np(s.genome), "contains_seq")
    monkeypatch.delenv(JOIN_ENV, raising=False)


def _probe_kmers(g, o, s, words, what):
    rs = set(s.resident)
    got = g.contains_kmers([o.kmer_of_word(w) for w in words])
    bad = [(qs.bucket_of(s, w), w in rs) for w, f in zip(words, got.tolist()) if f != (w in rs)]
    assert not bad, f"{what}: {len(bad)} wrong of {len(words)}; ((prefix, length, kind, rank), expected): {bad[:8]}"


# ---- a. the join's classes and the per-query kernel at the exact edges ------------------------------------------------------
@pytest.mark.parametrize("name", list(qs.EDGE_SHAPES))
def test_membership_at_every_bucket_class_edge(name, monkeypatch):
    """Buckets of exactly 1, 8, 9, 1024 words (Vecs) and 1025, 2729, 2730, 2731, 4094, 4095, 4096, 4097 words (Tries), as far as the
    shape has prefixes for them: the `full` table up to JOIN_FULL_MAX, the tag table up to JOIN_TAB_MAX, the binary search beyond; the
    (QL + 1)-ary search and the QL-wide scan of k_contains. The whole genome is queried: hits, misses below, between and above the
    elements of every bucket, and prefixes without a bucket."""
    _need_gpu()
    s = qs.shape(qs.EDGE_SHAPES[name])
    g, o = _pair(s, s.resident)
    assert g.serialize() == o.serialize()
    c = g.consts()
    assert c["suffix_bits"] == s.sb
    assert _table(g) == {b.prefix: (b.length, b.kind) for b in s.buckets.values()}
    assert sorted(b.length for b in s.buckets.values() if b.edges == ("outer" if name.endswith("-b") else "inner")) == sorted(qs.EDGE_SHAPES[name][3])
    _query_every_way(g, s, monkeypatch)
    borders = [w for b in s.buckets.values() for w in qs.border_words(b)]
    _probe_kmers(g, o, s, borders, "contains_kmers on the borders")
    assert [g.contains(o.kmer_of_word(w)) for w in borders[:8]] == [w in set(s.resident) for w in borders[:8]]
    assert g.serialize() == o.serialize() and g.validate() == 0  # a query changes nothing


# ---- b. short Tries (they come out of files) -------------------------------------------------------------------------------
def test_membership_in_tries_of_every_short_length(monkeypatch):
    """Trie buckets of every length 1 .. 100, of 728, 729, 730 (9^3: where the (QL + 1)-ary search takes a step more) and 1023, made as
    in test_insert_into_short_tries_of_a_loaded_file: ascending inserts, exported, installed with kind = Trie; the oracle loads the
    bytes. Every element and every miss that shares its bucket is queried."""
    _need_gpu()
    s = qs.shape(qs.SHORT_TRIE_SHAPE, ascending=True, kind_of=lambda n: qs.TRIE)
    g0 = cbl_amd.CBL(s.k, s.pb)
    _insert_words(g0, s.resident)
    assert set(_table(g0).values()) == {(b.length, qs.VEC) for b in s.buckets.values()}
    nb, nw, B = g0.num_buckets(), g0.count(), g0.consts()["bytes"]
    prefix = torch.empty(nb, dtype=torch.int32, device="cuda")
    count = torch.empty(nb, dtype=torch.int32, device="cuda")
    kind = torch.empty(nb, dtype=torch.uint8, device="cuda")
    suffix = torch.empty(nw * B, dtype=torch.uint8, device="cuda")
    g0.resident_export(prefix, count, kind, suffix)
    kind.fill_(1)
    g, o = cbl_amd.CBL(s.k, s.pb), Oracle(s.k, s.pb)
    g.install_buckets_device([(nb, nw, prefix, count, kind, suffix)])
    blob = g.serialize()
    o.load(blob)
    assert o.serialize() == blob and o.count() == nw == len(s.resident)
    assert g.validate(strict=False) == 0
    assert _table(g) == {b.prefix: (b.length, qs.TRIE) for b in s.buckets.values()}
    assert sorted({b.length for b in s.buckets.values()}) == sorted(qs.SHORT_TRIE_LENGTHS)
    assert o.iter_words() == sorted(s.resident)  # the oracle holds the crafted set
    every = [w for b in s.buckets.values() for w in b.candidates]
    _probe_kmers(g, o, s, every, "contains_kmers on every element and every miss of the same bucket")
    _query_every_way(g, s, monkeypatch)
    assert [o.kmer_of_word(w) for w in sorted(s.resident)] == list(g.iter())
    assert g.validate(strict=False) == 0 and g.serialize() == blob


# ---- c. long unordered Vecs: only `|=` leaves them ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(qs.MERGE_SHAPES))
def test_membership_and_iter_in_long_vecs_left_by_merges(name, monkeypatch):
    """Five indexes whose buckets are Vecs of at most 1024 words, `|=` into the first: Vecs of 4500 and of 2500 words, self's elements
    sorted and the last share's behind them (src/trievec/set_ops.rs:43-71) — not ascending, so only a scan finds every element: the
    Vec branch of the join beyond JOIN_TAB_MAX, its table below, and the long scan of k_contains."""
    _need_gpu()
    s = qs.shape(qs.MERGE_SHAPES[name])
    pairs = [_pair(s, part) for part in qs.shares(s, qs.MERGE_SHARES)]
    g, o = pairs[0]
    for g2, o2 in pairs[1:]:
        g |= g2
        o.merge(o2)
    assert g.serialize() == o.serialize() and g.count() == len(s.resident)
    assert g.validate(strict=False) == 0
    table = _table(g)
    assert table == {b.prefix: (b.length, qs.VEC) for b in s.buckets.values()}
    lengths = sorted(n for n, _ in table.values())
    assert lengths[-1] > qs.JOIN_TAB_MAX and qs.THRESHOLD < lengths[0] <= qs.JOIN_TAB_MAX
    for p, kd, stored in g.buckets():
        assert kd == qs.VEC and stored != sorted(stored) and len(stored) == s.buckets[p].length  # a search would miss elements
    _query_every_way(g, s, monkeypatch)
    _probe_kmers(g, o, s, [w for b in s.buckets.values() for w in qs.border_words(b)], "contains_kmers on the borders")
    got = list(g.iter())
    assert got == [o.kmer_of_word(w) for w in o.iter_words()] and len(got) == g.count()
    for g2, _ in pairs:
        g2.close()


# ---- d. contains_all with exactly one absent k-mer ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,pb", qs.ONE_ABSENT)
def test_contains_all_with_one_absent_kmer(k, pb, monkeypatch):
    """A sequence of three chunks whose words are all resident but one: the first k-mer, the last, the last of the first chunk, the
    first of the second chunk, none."""
    _need_gpu()
    n = qs.ONE_ABSENT_KMERS
    for absent in qs.ONE_ABSENT_AT:
        seq, words, resident = qs.all_but_one(k, pb, n, 1000 * k + pb, absent)
        g = cbl_amd.CBL(k, pb)
        _insert_words(g, resident)
        assert g.count() == len(resident)
        want = np.ones(n, dtype=bool)
        if absent is not None:
            want[absent] = False
        bases = np.frombuffer(seq, dtype=np.uint8)
        offsets = np.array([0, len(bases)], dtype=np.uint64)
        for join in (None, "1"):
            if join is None:
                monkeypatch.delenv(JOIN_ENV, raising=False)
            else:
                monkeypatch.setenv(JOIN_ENV, join)
            assert g.contains_all(seq) is (absent is None), (absent, join)
            assert np.flatnonzero(~g.contains_seq_np(seq)).tolist() == ([] if absent is None else [absent]), (absent, join)
            flags, t, p = g.contains_seqs(bases, offsets)
            assert np.array_equal(flags, want) and (t, p) == (n, int(want.sum())), (absent, join)
            assert g.contains_seqs(bases, offsets, flags=False)[1:] == (n, int(want.sum())), (absent, join)
        monkeypatch.delenv(JOIN_ENV, raising=False)
        g.close()


# ---- e. iter on Tries and wide k-mers ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["15-6", "31-3-a", "31-3-b", "45-6"])
def test_iter_over_tries_and_wide_kmers(name):
    """CBL::iter over the indexes of (a): prefixes ascending, a Vec as inserted, a Trie ascending, every word turned back into its k-mer
    (narrow, wide suffix, k-mers of more than 64 bits)."""
    _need_gpu()
    s = qs.shape(qs.EDGE_SHAPES[name])
    g, o = _pair(s, s.resident)
    want = [o.kmer_of_word(w) for w in qs.iteration_order(s)]
    got = list(g.iter())
    assert len(got) == g.count() == len(want)
    if got != want:
        i = next(i for i, (a, b) in enumerate(zip(got, want)) if a != b)
        pytest.fail(f"iter differs first at element {i}: bucket (prefix, length, kind, rank) {qs.bucket_of(s, qs.iteration_order(s)[i])}")
    assert g.contains_kmers(got[:2000]).all() and g.contains_kmers(got[-2000:]).all()
    assert want == [o.kmer_of_word(w) for w in o.iter_words()]  # and the oracle iterates the same way
