"""The bucket stage of the build and of `|=` at every run-length class edge: k_classify / k_classify_merge and the kernels behind their classes
against crafted buckets whose run length — resident plus arriving words, duplicates included — sits on either side of every edge. The batches
come from tests/build_shapes.py; tests/test_build_shapes.py shows on the CPU that every named length, fill and class is there and that the
model equals the oracle. Every expectation is that closed-form model (or PyCBL.merge), never the GPU path; byte identity has no tolerance.

Route evidence. A context created with profile=True counts, per stage, the timers that ran (stage_times) and, for `|=`, the words the stage's
kernels were given (stage_units). For the build that tells: bucket_small ran exactly when a small class is populated; bucket_big and bucket_huge
did not run without a long run, and which of them a long run took where the code leaves no choice (see _routes). It cannot tell bucket_medium
(its timer brackets the stage in every batch, whatever is populated), nor which kernel inside a stage ran: counting sort, walk kernel, claim
table or the radix retry, and whether the pre-pass of the long runs finished a run or passed it on. For `|=` every stage's words are predicted
exactly from the restated classification, the gather's included, which shows the in-place route against the gathered one."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402

import build_shapes as bs  # noqa: E402  (tests/)

M64 = (1 << 64) - 1
BUILD_CASES = [(n, c) for n in bs.CONFIGS for c in bs.COMPOSITIONS]
MERGE_CASES = [(n, g) for n in bs.CONFIGS for g in range(len(bs.MERGE_GROUPS))]
ROUTES = ((None, None), ("CBLX_MERGE_UNION", "0"), ("CBLX_MERGE_DIRECT", "0"))


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


def _table(g):
    p, l, kd = g.bucket_table_np()
    return {int(a): (int(b), int(c)) for a, b, c in zip(p, l, kd)}


def _loaded(k, pb, blob, what):
    g = cbl_amd.CBL(k, pb, profile=True)
    g.load(blob)
    assert g.serialize() == blob, f"{what}: the crafted bytes do not round-trip"
    return g


def _same(g, m, what, about=lambda p: None):
    """g holds the model's bytes, count, bucket table and is sound — or a message that names the buckets that differ"""
    want = bs.serialize(m)
    if g.serialize() != want:
        got = {p: ("trie" if kd else "vec", list(items)) for p, kd, items in g.buckets()}
        want_b = {p: (kind, list(items)) for p, (kind, items) in m.buckets.items()}
        bad = [p for p in sorted(set(got) | set(want_b)) if got.get(p) != want_b.get(p)]
        where = [(p, about(p), "got %s" % (got.get(p, ("absent", []))[0],), len(got.get(p, ("", []))[1]), "want %s" % (m.buckets.get(p, ["absent", []])[0],),
                  len(m.buckets.get(p, ["", []])[1])) for p in bad[:6]]
        pytest.fail(f"{what}: bytes differ in {len(bad)} buckets; (prefix, bucket, got kind, length, wanted kind, length): {where}")
    assert g.count() == m.count(), what
    assert _table(g) == bs.table(m), what
    assert g.validate(strict=False) == 0, what


def _routes(P, classes, st, what):
    """stage_times launches against the classes the restated k_classify populates in this batch (see the module's docstring for what they cannot tell)"""
    ran = {k: st.get(k, (0.0, 0))[1] > 0 for k in ("bucket_small", "bucket_medium", "bucket_big", "bucket_huge")}
    small = any(c in ("CLS_S16", "CLS_S32") for c in classes)
    big, huge = "CLS_BIG" in classes, "CLS_HUGE" in classes
    assert ran["bucket_small"] == small, (what, classes, ran)
    assert ran["bucket_medium"], (what, ran)  # (the timer brackets the stage in every batch: no evidence of a populated class)
    if not (big or huge):
        assert not ran["bucket_big"] and not ran["bucket_huge"], (what, classes, ran)
    if big and P["msd"]:
        assert ran["bucket_big"], (what, classes, ran)  # the pre-pass or the split path; the split path may still pass a run on to bucket_huge
    if big and not P["msd"]:
        assert ran["bucket_huge"] and not ran["bucket_big"], (what, classes, ran)  # suffixes the split path does not take: the general kernel
    if huge and not P["prepass"]:
        assert ran["bucket_huge"], (what, classes, ran)  # (with the pre-pass a run of repeats may be finished before the general kernel)


def _build_case(s):
    _need_gpu()
    P = bs.props(s.name)
    m = bs.model_of(s)
    g = _loaded(s.k, s.pb, bs.serialize(m), f"{s.name}/{s.comp}")
    assert g.consts()["suffix_bits"] == s.sb
    by_prefix = {r.prefix: r for r in s.runs}
    first = None
    for again in (False, True):  # the same batches once more: run lengths of present words only, nothing changes
        for bi, (words, mates) in enumerate(s.batches):
            classes = []
            for j in mates:
                r = s.runs[j]
                kind, items = m.buckets.get(r.prefix, ["vec", []])
                classes.append(bs.classify_build(len(items), bs.TRIE if kind == "trie" else bs.VEC, len(items) + r.arriving))
            assert again or classes == [s.runs[j].cls for j in mates]
            what = f"{s.name}/{s.comp} batch {bi}{' again' if again else ''}: {[bs.describe(s.runs[j]) for j in mates[:4]]}"
            bs.insert_batch(m, words)
            g.stage_times_reset()
            _insert_words(g, words)
            _routes(P, classes, g.stage_times(), what)
            assert g.count() == m.count(), what
            assert _table(g) == bs.table(m), what
        _same(g, m, f"{s.name}/{s.comp}{' again' if again else ''}", lambda p: bs.describe(by_prefix[p]) if p in by_prefix else None)
        if again:
            assert g.serialize() == first, f"{s.name}/{s.comp}: the same batches once more changed the index"
        first = g.serialize()
    g.close()


# ---- a. the build: every edge alone in its batch, beside a witness class, and all of them interleaved in one batch ----------------------------
@pytest.mark.parametrize("name,comp", BUILD_CASES)
def test_build_at_every_run_length_class_edge(name, comp):
    """Runs of exactly 1, 2, 16 | 17, 32 | 33, 128 | 129, 256 | 257, 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097, 8192 | 8193, 16384 | 16385 words
    on no resident bucket, a Vec, a Trie (of up to 32 words under the small classes), a long Vec; arriving words all new, all present, one
    value, three values, every value twice, or sized to 1024 / 1025 distinct words in the end; random suffixes, suffixes that share their top 16
    bits, suffixes 0 and 2^SB - 1. `alone`: one run per batch; `beside_distinct` / `beside_repeats`: with a CLS_M16 run of distinct words / of one
    value (repeat_mode) in the same batch; `interleaved`: every run in one batch, the stream changing prefix every few words."""
    _build_case(bs.shape(bs.craft_build, name, comp))


@pytest.mark.parametrize("name", ["packed", "wide"])
def test_build_on_both_sides_of_big_max(name):
    """2^18 words (CLS_BIG) and 2^18 + 1 (CLS_HUGE), each alone in its batch: repeats that leave a Vec of 1024 words, and mostly distinct words on
    top of a resident Trie."""
    _build_case(bs.shape(bs.craft_huge, name))


# ---- b. `|=` ---------------------------------------------------------------------------------------------------------------------------------
def _merge_case(s, monkeypatch):
    _need_gpu()
    a0, b0 = bs.serialize(bs.model_of(s.a, s.k, s.pb)), bs.serialize(bs.model_of(s.b, s.k, s.pb))
    ma, mb = bs.model_of(s.a, s.k, s.pb), bs.model_of(s.b, s.k, s.pb)
    ma.merge(mb)
    by_prefix = {pr.prefix: pr for pr in s.pairs}

    def about(p):
        pr = by_prefix.get(p)
        return pr and dict(self=(pr.ks, pr.cs), other=(pr.ko, pr.co), c=pr.cs + pr.co, overlap=pr.overlap)

    for env, val in ROUTES:
        for e, _ in ROUTES[1:]:
            monkeypatch.delenv(e, raising=False)
        if env:
            monkeypatch.setenv(env, val)
        what = f"{s.name}/merge {s.group}, {env or 'default'}"
        ga, gb = _loaded(s.k, s.pb, a0, what), _loaded(s.k, s.pb, b0, what)
        ga.stage_times_reset()
        ga |= gb
        units = ga.stage_units()
        union_path, direct = env != "CBLX_MERGE_UNION", env != "CBLX_MERGE_DIRECT"
        classes = bs.merge_classes(s, union_path)
        _same(ga, ma, what + ": self " + str(sorted(set(classes))), about)
        _same(gb, mb, what + ": other", about)  # its Vecs on shared prefixes are sorted now
        want = bs.merge_units(s, union_path, direct, ma)
        assert {k: units[k] for k in want} == want, (what, sorted(set(classes)))
        ga.close()
        gb.close()
    for e, _ in ROUTES[1:]:
        monkeypatch.delenv(e, raising=False)


@pytest.mark.parametrize("name,gi", MERGE_CASES)
def test_merge_at_every_run_length_class_edge(name, gi, monkeypatch):
    """`a |= b` with cs + co of exactly 2, 128 | 129, 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097, 8192 | 8193 words per shared prefix; either side a
    shuffled Vec, an ascending Vec, a long Vec, a Trie or a Trie of up to 32 words; other disjoint, contained, interleaved, wholly below or wholly
    above self; buckets of every kind that only one side holds beside them. By the default route, with CBLX_MERGE_UNION=0 (Trie |= Trie through the
    length classes, CLS_BIG beyond 4096 words) and with CBLX_MERGE_DIRECT=0 (every run gathered)."""
    _merge_case(bs.shape(bs.craft_merge, name, gi), monkeypatch)


def test_merge_of_tries_on_both_sides_of_big_max(monkeypatch):
    """One Trie |= Trie pair of 2^18 words and one of 2^18 + 1: CLS_UNION; CLS_BIG and CLS_HUGE with the union route off."""
    _merge_case(bs.shape(bs.craft_merge_huge, "packed"), monkeypatch)


# ---- c. a long Vec made by `|=` on the device, touched by a later batch --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(bs.CONFIGS))
def test_long_vec_left_by_merge_turns_into_a_trie_when_touched(name):
    """Vec |= Vec leaves Vecs of 1500 words. A batch of present words only and a batch with new words each turn theirs into an ascending Trie
    (src/wordset/mod.rs:213-214 checks every touched container); the third, untouched, stays a Vec as stored."""
    _need_gpu()
    import random

    k, pb = bs.CONFIGS[name]
    sb = bs.props(name)["sb"]
    rng = random.Random("long vec " + name)
    prefixes = rng.sample(range(1 << pb), 3)
    a, b = {}, {}
    for p in prefixes:
        v = bs.Values(rng, sb, "random").take(1500)
        a[p], b[p] = bs._store(rng, "vec", v[:700]), bs._store(rng, "vec", v[600:1500])  # 100 shared
    ma, mb = bs.model_of(a, k, pb), bs.model_of(b, k, pb)
    ga, gb = _loaded(k, pb, bs.serialize(ma), name), _loaded(k, pb, bs.serialize(mb), name)
    ga |= gb
    ma.merge(mb)
    _same(ga, ma, f"{name}: after |=")
    assert set(bs.table(ma).values()) == {(1500, bs.VEC)}
    present = [(prefixes[0] << sb) | v for v in rng.sample(ma.buckets[prefixes[0]][1], 40)]
    fresh = [(prefixes[1] << sb) | v for v in bs.Values(rng, sb, "random").take(40) + ma.buckets[prefixes[1]][1][:5]]
    for words, p in ((present, prefixes[0]), (fresh, prefixes[1])):
        bs.insert_batch(ma, words)
        _insert_words(ga, words)
        _same(ga, ma, f"{name}: prefix {p} touched by {len(words)} words")
    assert bs.table(ma) == {prefixes[0]: (1500, bs.TRIE), prefixes[1]: (1540, bs.TRIE), prefixes[2]: (1500, bs.VEC)}
    ga.close()
    gb.close()
