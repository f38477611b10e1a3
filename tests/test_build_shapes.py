"""What tests/build_shapes.py delivers for tests/test_gpu_build_classes.py, checked on the CPU: every named run length on both sides of every class
edge, every fill's exact distinct count, every class of k_classify and k_classify_merge in every configuration it applies to — the two restated
classifications are the check — and the closed-form model of `insert_batch` against the C++ oracle byte for byte, against PyCBL word by word on
the short shapes. Nothing here is skipped: a shape that cannot deliver an edge fails. Run with -s to see the tables of what is delivered."""
import os
import re

import pytest

import build_shapes as bs
import setops_model as sm
from oracle import Oracle, pyref
from oracle.pyref import PyCBL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_CASES = [(n, c) for n in bs.CONFIGS for c in bs.COMPOSITIONS]
MERGE_CASES = [(n, g) for n in bs.CONFIGS for g in range(len(bs.MERGE_GROUPS))]
HUGE_CONFIGS = ("packed", "wide")  # one narrow, one wide

# run length -> class of a run without a resident Trie, from the issue's list of edges (not from classify_build)
CLASS_OF_LENGTH = {2: "CLS_S16", bs.WITNESS_C: "CLS_M16", 16: "CLS_S16", 17: "CLS_S32", 32: "CLS_S32", 33: "CLS_M16", 128: "CLS_M16", 129: "CLS_M32", 256: "CLS_M32",
                   257: "CLS_M64", 512: "CLS_M64", 513: "CLS_M128", 1024: "CLS_M128", 1025: "CLS_M256", 2048: "CLS_M256", 2049: "CLS_M512",
                   4096: "CLS_M512", 4097: "CLS_BIG", 8192: "CLS_BIG", 8193: "CLS_BIG", 16384: "CLS_BIG", 16385: "CLS_BIG", 1 << 18: "CLS_BIG",
                   (1 << 18) + 1: "CLS_HUGE"}
# merge edge pair -> classes of its both-sided buckets with the union route off: (narrow suffix, wide suffix); with it on, Trie |= Trie is CLS_UNION
MERGE_CLASSES_OFF = [({"CLS_M16"},) * 2, ({"CLS_M16", "CLS_M64"},) * 2, ({"CLS_M64", "CLS_M128"},) * 2, ({"CLS_M128", "CLS_M256"},) * 2,
                     ({"CLS_M256", "CLS_M512"},) * 2, ({"CLS_M512", "CLS_BIG", "CLS_M1024"}, {"CLS_M512", "CLS_BIG", "CLS_HUGE"}),
                     ({"CLS_BIG", "CLS_M1024", "CLS_HUGE"}, {"CLS_BIG", "CLS_HUGE"})]


def _final(s):
    """the model after every batch of the shape, once per process"""
    def final_model(name, comp):
        m = bs.model_of(s)
        for words, _ in s.batches:
            bs.insert_batch(m, words)
        return m
    return bs.shape(final_model, s.name, s.comp)


def _replay(c: PyCBL, words):
    """PyCBL word by word: the loop of PyCBL.insert_seq on crafted words (groups of equal prefixes, the length check after each)"""
    sb = c.P["SB"]
    i = 0
    while i < len(words):
        p, j = words[i] >> sb, i
        while j < len(words) and words[j] >> sb == p:
            c._insert_word(words[j])
            j += 1
        b = c.buckets[p]
        if len(b[1]) > pyref.THRESHOLD and b[0] == "vec":
            b[0] = "trie"
        if b[0] == "trie":
            b[1].sort()
        i = j
    return c


def test_configs_have_the_properties_they_are_named_for():
    P = {n: bs.props(n) for n in bs.CONFIGS}
    assert [P[n]["sb"] for n in ("packed", "narrow64", "wide", "radix")] == [42, 64, 81, 117]
    assert P["packed"]["sb"] + 12 <= 64 and P["packed"]["packed"] and P["packed"]["prepass"]
    assert P["narrow64"]["sb"] == 64 and not P["narrow64"]["packed"] and not P["narrow64"]["wide"] and not P["narrow64"]["prepass"]
    assert 64 < P["wide"]["sb"] <= 116 and P["wide"]["wide"] and P["wide"]["msd"]
    assert P["radix"]["sb"] > 116 and P["radix"]["wide"] and not P["radix"]["msd"]
    for n, (k, pb) in bs.CONFIGS.items():
        assert pyref.params(k, pb)["WB"] <= 128 and pyref.params(k, pb)["SB"] == P[n]["sb"]


def test_constants_mirror_the_kernels():
    def src(name):
        with open(os.path.join(ROOT, "cbl_amd", "csrc", name)) as f:
            return f.read()

    kb, cm = src("kernels_bucket.hpp"), src("common.hpp")
    const = lambda text, name: int(re.search(r"\b%s = (\d+)\b" % name, text).group(1))
    assert const(kb, "SMALL_MAX") == bs.SMALL_MAX and const(kb, "MED_ITEMS") == bs.MED_ITEMS and const(kb, "PK_BITS") == bs.PK_BITS
    assert const(kb, "BIG_SUB") == bs.BIG_SUB and "BIG_MAX = 1u << 18" in kb and bs.BIG_MAX == 1 << 18
    assert const(cm, "VEC_THRESHOLD") == bs.THRESHOLD == pyref.THRESHOLD
    assert (const(kb, "KIND_VEC"), const(kb, "KIND_TRIE")) == (bs.VEC, bs.TRIE)
    # the edges of both classifications, as (multiple of MED_ITEMS, class) in source order: k_classify, then k_classify_merge
    edges = [(int(n), cls) for n, cls in re.findall(r"c\s*<=\s*(\d+)\s*\*\s*MED_ITEMS\b[^;]*?\bcls\s*=\s*(CLS_\w+)\s*;", kb)]
    assert edges == [(16, "CLS_M16"), (32, "CLS_M32"), (64, "CLS_M64"), (128, "CLS_M128"), (256, "CLS_M256"), (512, "CLS_M512"),
                     (16, "CLS_M16"), (64, "CLS_M64"), (128, "CLS_M128"), (256, "CLS_M256"), (512, "CLS_M512"), (1024, "CLS_M1024")], edges
    assert [bs.big_bits(c) for c in (4097, 8192, 8193, 16384, 16385, 1 << 18)] == [3, 3, 4, 4, 5, 8]


def _check_run(r, sb):
    assert r.rlen + r.arriving == r.c == len(r.resident) + len(r.stream) and len(set(r.resident)) == r.rlen
    assert all(0 <= v < 1 << sb for v in r.resident + r.stream)
    kind = bs.TRIE if r.rkind == "trie" else bs.VEC
    assert r.cls == bs.classify_build(r.rlen, kind, r.c)
    if r.rkind == "trie" and r.c <= bs.SMALL_MAX:
        assert r.cls == "CLS_M16"  # the small classes refuse a resident Trie
    elif r.c > 1:
        assert r.cls == CLASS_OF_LENGTH[r.c], (r.c, r.cls)
    else:
        assert r.cls == "single"
    if r.rkind == "trie" or r.rlen < 2:
        assert r.resident == sorted(r.resident)
    elif r.rlen > 3:  # (two or three shuffled words may come out ascending)
        assert r.resident != sorted(r.resident)
    if r.rkind != "trie":
        assert (r.rlen > bs.THRESHOLD) == (r.rkind == "lvec")
    every = set(r.resident) | set(r.stream)
    new = set(r.stream) - set(r.resident)
    assert len(every) == r.distinct
    if r.fill in bs.FILLS:
        assert r.distinct == bs.final_distinct(r.rlen, r.arriving, r.fill)
    if r.fill == "distinct":
        assert len(new) == r.arriving
    elif r.fill == "present":
        assert not new
    elif r.fill == "one_value":
        assert len(set(r.stream)) == 1 and len(new) == 1
    elif r.fill == "three_values":
        n = min(3, r.arriving)
        assert len(new) == len(set(r.stream)) == n and all(v == r.stream[j % n] for j, v in enumerate(r.stream))  # the values cycle
    elif r.fill == "twice":
        h = r.arriving // 2
        assert r.stream[:h] == r.stream[r.arriving - h:] and len(new) == (r.arriving + 1) // 2  # the second copies behind all the firsts
    elif r.fill in ("to_1024", "to_1025"):
        assert r.distinct == int(r.fill[3:])
    if r.pattern == "shared_top":
        assert len({v >> (sb - 16) for v in every}) == 1
    if r.pattern == "sentinels" and r.c >= 2 and r.fill not in ("one_value",) and (r.rlen >= 2 or len(new) >= 2):
        assert {0, (1 << sb) - 1} <= every


@pytest.mark.parametrize("name,comp", BUILD_CASES)
def test_build_shapes_deliver_every_edge_fill_and_class(name, comp):
    s = bs.shape(bs.craft_build, name, comp)
    witness = comp in ("beside_distinct", "beside_repeats")
    edge = [r for r in s.runs if not (witness and r.c == bs.WITNESS_C and r.rkind == "none" and r.fill in ("distinct", "one_value") and r.pattern == "random"
                                      and r.prefix in {s.runs[m[1]].prefix for _, m in s.batches if len(m) > 1})]
    want = list(bs.BUILD_LENGTHS)
    assert sorted({r.c for r in edge}) == want
    assert len({r.prefix for r in s.runs}) == len(s.runs)  # distinct prefixes
    for r in s.runs:
        _check_run(r, s.sb)
    by_c = {}
    for r in edge:
        by_c.setdefault(r.c, []).append(r)
    for c in want:  # every length: without a resident bucket, on a Vec, on a Trie; both sides of an edge alike
        kinds = {r.rkind for r in by_c[c]}
        assert kinds >= ({"none", "vec", "trie"} if c > 1 else {"none"}), (c, kinds)
        twin = c + 1 if c % 2 == 0 and c > 2 else c - 1 if c > 2 else None
        if twin in by_c:
            mine, its = ({(r.rkind, r.fill, r.pattern) for r in by_c[x]} for x in (c, twin))
            assert mine <= its or its <= mine  # (to_1024 / to_1025 need 1025 words, a long Vec more)
    classes = {r.cls for r in edge}
    assert classes >= set(bs.BUILD_CLASSES[:-1])  # (CLS_HUGE: the 2^18 shapes)
    assert any(r.rkind == "trie" and r.rlen <= 32 and r.c in (16, 17, 32) for r in edge) and "single" in classes
    if comp == "alone":
        assert {r.fill for r in edge} == set(bs.FILLS) and {r.pattern for r in edge} == set(bs.PATTERNS)
        assert {r.rkind for r in edge} == set(bs.RKINDS)
        long_ = [r for r in edge if r.c >= 2048]
        assert {(r.fill, r.c) for r in long_ if r.fill[:3] == "to_"} >= {(f, c) for f in ("to_1024", "to_1025") for c in (2048, 2049, 4096, 4097, 8192, 8193)}
        assert any(r.rkind == "lvec" and r.fill == "present" for r in long_) and any(r.rkind == "lvec" and r.fill == "distinct" for r in long_)
        assert {bs.big_bits(r.c) for r in edge if r.cls == "CLS_BIG"} == {3, 4, 5}
    sb = s.sb
    for words, mates in s.batches:
        pre = [w >> sb for w in words]
        groups = sum(1 for i, p in enumerate(pre) if i == 0 or pre[i - 1] != p)
        assert set(pre) == {s.runs[j].prefix for j in mates} and len(words) == sum(s.runs[j].arriving for j in mates)
        if comp == "interleaved":
            assert len(s.batches) == 1 and groups > 20 * len(mates)  # a prefix is visited in several groups
            for j in mates[:10]:
                r = s.runs[j]
                assert [w & ((1 << sb) - 1) for w in words if w >> sb == r.prefix] == r.stream  # each run's own order kept
        else:
            assert groups == len(mates) == (2 if witness else 1)
            if witness:
                w = s.runs[mates[1]]
                assert w.cls == "CLS_M16" and w.c == bs.WITNESS_C and len(set(w.stream)) == (1 if comp == "beside_repeats" else bs.WITNESS_C)
    assert sum(len(w) for w, _ in s.batches) <= 350_000
    m = _final(s)
    for r in s.runs:
        kind, items = m.buckets[r.prefix]
        assert len(items) == r.distinct and (kind == "trie") == (r.rkind == "trie" or r.distinct > 1024 or r.rkind == "lvec"), bs.describe(r)
    print("\nbuild %-8s %-15s SB=%3d: %d runs, %d words; lengths %s" % (name, comp, s.sb, len(edge), sum(len(w) for w, _ in s.batches), want))
    for c in want:
        print("  c=%-6d %s" % (c, "; ".join("%s%s %s/%s -> %s" % (r.rkind, r.rlen or "", r.fill, r.pattern, r.cls) for r in by_c[c])))


@pytest.mark.parametrize("name,comp", BUILD_CASES)
def test_model_equals_the_oracle_on_every_build_shape(name, comp):
    s = bs.shape(bs.craft_build, name, comp)
    blob = bs.serialize(bs.model_of(s))
    o = Oracle(s.k, s.pb)
    o.load(blob)
    assert o.serialize() == blob
    m = _final(s)
    for words, _ in s.batches:
        o.insert_words(words)
    want = bs.serialize(m)
    assert o.serialize() == want and o.count() == m.count()
    for words, _ in s.batches[:: max(1, len(s.batches) // 20)]:  # the same words once more: nothing changes
        o.insert_words(words)
        bs.insert_batch(m, words)
    assert o.serialize() == want == bs.serialize(m)


@pytest.mark.parametrize("name", list(bs.CONFIGS))
def test_model_equals_pycbl_word_by_word_on_the_short_shapes(name):
    """Every run of up to 1025 words, and of the longer ones up to 5000 words those a fill or a long Vec makes special, each as its own batch;
    then the interleaved batch cut down to the prefixes of its runs of up to 1025 words (several groups per prefix)."""
    s = bs.shape(bs.craft_build, name, "alone")
    n = 0
    for r in s.runs:
        if r.c > 5000 or (r.c > 1025 and not (r.fill[:3] == "to_" or r.rkind == "lvec")):
            continue
        res = {r.prefix: ("trie" if r.rkind == "trie" else "vec", r.resident)} if r.rlen else {}
        words = [(r.prefix << s.sb) | v for v in r.stream]
        a, b = bs.model_of(res, s.k, s.pb), bs.model_of(res, s.k, s.pb)
        assert bs.insert_batch(a, words).buckets == _replay(b, words).buckets, bs.describe(r)
        assert bs.serialize(a) == b.serialize()
        n += 1
    assert n >= 80
    s = bs.shape(bs.craft_build, name, "interleaved")
    keep = {r.prefix for r in s.runs if r.c <= 1025}
    words = [w for w in s.batches[0][0] if w >> s.sb in keep]
    res = {p: v for p, v in s.resident.items() if p in keep}
    a, b = bs.model_of(res, s.k, s.pb), bs.model_of(res, s.k, s.pb)
    assert bs.insert_batch(a, words).buckets == _replay(b, words).buckets
    assert {k for k, _ in a.buckets.values()} == {"vec", "trie"} and max(len(v) for _, v in a.buckets.values()) == 1025


@pytest.mark.parametrize("name", list(bs.CONFIGS))
def test_quick_serializer_equals_pycbl(name):
    s = bs.craft_build(name, "alone", lengths=(2, 33, 1025, 2049))
    m = bs.model_of(s)
    assert bs.serialize(m) == m.serialize()
    for words, _ in s.batches:
        bs.insert_batch(m, words)
    assert bs.serialize(m) == m.serialize()
    assert {k for k, _ in m.buckets.values()} == {"vec", "trie"}


@pytest.mark.parametrize("name", HUGE_CONFIGS)
def test_huge_shapes_deliver_both_sides_of_big_max(name):
    """2^18 (CLS_BIG) and 2^18 + 1 (CLS_HUGE), each as a run of repeats that stays a Vec of 1024 words and as a mostly distinct one. The mostly
    distinct runs arrive on a resident Trie: the oracle scans a Vec linearly, and 2^18 distinct words into one took it far more than 10 s."""
    s = bs.shape(bs.craft_huge, name)
    for r in s.runs:
        _check_run(r, s.sb)
    assert [(r.c, r.fill, r.cls) for r in s.runs] == [(1 << 18, "to_1024", "CLS_BIG"), (1 << 18, "mostly_distinct", "CLS_BIG"),
                                                      ((1 << 18) + 1, "to_1024", "CLS_HUGE"), ((1 << 18) + 1, "mostly_distinct", "CLS_HUGE")]
    assert all(r.distinct == 1024 or r.distinct > 250_000 for r in s.runs)
    m = bs.model_of(s)
    o = Oracle(s.k, s.pb)
    o.load(bs.serialize(m))
    for words, _ in s.batches:
        bs.insert_batch(m, words)
        o.insert_words(words)
    assert o.serialize() == bs.serialize(m)
    assert sorted(bs.table(m).values()) == sorted((r.distinct, bs.VEC if r.distinct == 1024 else bs.TRIE) for r in s.runs)
    print("\nbuild %-8s huge: %s" % (name, [(r.c, r.rkind, r.rlen, r.fill, r.cls) for r in s.runs]))


def _merged(s):
    def merged_models(name, group):
        a, b = bs.model_of(s.a, s.k, s.pb), bs.model_of(s.b, s.k, s.pb)
        a.merge(b)
        return a, b
    return bs.shape(merged_models, s.name, s.group)


def _check_pairs(s):
    for pr in s.pairs:
        assert (len(pr.self_items), len(pr.other_items)) == (pr.cs, pr.co) and len(set(pr.self_items)) == pr.cs and len(set(pr.other_items)) == pr.co
        for mk, items in ((pr.ks, pr.self_items), (pr.ko, pr.other_items)):
            lo, hi = bs._MRANGE[mk]
            assert lo <= len(items) <= hi
            if mk in ("svec", "trie", "strie") or len(items) < 2:
                assert items == sorted(items)
            elif len(items) > 3:  # (two or three shuffled words may come out ascending)
                assert items != sorted(items)
        S, O = set(pr.self_items), set(pr.other_items)
        if pr.overlap == "disjoint":
            assert not S & O and (min(pr.cs, pr.co) < 2 or (min(O) < max(S) and min(S) < max(O)))
        elif pr.overlap == "contained":
            assert O <= S or S <= O
        elif pr.overlap == "interleaved":
            assert S & O and (O - S or pr.co == 1) and (S - O or pr.cs == 1)
        elif pr.overlap == "below":
            assert max(O) < min(S)
        else:
            assert min(O) > max(S)


@pytest.mark.parametrize("name,gi", MERGE_CASES)
def test_merge_shapes_deliver_every_edge_kind_and_class(name, gi):
    s = bs.shape(bs.craft_merge, name, gi)
    wide = bs.props(name)["wide"]
    _check_pairs(s)
    assert sorted({pr.cs + pr.co for pr in s.pairs}) == list(bs.MERGE_GROUPS[gi])
    for c in bs.MERGE_GROUPS[gi]:
        got = {(pr.ks, pr.ko) for pr in s.pairs if pr.cs + pr.co == c}
        feasible = {(a, b) for a in bs.MKINDS for b in bs.MKINDS if bs.split(c, a, b) is not None}
        assert got == feasible if c <= 1025 else got >= {p for p in (("trie", "trie"), ("vec", "vec"), ("lvec", "trie"), ("trie", "lvec")) if p in feasible}
    on, off = bs.merge_classes(s, True), bs.merge_classes(s, False)
    tt = [bs.is_trie(pr.ks) and bs.is_trie(pr.ko) for pr in s.pairs]
    assert all((a == "CLS_UNION") == bool(t) and (t or a == b) for a, b, t in zip(on, off, tt)) and any(tt)
    assert set(off) == MERGE_CLASSES_OFF[gi][wide], (set(off), gi)
    # buckets only one side holds, of every kind, beside them
    both = {pr.prefix for pr in s.pairs}
    for side in (s.a, s.b):
        alone = [v for p, v in side.items() if p not in both]
        assert sorted((k, len(v) > 1024, len(v) <= 32) for k, v in alone) == [("trie", False, True), ("trie", True, False), ("vec", False, False), ("vec", False, False), ("vec", True, False)]
    assert not (set(s.a) - both) & (set(s.b) - both)
    print("\nmerge %-8s c=%s: %d pairs; union on %s; off %s" % (name, bs.MERGE_GROUPS[gi], len(s.pairs), sorted(set(on)), sorted(set(off))))
    print("  " + "; ".join("%d=%s%d|%s%d %s" % (pr.cs + pr.co, pr.ks, pr.cs, pr.ko, pr.co, pr.overlap) for pr in s.pairs))


def test_merge_shapes_cover_every_kind_pair_overlap_and_class():
    for name in bs.CONFIGS:
        shapes = [bs.shape(bs.craft_merge, name, gi) for gi in range(len(bs.MERGE_GROUPS))]
        pairs = [pr for s in shapes for pr in s.pairs]
        # beyond 1025 words: every pair of kinds that can hold 8193 words between them (one side a long Vec or a Trie)
        assert {(pr.ks, pr.ko) for pr in pairs if pr.cs + pr.co >= 2048} >= {(a, b) for a in bs.MKINDS for b in bs.MKINDS if bs.split(8193, a, b) is not None}
        assert {(pr.ks, pr.overlap) for pr in pairs} == {(a, o) for a in bs.MKINDS for o in bs.OVERLAPS}
        assert {(pr.ko, pr.overlap) for pr in pairs} == {(a, o) for a in bs.MKINDS for o in bs.OVERLAPS}
        classes = {c for s in shapes for u in (True, False) for c in bs.merge_classes(s, u)}
        assert classes == set(bs.MERGE_CLASSES) - ({"CLS_M1024"} if bs.props(name)["wide"] else set())
    assert sorted(c for g in bs.MERGE_GROUPS for c in g) == list(bs.MERGE_LENGTHS)


@pytest.mark.parametrize("name,gi", MERGE_CASES)
def test_pycbl_merge_equals_the_oracle_on_every_merge_shape(name, gi):
    s = bs.shape(bs.craft_merge, name, gi)
    _merge_against_oracle(s)


def _merge_against_oracle(s):
    a0, b0 = bs.serialize(bs.model_of(s.a, s.k, s.pb)), bs.serialize(bs.model_of(s.b, s.k, s.pb))
    oa, ob = Oracle(s.k, s.pb), Oracle(s.k, s.pb)
    oa.load(a0)
    ob.load(b0)
    assert oa.serialize() == a0 and ob.serialize() == b0
    oa.merge(ob)
    a, b = _merged(s)
    assert oa.serialize() == bs.serialize(a) and ob.serialize() == bs.serialize(b)
    assert sm.words(a) == sm.words(bs.model_of(s.a, s.k, s.pb)) | sm.words(b) and oa.count() == a.count()
    for pr in s.pairs:  # other's Vecs on shared prefixes end up sorted; a Vec self stays a Vec whatever its length
        assert b.buckets[pr.prefix][1] == sorted(pr.other_items)
        assert a.buckets[pr.prefix][0] == ("trie" if bs.is_trie(pr.ks) else "vec")
    assert b0 != bs.serialize(b) or not any(pr.ko == "vec" and pr.co > 3 for pr in s.pairs)


@pytest.mark.parametrize("name", ["packed"])
def test_huge_merge_pair_delivers_both_sides_of_big_max(name):
    s = bs.shape(bs.craft_merge_huge, name)
    _check_pairs(s)
    assert [pr.cs + pr.co for pr in s.pairs] == [1 << 18, (1 << 18) + 1]
    assert bs.merge_classes(s, True) == ["CLS_UNION", "CLS_UNION"] and bs.merge_classes(s, False) == ["CLS_BIG", "CLS_HUGE"]
    _merge_against_oracle(s)
    print("\nmerge %-8s huge: Trie |= Trie of %s words: CLS_UNION; CLS_BIG / CLS_HUGE with the union route off" % (name, [pr.cs + pr.co for pr in s.pairs]))


def test_predicted_stage_units_add_up():
    """merge_units (what tests/test_gpu_build_classes.py expects of cblx_stage_units): every both-sided word is in exactly one bucket stage, and
    the gather moves everything but the buckets read in place and the unions."""
    for name in bs.CONFIGS:
        s = bs.shape(bs.craft_merge, name, 5)
        a, _ = _merged(s)
        both = sum(pr.cs + pr.co for pr in s.pairs)
        total = sum(len(v) for _, v in s.a.values()) + sum(len(v) for _, v in s.b.values())
        u_off = bs.merge_units(s, False, False, a)
        assert u_off["bucket_medium"] + u_off["bucket_huge"] + u_off["bucket_big"] == both and u_off["merge_gather"] == total
        u_on = bs.merge_units(s, True, True, a)
        assert u_on["bucket_big"] == sum(len(a.buckets[pr.prefix][1]) for pr in s.pairs if bs.is_trie(pr.ks) and bs.is_trie(pr.ko))
        assert (u_on["merge_gather"] < bs.merge_units(s, True, False, a)["merge_gather"]) == bs.props(name)["msd"]
