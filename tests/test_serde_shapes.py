"""What tests/serde_shapes.py delivers for tests/test_gpu_serde_edges.py, checked on the CPU. The restated geometry is read out of
kernels_serde.hpp and host_index.hpp; the expected bytes of every shape equal the C++ oracle's (load + serialize, count, iter_words) and, on the
small shapes, PyCBL.serialize; and every class, both sides of every edge, every fan-out, both sides of the staging threshold of every emitting
instance at all 16 misalignments, the split plans and the chunk geometry are found in the crafted tables by the restated classify / split_plan /
layout, not by the crafter's labels alone. There is no route counter in the serializer: which path a bucket takes on the GPU rests on this file.
Nothing here is skipped: a shape that cannot deliver a piece fails."""
import os
import re
from collections import Counter

import pytest

import build_shapes as bs
import serde_shapes as ss
from oracle import Oracle, pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDS = [ss.case_id(c) for c in ss.CASES]


def _src(name):
    with open(os.path.join(ROOT, "cbl_amd", "csrc", name)) as f:
        return f.read()


def _marked(s, label):
    got = [p for p, m in s.marks.items() if m == label]
    assert len(got) == 1, (s.name, label, got)
    return s.buckets[got[0]]


def _layout_of(s, label):
    p = [p for p, m in s.marks.items() if m == label]
    assert len(p) == 1, (s.name, label)
    return [e for e in ss.layout(s) if e.prefix == p[0]][0]


def fanouts(items, by):
    """{level: Counter of child counts of the nodes of that level}, by the definition: a node is a distinct prefix of `level` bytes, its children
    the distinct prefixes one byte longer"""
    out = {}
    for d in range(by):
        kids = Counter()
        for child in {s >> (8 * (by - 1 - d)) for s in items}:
            kids[child >> 8] += 1
        out[d] = Counter(kids.values())
    return out


# ---- the restated constants --------------------------------------------------------------------------------------------------------------------
def test_constants_mirror_the_sources():
    ks, hi = _src("kernels_serde.hpp"), _src("host_index.hpp")
    line = lambda text, n: text.split("\n")[n - 1]
    assert "static const u32 SER_TINY = 32;" in line(ks, 69) and ss.SER_TINY == 32
    assert "SER_CAP64 = 64 * 16, SER_CAP256 = 256 * 16, SER_CAP1024 = 1024 * 8;" in line(ks, 68)
    assert (ss.SER_CAP64, ss.SER_CAP256, ss.SER_CAP1024) == (1024, 4096, 8192)
    assert "static const u32 SER_SPLIT_MAX = 1u << 21;" in line(ks, 67) and ss.SER_SPLIT_MAX == 1 << 21
    assert "static const u32 SER_CHUNKS = 32;" in line(ks, 62) and ss.SER_CHUNKS == 32
    assert "constexpr u32 STAGE = EMIT ? (u32)CAP * 13u + 64u : 0u;" in line(ks, 126) and (ss.STAGE_PER_ELEMENT, ss.STAGE_SLACK) == (13, 64)
    assert "CAP = THREADS * ITEMS" in ks and "const bool staged = EMIT && esz + mis <= STAGE;" in line(ks, 140)
    assert "const u32 mis = EMIT ? (u32)(reinterpret_cast<uintptr_t>(gdst) & 15u) : 0u;" in ks
    assert "return v <= 250 ? 1u : v < (1ull << 16) ? 3u : v < (1ull << 32) ? 5u : 9u;" in line(ks, 24)
    assert "const bool tiny = live && kind[r] == KIND_VEC && n <= SER_TINY;" in line(ks, 81)
    assert ("cls = n <= SER_CAP64 ? SER_C64 : n <= SER_CAP256 ? SER_C256 : n <= SER_CAP1024 ? SER_C1024 : "
            "(kind[r] == KIND_TRIE && n <= SER_SPLIT_MAX && BYTES > 1) ? SER_SPLIT : SER_HOST;") in line(ks, 105)
    assert "(u32)(r / per)" in line(ks, 106)
    assert "if (c > SER_CAP1024) atomicOr(&s_bad, 1u);" in line(ks, 329)
    assert "if (c) cls = c <= SER_CAP64 ? 0 : c <= SER_CAP256 ? 1 : 2;" in line(ks, 335)
    # the instances: sizing and emitting, of whole buckets and of sub-ranges
    inst = lambda text: [tuple(int(x) for x in m) for m in re.findall(r"integral_constant<int, (\d+)>\(\), integral_constant<int, (\d+)>\(\)", text)]
    sub, whole = hi[hi.index("auto sub_buckets"): hi.index("const u64 per =")], hi[hi.index("auto buckets = "): hi.index("if (nb) {")]
    for text in (sub, whole):
        assert inst(text)[:4] == [ss.EMITTING["c64"], ss.SIZING["c64"], ss.EMITTING["c256"], ss.SIZING["c256"]]
        assert inst(text)[4:] == [(1024, 8)] or (len(inst(text)) == 4 and text.count("k_serde_bucket<1024, 8, WS, EM") == 1)
    assert ss.SIZING["c1024"] == ss.EMITTING["c1024"] == (1024, 8)
    for cls, cap in zip(ss.WG_CLASSES, (ss.SER_CAP64, ss.SER_CAP256, ss.SER_CAP1024)):
        assert ss.SIZING[cls][0] * ss.SIZING[cls][1] == ss.EMITTING[cls][0] * ss.EMITTING[cls][1] == cap
    assert ss.SIZING["c64"][0] // 64 == 1 and all(th // 64 > 1 for th, _ in list(ss.EMITTING.values()) + [ss.SIZING["c256"], ss.SIZING["c1024"]])  # the one NW == 1 instance
    assert "const u64 per = std::max<u64>(1, ceil_div(nb, (u64)SER_CHUNKS));" in hi
    assert "const bool chunked = (bool)on_chunk && nb >= 4 * SER_CHUNKS && blob.n >= chunk_min;" in hi and ss.CHUNKED_MIN_BUCKETS == 128
    # where the blob starts: a pool block (hipMalloc's pointer), the body hs.pos bytes in
    assert "blob.bytes = Buf<u8>(c->pool, blob.n + 16);" in hi and "u8* body = blob.bytes.get() + hs.pos;" in hi
    ctx = _src("ctx.hpp")
    assert "sz = (sz + 255) & ~(size_t)255;" in ctx and "hipError_t e = hipMalloc(&p, sz);" in ctx and "blks.push_back({p, sz, true});" in ctx


def test_widths_are_what_they_are_named_for():
    want = {"packed": (42, 6, 2), "narrow64": (64, 8, 8), "wide": (81, 11, 1), "radix": (117, 15, 5), "b4": (29, 4, 5), "b1": (8, 1, 8), "pb24": (44, 6, 4)}
    for w, (sb, by, tb) in want.items():
        k, pb, gsb, gby = ss.geom(w)
        assert (gsb, gby, ss.top_bits(gsb, gby)) == (sb, by, tb) and pyref.params(k, pb)["BYTES"] == by, w
    assert ss.geom("pb24")[1] > 16 and all(ss.geom(w)[1] <= 16 for w in ss.ALL_WIDTHS)
    assert [ss.vlen(v) for v in (0, 250, 251, 65535, 65536, (1 << 32) - 1, 1 << 32)] == [1, 1, 3, 3, 5, 5, 9]
    assert [len(pyref.PyCBL._varint(v)) for v in (0, 250, 251, 65535, 65536)] == [1, 1, 3, 3, 5]
    for kind, n, by, cls in (("vec", 32, 6, "tiny"), ("vec", 33, 6, "c64"), ("trie", 1, 6, "c64"), ("trie", 32, 6, "c64"), ("vec", 1024, 6, "c64"), ("vec", 1025, 6, "c256"),
                             ("trie", 4096, 6, "c256"), ("trie", 4097, 6, "c1024"), ("vec", 8192, 6, "c1024"), ("vec", 8193, 6, "host"), ("trie", 8193, 6, "split"),
                             ("trie", 1 << 21, 6, "split"), ("trie", (1 << 21) + 1, 6, "host"), ("trie", 8193, 1, "host")):
        assert ss.classify(kind, n, by) == cls, (kind, n, by)


# ---- the model's bytes against the oracle --------------------------------------------------------------------------------------------------------
def _against_oracle(s, pycbl=False):
    want = ss.expected(s)
    m = ss.model(s)
    if len(want) < 1 << 24:
        assert want == bs.serialize(m), s.name
    o = Oracle(s.k, s.pb)
    o.load(want)
    assert o.serialize() == want, s.name
    words = sorted((p << s.sb) | x for p, (_, items) in s.buckets.items() for x in items)
    assert o.count() == len(words) == len(set(words)) == m.count(), s.name
    assert o.n_buckets() == len(s.buckets)
    if len(words) <= 400000:
        assert sorted(o.iter_words()) == words, s.name
    if pycbl:
        assert m.serialize() == want, s.name
    for p, (kind, items) in s.buckets.items():
        assert kind in ("vec", "trie") and all(0 <= x < 1 << s.sb for x in (items[0], items[-1], max(items)))
        assert kind == "vec" or all(a < b for a, b in zip(items, items[1:])), (s.name, p)
    lay = ss.layout(s)
    assert sum(e.size for e in lay) + len(ss.header(len(s.buckets))) == len(want)
    pr, ct, kd, sf = ss.arrays(s)
    assert pr.dtype.name == "uint32" and ct.dtype.name == "uint32" and kd.dtype.name == "uint8" and sf.dtype.name == "uint8"
    assert len(sf) == s.by * len(words) and pr.tolist() == sorted(s.buckets) and ct.tolist() == [e.n for e in lay]
    if lay:  # the first and the last stored suffix, byte for byte
        first, last = s.buckets[lay[0].prefix][1][0], s.buckets[lay[-1].prefix][1][-1]
        assert bytes(sf[: s.by]) == first.to_bytes(s.by, "little") and bytes(sf[-s.by:]) == last.to_bytes(s.by, "little")


@pytest.mark.parametrize("case", ss.CASES, ids=IDS)
def test_model_bytes_equal_the_oracle(case):
    s = ss.shape(*case)
    _against_oracle(s, pycbl=sum(len(v[1]) for v in s.buckets.values()) <= 20000)


def test_model_bytes_equal_the_oracle_on_both_sides_of_split_max():
    """Tries of 2^21 and 2^21 + 1 words, packed: the expected bytes are the model's, the oracle reloads them and writes them back."""
    s = ss.shape(ss.craft_split_max)
    _against_oracle(s)
    a, b = _marked(s, "length %d" % ss.SER_SPLIT_MAX), _marked(s, "length %d" % (ss.SER_SPLIT_MAX + 1))
    assert ss.classify(a[0], len(a[1]), s.by) == "split" and ss.classify(b[0], len(b[1]), s.by) == "host"
    counts, classes, bad = ss.split_plan(a[1], s.by)
    assert bad and sum(counts) == 1 << 21 and [c > ss.SER_CAP1024 for c in counts[:4]] == [True] * 4 and not any(counts[4:])  # 4 sub-ranges: the plan hands it to the host


# ---- coverage ----------------------------------------------------------------------------------------------------------------------------------
def test_length_edges_are_there_in_every_width():
    for w in ss.ALL_WIDTHS:
        k, pb, sb, by = ss.geom(w)
        for kind in ("vec", "trie"):
            s = ss.shape(ss.craft_lengths, w, kind)
            got = {}
            lay = ss.layout(s)
            for i, e in enumerate(lay):
                if e.prefix in s.marks:
                    assert s.marks[e.prefix] == "length %d" % e.n and e.kind == kind
                    got[e.n] = e.cls
                    assert 0 < i < len(lay) - 1 and lay[i - 1].prefix not in s.marks and lay[i + 1].prefix not in s.marks  # between ordinary neighbours
            assert sorted(got) == [n for n in ss.LENGTHS if n <= 1 << sb], (w, kind)
            if sb > 13:
                assert sorted(got) == list(ss.LENGTHS)
            for n, cls in got.items():
                want = ("tiny" if n <= 32 and kind == "vec" else "c64" if n <= 1024 else "c256" if n <= 4096 else "c1024" if n <= 8192 else "host" if kind == "vec" else "split")
                assert cls == want, (w, kind, n, cls)
            if kind == "vec":  # a Vec of more than 1024 words is stored as `|=` leaves it, a shorter one unsorted
                for p, m in s.marks.items():
                    items = s.buckets[p][1]
                    assert len(items) < 8 or items != sorted(items), (w, p)
    assert {n for n in ss.LENGTHS} >= {1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192, 8193}
    # 64 * ITEMS of every instance, on both sides: 1024 (<64, 16>), 256 (<256, 4> and <1024, 4>), 512 words into the <1024, 8> instance's bucket
    assert {64 * it for _, it in list(ss.SIZING.values()) + list(ss.EMITTING.values())} == {1024, 256, 512}
    assert {1023, 1024, 1025, 255, 256, 257, 4096 + 511, 4096 + 512, 4096 + 513} <= set(ss.LENGTHS)


def test_trie_patterns_are_there():
    roots, mids = {}, {}
    for w in ss.ALL_WIDTHS:
        k, pb, sb, by = ss.geom(w)
        s = ss.shape(ss.craft_patterns, w)
        assert all(kind == "trie" for kind, _ in s.buckets.values())
        labels = set(s.marks.values())
        lay = {s.marks[e.prefix]: e for e in ss.layout(s)}
        for c in ss.FANOUTS:
            if "fanout root %d" % c in labels:
                f = fanouts(_marked(s, "fanout root %d" % c)[1], by)
                assert f[0] == Counter({c: 1}), (w, c)
                roots.setdefault(c, set()).add(w)
            if by >= 2:
                f = fanouts(_marked(s, "fanout mid %d" % c)[1], by)
                assert f[0] == Counter({1: 1}) and f[1] == Counter({c: 1}), (w, c)
                mids.setdefault(c, set()).add(w)
        if by == 1:
            assert fanouts(_marked(s, "dense all")[1], 1)[0] == Counter({256: 1})  # the root is the leaf level
            assert {0, 255} <= set(_marked(s, "sentinels")[1])
            continue
        for cls, n in ss.PATTERN_LENGTHS.items():
            assert lay["dense %s" % cls].cls == lay["sparse %s" % cls].cls == lay["random %s" % cls].cls == cls and lay["dense %s" % cls].n == n
            d = _marked(s, "dense %s" % cls)[1]
            assert d == list(range(d[0], d[0] + n))
            f = fanouts(d, by)
            assert 256 in f[by - 1] and all(f[j] == Counter({1: 1}) for j in range(by - 2)), (w, cls)  # 256 children at the leaves, single chains above
            sp = _marked(s, "sparse %s" % cls)[1]
            f = fanouts(sp, by)
            assert all(f[j] == Counter({1: n}) for j in range(min(3, by), by)) and f[0] == Counter({min(n, 1 << ss.top_bits(sb, by)): 1}), (w, cls)  # a chain of its own per element
            sen = _marked(s, "sentinels %s" % cls)[1]
            assert sen[0] == 0 and sen[-1] == (1 << sb) - 1
            tb = _marked(s, "top bits %s" % cls)[1]
            assert all(x >> (8 * (by - 1)) == (1 << ss.top_bits(sb, by)) - 1 for x in tb) and len(tb) == n
        assert lay["dense c1024"].n == 8192  # ranks up to 8192 in the u16 s_ns
        for j in sorted({0, 7, 8, by - 1}):
            if j >= by:
                continue
            for label in ("only byte %d" % j, "only byte %d, 2" % j):
                if label in labels:
                    items = _marked(s, label)[1]
                    x = 0
                    for a in items[1:]:
                        x |= a ^ items[0]
                    assert x and x >> (8 * j) < 256 and x & ((1 << (8 * j)) - 1) == 0, (w, label)
            assert len(_marked(s, "only byte %d" % j)[1]) == (256 if j < by - 1 else 1 << ss.top_bits(sb, by))
        if by > 9:
            assert {"only byte 7", "only byte 8", "only byte %d" % (by - 1)} <= labels  # top_diff_byte switches words at byte 8
    assert all(roots[c] >= {"narrow64", "b1"} for c in ss.FANOUTS), roots
    assert all(mids[c] == set(ss.ALL_WIDTHS) - {"b1"} for c in ss.FANOUTS), mids


def test_staging_threshold_is_met_from_both_sides_at_every_misalignment():
    s = ss.shape(ss.craft_stage_vecs)
    assert s.by == 15
    seen = Counter()
    for e in ss.layout(s):
        if e.prefix not in s.marks:
            assert e.kind == "trie" and 1 <= e.n <= 16
            continue
        _, cls, _, mis, side = s.marks[e.prefix].split()
        stage = ss.stage_bytes(cls)
        assert e.kind == "vec" and e.cls == cls and e.mis == int(mis) and e.size == ss.vec_size(e.prefix, e.n, 15)
        if side == "under":
            assert e.staged and stage - 16 < e.size + e.mis <= stage, e
        else:
            assert not e.staged and stage < e.size + e.mis <= stage + 16, e
        seen[(cls, e.mis, e.staged)] += 1
    assert seen == Counter({(cls, mis, st): 1 for cls in ss.WG_CLASSES for mis in range(16) for st in (True, False)})
    assert [ss.stage_bytes(c) for c in ss.WG_CLASSES] == [13376, 53312, 106560]
    ns = {cls: {e.n for e in ss.layout(s) if e.cls == cls and e.kind == "vec"} for cls in ss.WG_CLASSES}
    assert 835 in ns["c64"] and 3331 in ns["c256"] and 6659 in ns["c1024"], ns
    for w in ss.STAGE_TRIE_WIDTHS:  # for the <256, 4> emitter a Trie that is staged and, one word longer in its own list, one that is not
        t = ss.shape(ss.craft_stage_tries, w)
        u, o = _layout_of(t, "stage trie under"), _layout_of(t, "stage trie over")
        assert u.cls == o.cls == "c64" and u.kind == o.kind == "trie" and u.staged and not o.staged
        assert u.size + u.mis <= 13376 < o.size + o.mis and 13376 - u.size - u.mis < 64 and o.size + o.mis - 13376 <= 64, (u, o)
    # every class has a staged and a direct Trie; sparse in a wide width is direct, random packed suffixes are staged
    tries = Counter()
    for case in ss.FAMILIES["patterns"] + ss.FAMILIES["lengths"]:
        t = ss.shape(*case)
        for e in ss.layout(t):
            if e.kind == "trie" and e.cls in ss.WG_CLASSES:
                tries[(e.cls, e.staged)] += 1
                m = t.marks.get(e.prefix, "")
                if m.startswith("sparse") and t.width in ("wide", "radix"):
                    assert not e.staged, (t.name, e)
                if m.startswith("random") and t.width == "packed":
                    assert e.staged, (t.name, e)
    assert all(tries[(cls, st)] for cls in ss.WG_CLASSES for st in (True, False)), tries


def test_split_plans_are_there():
    for w in ss.SPLIT_WIDTHS:
        k, pb, sb, by = ss.geom(w)
        T = 1 << ss.top_bits(sb, by)
        s = ss.shape(ss.craft_split, w)
        lay = ss.layout(s)
        lens, good, bad_n, gap = set(), 0, 0, False
        for i, e in enumerate(lay):
            if e.prefix not in s.marks:
                assert e.cls in ("tiny", "c64")
                continue
            assert e.cls == "split" and lay[i - 1].prefix not in s.marks and lay[i + 1].prefix not in s.marks, (w, e)
            counts, classes, bad = ss.split_plan(s.buckets[e.prefix][1], by)
            assert sum(counts) == e.n and not any(counts[T:])
            if s.marks[e.prefix].startswith("split bad"):
                assert bad and sorted(counts)[-1] == ss.SER_CAP1024 + 1 and sorted(counts)[-2] < 10  # bad through exactly one sub-range of 8193
                bad_n += 1
                if s.marks[e.prefix] == "split bad alone":
                    assert sum(1 for c in counts if c) == 1  # one present top byte
            else:
                assert not bad
                good += 1
                if s.marks[e.prefix].startswith("split sub-ranges"):
                    lens |= set(counts)
                    assert counts[0] and counts[T - 1]
                    present = [t for t in range(T) if counts[t]]
                    gap = gap or any(b - a > 1 for a, b in zip(present, present[1:]))  # a gap of absent bytes in the middle
        assert lens >= {0, 1, 1024, 1025, 4096, 4097, 8192} and bad_n == 2 and good >= 2 and gap, (w, lens)
        assert {ss.sub_class(c) for c in lens} == {None, "c64", "c256", "c1024"}
        if T == 256:
            for c0 in (250, 251, 256):
                counts, _, bad = ss.split_plan(_marked(s, "split present %d" % c0)[1], by)
                assert sum(1 for c in counts if c) == c0 and not bad and counts[0] and counts[255]
    assert 1 << ss.top_bits(*ss.geom("narrow64")[2:]) == 256
    assert [ss.sub_class(c) for c in (0, 1, 1024, 1025, 4096, 4097, 8192, 8193)] == [None, "c64", "c64", "c256", "c256", "c1024", "c1024", "over"]


def test_prefix_varints_are_there():
    seen = {}
    for w, v in ss.varint_cases():
        s = ss.shape(ss.craft_varints, w, v)
        k, pb, sb, by = ss.geom(w)
        assert sorted(s.buckets) == ss.varint_prefixes(pb) and 0 in s.buckets and (1 << pb) - 1 in s.buckets
        for e, raw in zip(ss.layout(s), ss.entries(s)):
            assert raw[: ss.vlen(e.prefix)] == pyref.PyCBL._varint(e.prefix)
            seen.setdefault(e.prefix, set()).add((e.kind, e.cls))
    for p in (0, 250, 251, 65535, 65536, (1 << 24) - 1):
        assert seen[p] >= {("vec", "tiny"), ("vec", "c64"), ("trie", "c64")}, (p, seen[p])
    assert ("trie", "split") in seen[250] and ("trie", "split") in seen[251]
    assert [ss.vlen(p) for p in (250, 251, 65535, 65536)] == [1, 3, 3, 5]


def test_chunk_geometry_is_there():
    for w in ss.CHUNK_WIDTHS:
        k, pb, sb, by = ss.geom(w)
        by_case = {c: ss.shape(ss.craft_chunks, w, c) for c in ss.CHUNK_CASES}
        assert [len(by_case[c].buckets) for c in ss.CHUNK_CASES] == [127, 128, 129, 1000, 128, 160, 0]
        assert [len(by_case[c].buckets) >= ss.CHUNKED_MIN_BUCKETS for c in ss.CHUNK_CASES] == [False, True, True, True, True, True, False]
        for c, s in by_case.items():
            nb = len(s.buckets)
            wg = Counter()
            for e in ss.layout(s):
                ch, per = ss.chunk_of(e.rank, nb)
                assert ch < ss.SER_CHUNKS
                if e.cls in ss.WG_CLASSES:
                    wg[ch] += 1
            per = ss.chunk_of(0, nb)[1]
            used = -(-nb // per) if nb else 0
            if c == "129":
                assert per == 5 and used == 26 and nb - 25 * per == 4  # the last chunk short, six chunks with no bucket at all
            if c == "1000":
                assert per == 32 and used == 32 and nb - 31 * per == 8 and nb % 32
            if c == "128":
                assert per == 4 and used == 32
            if c == "tiny_chunk":
                assert wg[3] == 0 and wg[2] and wg[4] and per == 4  # a chunk of `per` buckets with no workgroup launch
            if c == "long_first":
                assert set(wg) == {0} and wg[0] >= 3 and len({e.cls for e in ss.layout(s)} & set(ss.WG_CLASSES)) >= 2
            if c in ("127", "128", "129"):
                assert {e.cls for e in ss.layout(s)} >= {"tiny", "c64", "c256"} and sum(1 for k_ in range(used) if wg[k_]) >= 20


def test_untouched_buckets_of_the_stale_shapes():
    for w in ss.STALE_WIDTHS:
        k, pb, sb, by = ss.geom(w)
        first, second, kept = ss.craft_stale(w)
        m = pyref.PyCBL(k, pb)
        bs.insert_batch(m, first)
        before = {p: (m.buckets[p][0], list(m.buckets[p][1])) for p in kept}
        bs.insert_batch(m, second)
        assert not {x >> sb for x in second} & set(kept) and len(kept) == len(ss.STALE_LENGTHS)
        assert all((m.buckets[p][0], m.buckets[p][1]) == before[p] for p in kept)
        cls = [ss.classify(m.buckets[p][0], len(m.buckets[p][1]), by) for p in kept]
        assert cls == ["c64", "c256", "c1024", "split"] + ["tiny"] * 5 + ["c64"] and [m.buckets[p][0] for p in kept] == ["vec", "trie", "trie", "trie"] + ["vec"] * 6, (w, cls)
        assert [len(m.buckets[p][1]) for p in kept] == list(ss.STALE_LENGTHS) and ss.STALE_LENGTHS.count(1) == 3
        assert all(p >> (pb - 1) == 1 and p & 1 for p in kept)  # bits above SB that a full word would carry
        assert not ss.split_plan(m.buckets[kept[3]][1], by)[2]
        o = Oracle(k, pb)
        o.insert_words(first)
        o.insert_words(second)
        assert o.serialize() == bs.serialize(m), w


# ---- the bytes tell ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["lengths", "patterns", "stage", "split", "varints"])
def test_every_crafted_bucket_shows_in_its_bytes(family):
    """one suffix changed changes the entry, and so does a swap of two stored elements of a Vec"""
    for case in ss.FAMILIES[family]:
        s = ss.shape(*case)
        for p, label in s.marks.items():
            kind, items = s.buckets[p]
            base = ss.entry_bytes(s, p, kind, items)
            have = set(items)
            if len(have) < 1 << s.sb:
                j = len(items) // 2
                new = next(items[j] ^ d for d in range(1, 1 << s.sb) if items[j] ^ d not in have and items[j] ^ d < 1 << s.sb)
                changed = items[:j] + [new] + items[j + 1:]
                assert ss.entry_bytes(s, p, kind, sorted(changed) if kind == "trie" else changed) != base, (s.name, label)
            if kind == "vec" and len(items) > 1:
                sw = list(items)
                sw[0], sw[-1] = sw[-1], sw[0]
                assert ss.entry_bytes(s, p, kind, sw) != base, (s.name, label)
