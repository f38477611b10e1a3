"""|a AND b| on the GPU without building an index (cblx_intersection_count, CBL.intersection_count / set_op_count / intersection_matrix, `cbl compare`)
against plain Python sets. Operands are installed with `CBL.load(PyCBL(...).serialize())` from crafted {prefix: (kind, items)} dicts, so kind, stored
order and length are the test's own. Every case asserts the count, the number of prefixes both hold, the route every such bucket took (the table of
tests/similarity_shapes.py, which tests/host/common_route_unit.cpp holds against the device's rule) and that BOTH OPERANDS SERIALIZE TO THE SAME BYTES
after the call: that is what tells this feature from `&`, which sorts the Vec buckets it visits."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd import CBL, synth  # noqa: E402
from cbl_amd.__main__ import compare_report, main as cli_main  # noqa: E402
from oracle import Oracle  # noqa: E402
from oracle.pyref import PyCBL, params  # noqa: E402

import setops_model as sm  # noqa: E402  (tests/)
import similarity_shapes as ss  # noqa: E402  (tests/)

T = 512  # kernels_setops.hpp UNI_TILE: outputs of one round of k_common_merge
CFGS = [(31, 24), (59, 28)]  # a narrow and a wide suffix


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _sb(k, pb):
    return params(k, pb)["SB"]


def _gpu(m: PyCBL):
    g = CBL(m.P["K"], m.P["PB"], canonical=m.canonical)
    g.load(m.serialize())
    return g


def _side(rng, kind, items):
    """a bucket as stored: a Trie ascending, a Vec shuffled"""
    items = list(items)
    if kind == "trie":
        items.sort()
    else:
        rng.shuffle(items)
    return (kind, items)


def _pair(rng, sb, na, nb, shared):
    """two lists of na and nb distinct values with exactly `shared` in common, in random order"""
    pool = sm.distinct(rng, na + nb - shared, sb)
    common = pool[:shared]
    return common + pool[shared:na], common + pool[na:]


def _route_counts(ba, bb, routes=None):
    cnt = [0] * 4
    for p in set(ba) & set(bb):
        (ka, ia), (kb, ib) = ba[p], bb[p]
        r = routes[p] if routes is not None and p in routes else ss.route(len(ia), len(ib), ka == "trie", kb == "trie")
        cnt[r] += 1
    return dict(zip(ss.ROUTES, cnt))


def _bad_prefixes(k, pb, canonical, ba, bb):
    """after a wrong total: the shared prefixes whose bucket alone is counted wrong (for the assertion's message)"""
    bad = []
    for p in sorted(set(ba) & set(bb)):
        ga, gb = _gpu(sm.from_buckets(k, pb, canonical, {p: ba[p]})), _gpu(sm.from_buckets(k, pb, canonical, {p: bb[p]}))
        got, exp = ga.intersection_count(gb), len(set(ba[p][1]) & set(bb[p][1]))
        if got != exp:
            bad.append((p, ba[p][0], len(ba[p][1]), bb[p][0], len(bb[p][1]), got, exp))
        ga.close()
        gb.close()
    return bad[:12]


def _check(k, pb, ba, bb, routes=None, canonical=False):
    """the four assertions of every case: count, prefixes both hold, routes, operands unchanged to the byte"""
    _need_gpu()
    ma, mb = sm.from_buckets(k, pb, canonical, ba), sm.from_buckets(k, pb, canonical, bb)
    sa, sb_ = ma.serialize(), mb.serialize()
    ga, gb = _gpu(ma), _gpu(mb)
    assert ga.serialize() == sa and gb.serialize() == sb_  # as crafted, stored order included
    exp = len(sm.words(ma) & sm.words(mb))
    n, st = ga.intersection_count(gb, stats=True)
    exp_routes = _route_counts(ba, bb, routes)
    print(f"K={k} PB={pb}: common {n} (expected {exp}), both {st['both']}, routes {st} (expected {exp_routes})")
    assert n == exp, _bad_prefixes(k, pb, canonical, ba, bb)
    assert st["both"] == len(set(ba) & set(bb))
    assert {r: st[r] for r in ss.ROUTES} == exp_routes
    assert ga.serialize() == sa, "left operand after the call"
    assert gb.serialize() == sb_, "right operand after the call"
    assert gb.intersection_count(ga) == exp  # the other order stages the other side on ties
    assert ga.serialize() == sa and gb.serialize() == sb_
    ga.close()
    gb.close()


KIND = ("vec", "trie")


# ---------------------------------------------------------------- route edges
@pytest.mark.parametrize("k,pb", CFGS)
def test_route_edges(k, pb):
    """every row of the hand-written route table whose lengths fit a test: ca + cb = 255 / 256 / 257 three ways, the shorter side at 1023 / 1024 / 1025
    against as many and against 5000 words, all four pairs of kinds, Vecs shuffled; ties (ca == cb, a shuffled Vec, b a Trie) stage a's side"""
    sb, rng = _sb(k, pb), random.Random(k * 131 + pb)
    ba, bb, routes, p = {}, {}, {}, 2
    for ca, cb, ka, kb, r, _ in ss.ROUTE_ROWS:
        if max(ca, cb) > 5000:
            continue
        A, B = _pair(rng, sb, ca, cb, rng.randint(0, min(ca, cb)))
        ba[p], bb[p], routes[p] = _side(rng, KIND[ka], A), _side(rng, KIND[kb], B), r
        p += 5
    assert sorted(set(routes.values())) == [0, 1, 2, 3]
    _check(k, pb, ba, bb, routes)


# ---------------------------------------------------------------- sharing patterns
def _one_shared(rng, sb, na, nb, i, j, kind_a, kind_b):
    """two stored lists with exactly one word in common, which is word i of a's stored order and word j of b's (a Trie's stored order is ascending)"""
    v = 1 << (sb - 1)
    pool = [x for x in sm.distinct(rng, 3 * (na + nb) + 64, sb) if x != v]
    lows, highs = [x for x in pool if x < v], [x for x in pool if x > v]
    assert len(lows) >= i + j and len(highs) >= na + nb - 2 - i - j

    def build(kind, low, high, at):
        if kind == "trie":
            items = sorted(low + [v] + high)
        else:
            rest = low + high
            rng.shuffle(rest)
            items = rest[:at] + [v] + rest[at:]
        assert items[at] == v
        return (kind, items)

    return build(kind_a, lows[:i], highs[:na - 1 - i], i), build(kind_b, lows[i:i + j], highs[na - 1 - i:na + nb - 2 - i - j], j)


SHARING_SHAPES = [(100, 100, "vec", "vec", ss.WAVE), (700, 900, "vec", "trie", ss.WG), (3000, 5000, "trie", "trie", ss.MERGE), (3000, 5000, "vec", "trie", ss.SLICED)]


@pytest.mark.parametrize("k,pb", CFGS)
def test_sharing_patterns(k, pb):
    """none shared, the whole shorter side, a random half, exactly one — the first, the last or the middle word of either side's stored order — at one
    pair of lengths per route"""
    sb, rng = _sb(k, pb), random.Random(k * 17 + pb)
    ba, bb, routes, p = {}, {}, {}, 1
    for na, nb, ka, kb, r in SHARING_SHAPES:
        for shared in (0, na, na // 2):
            A, B = _pair(rng, sb, na, nb, shared)
            ba[p], bb[p], routes[p] = _side(rng, ka, A), _side(rng, kb, B), r
            p += 3
        for i in (0, na // 2, na - 1):
            for j in (0, nb // 2, nb - 1):
                ba[p], bb[p] = _one_shared(rng, sb, na, nb, i, j, ka, kb)
                routes[p] = r
                p += 3
    _check(k, pb, ba, bb, routes)


# ---------------------------------------------------------------- merge-path round edges
MERGE_LENS = (1025, 1536, 1537, 2049, 5000)


@pytest.mark.parametrize("pattern", ["straddling", "all_shared", "none_shared"])
@pytest.mark.parametrize("k,pb", CFGS)
def test_merge_round_edges(k, pb, pattern):
    """two Tries longer than a table: a's copy of a pair is the last output of every round and b's the first of the next; everything shared; nothing"""
    sb, rng = _sb(k, pb), random.Random(k * 7 + pb + len(pattern))
    ba, bb, routes, p = {}, {}, {}, 4
    for na in MERGE_LENS:
        for nb in MERGE_LENS:
            if pattern == "straddling":
                A, B = sm.straddling_lists(na, nb, T, rng, bits=sb)
                assert len(set(A) & set(B)) == min((na + nb - 1) // T, na, nb)
            elif pattern == "all_shared":
                big = sm.distinct(rng, max(na, nb), sb)
                small = rng.sample(big, min(na, nb))
                A, B = (big, small) if na >= nb else (small, big)
            else:
                A, B = _pair(rng, sb, na, nb, 0)
            ba[p], bb[p], routes[p] = ("trie", sorted(A)), ("trie", sorted(B)), ss.MERGE
            p += 9
    _check(k, pb, ba, bb, routes)


# ---------------------------------------------------------------- slice edges
@pytest.mark.parametrize("pattern", ["slice_edges", "all_shared"])
@pytest.mark.parametrize("k,pb", CFGS)
def test_slice_edges(k, pb, pattern):
    """a shuffled Vec of 1025 / 2048 / 2049 / 5000 words against a Vec and against a Trie of 5000, in both orders; shared are the words stored at
    positions 1023, 1024, 2047 and 2048 of the staged (shorter; a's on a tie) side — the last of a slice and the first of the next — or all of it"""
    sb, rng = _sb(k, pb), random.Random(k * 29 + pb + len(pattern))
    ba, bb, routes, p = {}, {}, {}, 0
    for n in (1025, 2048, 2049, 5000):
        for other_kind in KIND:
            for vec_is_a in (True, False):
                pool = sm.distinct(rng, n + 5000, sb)
                mine, fill = pool[:n], pool[n:]  # (`mine`: the stored order of the shuffled Vec)

                def pick(stored):
                    return list(stored) if pattern == "all_shared" else [stored[i] for i in (1023, 1024, 2047, 2048) if i < len(stored)]

                if n < 5000 or vec_is_a:  # the Vec is the staged side
                    shared = pick(mine)
                    other = _side(rng, other_kind, shared + fill[:5000 - len(shared)])
                else:  # a tie with the other side as a: that one is staged
                    other = _side(rng, other_kind, fill)
                    shared = pick(other[1])
                    mine = shared + mine[:n - len(shared)]
                    rng.shuffle(mine)
                mine = ("vec", mine)
                assert len(mine[1]) == n and len(other[1]) == 5000 and len(set(mine[1]) & set(other[1])) == len(shared)
                ba[p], bb[p] = (mine, other) if vec_is_a else (other, mine)
                routes[p] = ss.SLICED
                p += 11
    _check(k, pb, ba, bb, routes)


# ---------------------------------------------------------------- values
@pytest.mark.parametrize("k,pb", [(33, 10), (33, 9), (33, 8), (5, 8)])  # SUFFIX_BITS 63, 64, 65 and 6, the set tests/test_gpu_setops.py uses
def test_suffix_widths_and_special_values(k, pb):
    """suffix 0 and the all-ones suffix shared, held by a only, held by b only, at staged lengths that are no powers of two in the wave and the
    workgroup route (the table stores indices: no value is set apart); wide suffixes that agree in one half and differ in the other; lists that
    would pile up in a table with a weak hash"""
    sb = _sb(k, pb)
    assert sb == {(33, 10): 63, (33, 9): 64, (33, 8): 65, (5, 8): 6}[(k, pb)]
    ones, rng = (1 << sb) - 1, random.Random(sb)
    shapes = [(37, 90), (700, 1500)] if sb > 12 else [(5, 40), (23, 30)]  # (6 bits: 64 values in all, the wave route only)
    ba, bb, p = {}, {}, 0
    for na, nb in shapes:
        for special in ((0,), (ones,), (0, ones)):
            for place in ("shared", "a_only", "b_only"):
                for ka, kb in (("vec", "trie"), ("trie", "vec"), ("vec", "vec")):
                    pool = [x for x in sm.distinct(rng, na + nb, sb) if x not in (0, ones)]
                    A, B = pool[:na - len(special)], pool[na:na + nb - len(special)]
                    half = len(A) // 2
                    B = A[:half] + B[half:]  # half of a's other words are shared
                    if place != "b_only":
                        A = A + list(special)
                    if place != "a_only":
                        B = B + list(special)
                    ba[p], bb[p] = _side(rng, ka, A), _side(rng, kb, B)
                    p += 1
    if sb > 64:  # pairs that agree in the low 64 bits and differ above, and the reverse: neither may count
        for na, ka, kb in ((60, "vec", "vec"), (900, "vec", "trie"), (900, "trie", "trie")):
            A = [x & ~((1 << 64) | 1) for x in sm.distinct(rng, na, sb)]
            A = list(dict.fromkeys(A))
            B = [x | (1 << 64) for x in A[::2]] + [x | 1 for x in A[1::2]] + A[:7]
            ba[p], bb[p] = _side(rng, ka, A), _side(rng, kb, B)
            p += 1
    if sb >= 40:  # hash-adversarial lists: consecutive suffixes, multiples of 2^20, values that differ in their top 11 bits only
        low = rng.getrandbits(sb - 11)
        for gen, cap in ((lambda i: i, 1 << 20), (lambda i: i << 20, 1 << 20), (lambda i: (i << (sb - 11)) | low, 1 << 11)):
            for na, nb, ka, kb in ((100, 150, "vec", "vec"), (1024, 2000, "vec", "trie"), (2000, 1024, "trie", "vec")):
                idx = rng.sample(range(min(cap, 4096)), min(cap, 4096))
                A, B = [gen(i) for i in idx[:na]], [gen(i) for i in idx[na // 2:na // 2 + nb]]
                ba[p], bb[p] = _side(rng, ka, A), _side(rng, kb, B)
                p += 1
    top_p = (1 << pb) - 1
    ba[top_p], bb[top_p] = ("vec", [ones, 0]), ("trie", [0, ones])
    _check(k, pb, ba, bb)


@pytest.mark.parametrize("k,pb", CFGS)
def test_adversarial_lists_in_every_route(k, pb):
    """consecutive suffixes and multiples of 2^20 through the sliced and the merge-path route as well"""
    sb, rng = _sb(k, pb), random.Random(99)
    ba, bb, routes, p = {}, {}, {}, 7
    for gen in (lambda i: i, lambda i: i << 20):
        for ka, kb, r in (("vec", "trie", ss.SLICED), ("trie", "trie", ss.MERGE)):
            idx = rng.sample(range(8192), 8192)
            A, B = [gen(i) for i in idx[:3000]], [gen(i) for i in idx[1500:6500]]
            ba[p], bb[p], routes[p] = _side(rng, ka, A), _side(rng, kb, B), r
            p += 13
    _check(k, pb, ba, bb, routes)


# ---------------------------------------------------------------- masking: a built arena against a loaded one
@pytest.mark.parametrize("canonical", [False, True])
@pytest.mark.parametrize("k,pb", [(31, 24), (15, 6), (31, 3)])
def test_built_against_loaded(k, pb, canonical):
    """one operand built on the GPU from reads, the other loaded from the oracle's build of an overlapping read set: the two arenas need not agree above
    the suffix bits, so a compare that forgets the mask counts too few"""
    _need_gpu()
    ra, rb = synth.reads(11, 600, 150, 0), synth.reads(11, 600, 150, 300)
    oa, ob = Oracle(k, pb, canonical), Oracle(k, pb, canonical)
    oa.insert_seqs(*ra)
    ob.insert_seqs(*rb)
    exp = len(set(oa.iter_words()) & set(ob.iter_words()))
    assert 0 < exp < min(oa.count(), ob.count())
    for built, loaded, exp_ser in ((ra, ob, oa.serialize()), (rb, oa, ob.serialize())):
        g, h = CBL(k, pb, canonical=canonical), CBL(k, pb, canonical=canonical)
        g.insert_seqs(*built)
        h.load(loaded.serialize())
        assert g.serialize() == exp_ser
        for x, y in ((g, h), (h, g)):
            n, st = x.intersection_count(y, stats=True)
            print(f"K={k} PB={pb} canonical={canonical}: common {n} (expected {exp}), {st}")
            assert n == exp
            assert st["both"] == sum(st[r] for r in ss.ROUTES) > 0
        assert g.serialize() == exp_ser and h.serialize() == loaded.serialize()
        g.close()
        h.close()


# ---------------------------------------------------------------- operands left by earlier operations
def test_operands_with_slack_in_their_arenas():
    """a = x | y and b after b |= z: Vec buckets of 1025 and 5000 words and more, arenas with slack inside the runs"""
    _need_gpu()
    k, pb = 31, 24
    sb, rng = _sb(k, pb), random.Random(5)
    pool = sm.distinct(rng, 30000, sb)
    x = {3: _side(rng, "vec", pool[:1025]), 9: _side(rng, "vec", pool[2000:7000]), 12: _side(rng, "vec", pool[9000:9040])}
    y = {3: _side(rng, "vec", pool[1000:1060]), 9: _side(rng, "trie", pool[6900:8200]), 40: _side(rng, "vec", pool[9100:9200])}
    b0 = {3: _side(rng, "vec", pool[500:1100]), 9: _side(rng, "trie", pool[4000:7500]), 12: _side(rng, "vec", pool[9020:9030]), 40: _side(rng, "trie", pool[9150:10400])}
    z = {3: _side(rng, "vec", pool[1040:1500]), 9: _side(rng, "vec", pool[7400:7700]), 12: _side(rng, "trie", pool[9000:9025])}
    mx, my, mb0, mz = (sm.from_buckets(k, pb, False, d) for d in (x, y, b0, z))
    gx, gy, b, gz = _gpu(mx), _gpu(my), _gpu(mb0), _gpu(mz)
    a = CBL.set_op(gx, gy, "or")
    b |= gz
    wa, wb = sm.words(mx) | sm.words(my), sm.words(mb0) | sm.words(mz)
    assert a.count() == len(wa) and b.count() == len(wb)
    sa, sb_ = a.serialize(), b.serialize()
    tabs = []
    for g in (a, b):
        prefix, length, kind = g.bucket_table_np()
        tabs.append({int(p_): (KIND[int(kd)], [None] * int(ln)) for p_, ln, kd in zip(prefix, length, kind)})
    exp_routes = _route_counts(tabs[0], tabs[1])
    assert exp_routes["sliced"] >= 1 and exp_routes["workgroup"] >= 1 and exp_routes["wave"] >= 1
    n, st = a.intersection_count(b, stats=True)
    print(f"common {n} (expected {len(wa & wb)}), {st} (expected {exp_routes})")
    assert n == len(wa & wb) and b.intersection_count(a) == n
    assert st["both"] == len(set(tabs[0]) & set(tabs[1])) and {r: st[r] for r in ss.ROUTES} == exp_routes
    assert a.serialize() == sa and b.serialize() == sb_
    a2, b2 = CBL(k, pb), CBL(k, pb)
    a2.load(sa)
    b2.load(sb_)
    d = CBL.set_op(a2, b2, "and")
    assert d.count() == n
    for g in (gx, gy, gz, a, b, a2, b2, d):
        g.close()


# ---------------------------------------------------------------- contract
def _mixed(k, pb, seed):
    """two overlapping bucket dicts with one bucket per route, one-sided buckets on both sides, Vecs shuffled"""
    sb, rng = _sb(k, pb), random.Random(seed)
    ba, bb, p = {}, {}, 6
    for na, nb, ka, kb, _ in SHARING_SHAPES:
        A, B = _pair(rng, sb, na, nb, na // 3)
        ba[p], bb[p] = _side(rng, ka, A), _side(rng, kb, B)
        p += 10
    ba[1], bb[2] = _side(rng, "vec", sm.distinct(rng, 50, sb)), _side(rng, "trie", sm.distinct(rng, 1500, sb))
    return ba, bb


def test_pending_inserts_count():
    _need_gpu()
    k, pb = 31, 24
    ra, rb = synth.reads(3, 40, 150, 0), synth.reads(3, 40, 150, 20)
    a, b = CBL(k, pb), CBL(k, pb)
    oa, ob = Oracle(k, pb), Oracle(k, pb)
    for g, o, (bases, off) in ((a, oa, ra), (b, ob, rb)):
        for i in range(len(off) - 1):
            seq = bases[int(off[i]):int(off[i + 1])].tobytes()
            g.insert_seq(seq)  # no flush
            o.insert_seq(seq)
    exp = len(set(oa.iter_words()) & set(ob.iter_words()))
    assert exp > 0
    assert a.intersection_count(b) == exp
    assert a.count() == oa.count() and b.count() == ob.count()
    a.close()
    b.close()


def test_self_and_empty_operands():
    _need_gpu()
    k, pb = 31, 24
    ba, _ = _mixed(k, pb, 1)
    a, e, e2 = _gpu(sm.from_buckets(k, pb, False, ba)), CBL(k, pb), CBL(k, pb)
    zero = dict.fromkeys(("both",) + ss.ROUTES, 0)
    assert a.intersection_count(a) == a.count() > 0
    assert a.intersection_count(a, stats=True) == (a.count(), zero)
    for x, y in ((a, e), (e, a), (e, e2), (e, e)):
        assert x.intersection_count(y, stats=True) == (0, zero)
    assert a.jaccard(a) == 1.0 and a.containment(e) == 0.0 and e.containment(a) == 1.0 and e.jaccard(e2) == 1.0
    for g in (a, e, e2):
        g.close()


def test_stage_timer_common():
    """with FLAG_PROFILE the call's device time goes under the stage `common`, and under no stage of the build or the set algebra"""
    _need_gpu()
    k, pb = 31, 24
    ba, bb = _mixed(k, pb, 6)
    a, b = CBL(k, pb, profile=True), CBL(k, pb, profile=True)
    a.load(sm.from_buckets(k, pb, False, ba).serialize())
    b.load(sm.from_buckets(k, pb, False, bb).serialize())
    a.stage_times_reset()
    n = a.intersection_count(b)
    assert n == len(sm.words(sm.from_buckets(k, pb, False, ba)) & sm.words(sm.from_buckets(k, pb, False, bb)))
    st = a.stage_times()
    assert st["common"][1] == 1 and st["common"][0] > 0.0
    assert all(launches == 0 for name, (_, launches) in st.items() if name != "common")
    a.close()
    b.close()


def test_mismatched_operands_are_refused():
    _need_gpu()
    ba, _ = _mixed(31, 24, 2)
    a = _gpu(sm.from_buckets(31, 24, False, ba))
    sa = a.serialize()
    others = [_gpu(sm.from_buckets(29, 24, False, {5: ("vec", [1, 2, 3])})), _gpu(sm.from_buckets(31, 22, False, {5: ("vec", [1, 2, 3])})),
              _gpu(sm.from_buckets(31, 24, True, {5: ("vec", [1, 2, 3])}))]
    for o in others:
        so = o.serialize()
        for x, y in ((a, o), (o, a)):
            with pytest.raises(cbl_amd.CblxError) as e:
                x.intersection_count(y)
            assert e.value.code == cbl_amd.EINVAL
            with pytest.raises(cbl_amd.CblxError) as e:
                CBL.intersection_matrix([x, y])
            assert e.value.code == cbl_amd.EINVAL
        assert a.serialize() == sa and o.serialize() == so
    with pytest.raises(cbl_amd.CblxError) as e:
        a.intersection_count(others[2])
    assert "canonical" in str(e.value)
    for g in [a] + others:
        g.close()


def test_set_op_count_equals_the_built_result():
    _need_gpu()
    k, pb = 31, 24
    ba, bb = _mixed(k, pb, 3)
    for op in sm.OPS:  # (the built result sorts the operands' Vec buckets: fresh operands per op)
        a, b = _gpu(sm.from_buckets(k, pb, False, ba)), _gpu(sm.from_buckets(k, pb, False, bb))
        n = CBL.set_op_count(a, b, op)
        d = CBL.set_op(a, b, op)
        assert n == d.count() == len(sm.algebra(op, sm.words(sm.from_buckets(k, pb, False, ba)), sm.words(sm.from_buckets(k, pb, False, bb))))
        for g in (a, b, d):
            g.close()


# ---------------------------------------------------------------- matrix and CLI
def _four(k, pb):
    ba, bb = _mixed(k, pb, 4)
    ms = [sm.from_buckets(k, pb, False, ba), sm.from_buckets(k, pb, False, bb), sm.from_buckets(k, pb, False, {}), sm.from_buckets(k, pb, False, ba)]
    ws = [sm.words(m) for m in ms]
    return ms, np.array([[len(x & y) for y in ws] for x in ws], dtype=np.uint64)


def test_intersection_matrix():
    """four indexes, one of them empty and one the clone of another"""
    _need_gpu()
    k, pb = 31, 24
    ms, exp = _four(k, pb)
    gs = [_gpu(m) for m in ms]
    sers = [g.serialize() for g in gs]
    got = CBL.intersection_matrix(gs)
    assert got.dtype == np.uint64 and got.shape == (4, 4)
    assert (got == got.T).all() and [int(got[i, i]) for i in range(4)] == [g.count() for g in gs]
    assert (got == exp).all(), (got, exp)
    assert [g.serialize() for g in gs] == sers
    one = CBL.intersection_matrix(gs[:1])
    assert one.shape == (1, 1) and int(one[0, 0]) == gs[0].count()
    many = [CBL(k, pb) for _ in range(65)]
    for bad in ([], [gs[0], gs[1], gs[0]], many):
        with pytest.raises(cbl_amd.CblxError) as e:
            CBL.intersection_matrix(bad)
        assert e.value.code == cbl_amd.EINVAL
    assert (CBL.intersection_matrix(many[:64]) == 0).all()
    for g in gs + many:
        g.close()


def test_cli_compare(tmp_path, capsys):
    _need_gpu()
    k, pb = 31, 24
    ms, exp = _four(k, pb)
    paths = []
    for i, m in enumerate(ms[:3]):
        paths.append(str(tmp_path / f"i{i}.cbl"))
        (tmp_path / f"i{i}.cbl").write_bytes(m.serialize())
    capsys.readouterr()
    cli_main(["-k", str(k), "--prefix-bits", str(pb), "compare"] + paths)
    out = capsys.readouterr()
    lines, human = compare_report(exp[:3, :3])
    assert out.out.splitlines() == lines and len(lines) == 3
    assert out.err.splitlines()[-3:] == human
