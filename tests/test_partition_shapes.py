"""What tests/partition_shapes.py delivers for tests/test_gpu_partition_edges.py, checked on the CPU. Every configuration has the plan and the
record layout it is named for; every named piece — batch sizes, segment, group and run lengths, directory positions, sub-prefix fills — is found
in the crafted words by the restated segment, group and run arithmetic, not by the crafter's bookkeeping; every shape of more than one tile has
a Vec bucket whose bytes depend on the order across the edge it is crafted for; and the closed-form model equals the C++ oracle byte for byte on
every shape. Nothing here is skipped: a shape that cannot deliver a piece fails. Run with -s to see the table of what is delivered."""
import os
import re

import numpy as np
import pytest

import build_shapes as bs
import partition_shapes as ps
from oracle import Oracle, pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFGS = [(k, pb) for _, k, pb in ps.CONFIGS]
NAMED_SIZES = {0, 1, 4095, 4096, 4097, 8192, 8193}
NAMED_GROUPS = {0, 1, 4095, 4096, 4097}
NAMED_RUNS = {1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193}

# (K, PB): SUFFIX_BITS, nA, widths of the LSD passes, xb, hi bytes — written out from the issue's table, not from lsd_plan
EXPECT = {
    (31, 4): (64, 4, [], 0, 1), (31, 8): (60, 8, [], 0, 1), (21, 6): (42, 6, [], 0, 0), (59, 8): (117, 8, [], 0, 8),
    (31, 9): (59, 8, [1], 0, 1), (31, 16): (52, 8, [8], 0, 1),
    (31, 17): (51, 8, [8, 1], 0, 1), (31, 24): (44, 8, [8, 8], 0, 1), (21, 24): (24, 8, [8, 8], 0, 0), (59, 24): (101, 8, [8, 8], 0, 8),
    (27, 25): (35, 8, [8, 8], 1, 0), (31, 26): (42, 8, [8, 8], 2, 1), (31, 28): (40, 8, [8, 8], 4, 1), (59, 28): (97, 8, [8, 8], 4, 8),
}


def _shape(k, pb, name):
    return bs.shape(ps.craft, k, pb, name)


def prefix_array(k, pb, name):
    s = _shape(k, pb, name)
    return np.array([w >> s.sb for w in s.words], dtype=np.int64)


def _prefixes(k, pb, name):
    return bs.shape(prefix_array, k, pb, name)


# ---- the restated arithmetic on arrays of prefixes (ps.segment, ps.digit, ps.group, ps.run_of are the same on single prefixes) ------------------
def _seg(C, p):
    return p >> (C["pb"] - C["nA"])


def _dig(C, p, i):
    sh, w = C["passes"][i]
    return (p >> sh) & ((1 << w) - 1)


def _grp(C, p):
    return (_seg(C, p) << C["passes"][0][1]) | _dig(C, p, 0)


def pos_within(keys):
    """position of every record among the records of equal key, in stream order: where a stable partition by `keys` puts it inside its piece"""
    order = np.argsort(keys, kind="stable")
    sk = keys[order]
    new = np.r_[True, sk[1:] != sk[:-1]]
    starts = np.flatnonzero(new)
    pos = np.empty(len(keys), dtype=np.int64)
    pos[order] = np.arange(len(keys)) - starts[np.cumsum(new) - 1]
    return pos


def test_configs_have_the_plan_and_record_layout_they_are_named_for():
    assert sorted(CFGS) == sorted(EXPECT)
    for route, k, pb in ps.CONFIGS:
        C, P = ps.props(k, pb), pyref.params(k, pb)
        sb, nA, widths, xb, hb = EXPECT[(k, pb)]
        assert (P["SB"], C["sb"], C["nA"], [w for _, w in C["passes"]], C["xb"], C["hi_bytes"]) == (sb, sb, nA, widths, xb, hb), (k, pb)
        assert C["npass"] == len(widths) and nA + sum(widths) + xb == pb and P["WB"] == sb + pb <= 128
        assert hb == (0 if P["WB"] <= 64 else 1 if P["WB"] <= 72 else 8)
        if C["passes"]:  # the passes tile the prefix bits between the split's and pass A's, lowest first
            assert C["passes"][0][0] == xb and all(a[0] + a[1] == b[0] for a, b in zip(C["passes"], C["passes"][1:]))
            assert sum(C["passes"][-1]) == pb - nA
        if route == "a_only_hi_is_digit":
            assert sb == 64 and nA == P["WB"] - 64 == pb and not widths and hb == 1  # the segment is the dropped hi byte: k_boundaries_seg
        elif route == "a_only":
            assert not widths and not xb
        elif route == "one_pass":
            assert len(widths) == 1 and not xb  # low_bits = 0: the groups are the segments, no group cut
        elif route == "two_pass":
            assert len(widths) == 2 and widths[0] == 8 and nA + widths[0] <= 16 and not xb  # tbl_dir and grp_tiles
        else:
            assert pb > 24 and xb == pb - 24 and widths == [8, 8]
    assert {EXPECT[kp][3] for kp in ps.ROUTES["split"]} == {1, 2, 4} and [EXPECT[kp][4] for kp in ps.ROUTES["split"]] == [0, 1, 1, 8]
    assert [EXPECT[kp][4] for kp in ps.ROUTES["a_only"]] == [1, 0, 8] and EXPECT[(21, 6)][1] < 8
    assert [EXPECT[kp][4] for kp in ps.ROUTES["two_pass"]] == [1, 1, 0, 8] and [EXPECT[kp][2] for kp in ps.ROUTES["one_pass"]] == [[1], [8]]
    for k, pb in CFGS:  # the single-prefix functions against the array ones
        C = ps.props(k, pb)
        p = np.array([0, 1, (1 << pb) - 1, (1 << pb) // 3, 0x5A5A5A5 & ((1 << pb) - 1)], dtype=np.int64)
        assert [ps.segment(int(x), pb) for x in p] == _seg(C, p).tolist()
        assert all([ps.digit(int(x), pb, i) for x in p] == _dig(C, p, i).tolist() for i in range(C["npass"]))
        if C["npass"] == 2:
            assert [ps.group(int(x), pb) for x in p] == _grp(C, p).tolist()
            assert all(ps.prefix_of(C, ps.segment(int(x), pb), ps.digit(int(x), pb, 1), ps.digit(int(x), pb, 0), ps.sub_of(int(x), pb)) == x for x in p)
        assert [(ps.run_of(int(x), pb) << C["xb"]) | ps.sub_of(int(x), pb) for x in p] == p.tolist()


def test_constants_mirror_the_kernels():
    with open(os.path.join(ROOT, "cbl_amd", "csrc", "kernels_radix.hpp")) as f:
        kr = f.read()
    const = lambda name: int(re.search(r"\b%s = (\d+)\b" % name, kr).group(1))
    assert const("RDX_THREADS") * const("RDX_ITEMS") == ps.TILE and "RDX_TILE = RDX_THREADS * RDX_ITEMS" in kr
    assert "GRP_COLD_MAX = 64 * RDX_TILE" in kr and ps.GRP_COLD_MAX == 64 * ps.TILE == 262144
    assert "seg_start[s + 1] - seg_start[s] < GRP_COLD_MAX" in kr  # 262,143 cold, 262,144 hot
    assert const("SPLIT_ITEMS") == ps.SPLIT_ITEMS
    assert "c <= 64 * SPLIT_ITEMS ? 0 : (c <= 128 * SPLIT_ITEMS ? 1 : (c <= 256 * SPLIT_ITEMS ? 2 : 3))" in kr
    assert re.search(r"k_prefix_split<H, 512>", open(os.path.join(ROOT, "cbl_amd", "csrc", "pipeline.hpp")).read())
    assert [ps.split_tile(n) for n in (1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)] == [512, 512, 1024, 1024, 2048, 2048, 4096, 4096, 4096]
    assert ps.VEC_DISTINCT < bs.THRESHOLD == pyref.THRESHOLD  # every crafted bucket stays a Vec


def _ragged(C, p):
    """The ragged last tile of pass A lies in the last segment, and the ragged last tile of the last segment in every LSD pass — taken in the order
    that pass reads the segment in — holds a record whose digit in that pass is all ones (the value the tail slots are given)."""
    last = C["nseg"] - 1
    r = len(p) % ps.TILE
    assert r and (_seg(C, p[-r:]) == last).all()
    q = p[_seg(C, p) == last]
    rr = len(q) % ps.TILE
    assert rr
    for i, (_, w) in enumerate(C["passes"]):
        assert (_dig(C, q[-rr:], i) == (1 << w) - 1).any(), (C["k"], C["pb"], i)
        q = q[np.argsort(_dig(C, q, i), kind="stable")]
    return r, rr


def _decode(C, p):
    return ps.segment(p, C["pb"]), ps.digit(p, C["pb"], 1), ps.digit(p, C["pb"], 0), ps.sub_of(p, C["pb"])


def _fills_of(subs, nb):
    """which of the named fills a run's sub-prefixes, in stream order, are"""
    have, n = set(subs.tolist()), len(subs)
    out = set()
    if have == {0}:
        out.add("first")
    if have == {nb - 1}:
        out.add("last")
    if len(have) == nb and n >= nb:
        if (subs == np.arange(n) % nb).all():
            out.add("interleaved")
        if (np.diff(subs) <= 0).all():
            out.add("blocks_desc")
    if len(have) == nb - 1:
        out.add("all_but_one")
    return out


@pytest.mark.parametrize("k,pb", CFGS)
def test_every_named_piece_is_in_the_crafted_words(k, pb):
    C = ps.props(k, pb)
    names = ps.shape_names(k, pb)
    ones = (1 << pb) - 1
    lines = []
    # 1. batch and segment geometry
    assert [len(_shape(k, pb, "n%d" % n).words) for n in (1, 4095, 4096, 4097)] == [1, 4095, 4096, 4097]
    p = _prefixes(k, pb, "segments")
    cnt = np.bincount(_seg(C, p), minlength=C["nseg"])
    assert set(cnt[:8].tolist()) == NAMED_SIZES and cnt[0] in NAMED_SIZES - {0} and cnt[-1] in NAMED_SIZES - {0}
    assert any(cnt[i] and not cnt[i - 1] and not cnt[i + 1] for i in range(1, C["nseg"] - 1))
    lines.append("segments: N=%d, segments 0..7 %s, last %d, ragged tiles %s" % (len(p), cnt[:8].tolist(), cnt[-1], _ragged(C, p)))
    p = _prefixes(k, pb, "last_segment")
    assert (_seg(C, p) == C["nseg"] - 1).all() and len(p) > ps.TILE
    lines.append("last_segment: N=%d, ragged tiles %s" % (len(p), _ragged(C, p)))
    # 2. directory positions
    p = _prefixes(k, pb, "directory")
    S = set(p.tolist())
    assert {x for x in (0, 1, 63, 64, 65, ones) if x <= ones} <= S
    assert any(x + 1 in S and ps.segment(x, pb) != ps.segment(x + 1, pb) for x in S)
    once = {int(x) for x, c in zip(*np.unique(p, return_counts=True)) if c == 1}
    if C["npass"] == 2:
        dmax = (1 << C["passes"][1][1]) - 1
        edges = set()
        for x in S:
            seg, d, low, sub = _decode(C, x)
            if d == dmax and sub == C["nb"] - 1 and (low < 255 or seg + 1 < C["nseg"]):
                nxt = ps.prefix_of(C, seg + (low == 255), 0, (low + 1) & 255, 0)
                if nxt in S:
                    assert ps.group(nxt, pb) == ps.group(x, pb) + 1
                    edges.add(low == 255)
        assert edges == {False, True}  # a group edge inside a segment, and one that is a segment edge too
    if C["pps"] <= ps.FULL_SEGMENT_MAX:
        full = [s for s in range(C["nseg"]) if all(s * C["pps"] + i in once for i in range(C["pps"]))]
        assert full
        lines.append("directory: %d buckets; segment %s whole (%d prefixes, one record each)" % (len(S), full, C["pps"]))
    else:
        by_group, by_col = {}, {}
        for x in once:
            seg, d, low, sub = _decode(C, x)
            by_group.setdefault((seg, low), set()).add(d)
            by_col.setdefault((seg, d), set()).add(low)
        g = [key for key, v in by_group.items() if len(v) == dmax + 1]
        c = [key for key, v in by_col.items() if len(v) == 256]
        assert g and c
        assert C["xb"] == 0 or len({ps.sub_of(x, pb) for x in once}) == C["nb"]
        lines.append("directory: %d buckets; group (segment, low) %s whole, last-pass column (segment, digit) %s whole" % (len(S), g, c))
    if "all_prefixes" in names:
        p = _prefixes(k, pb, "all_prefixes")
        u, c = np.unique(p, return_counts=True)
        assert len(u) == 1 << pb and (c == 1).sum() == (1 << pb) - len(ps.ALL_PREFIXES_WITNESS) and (np.diff(p) < 0).sum() > len(p) // 4
        lines.append("all_prefixes: N=%d, %d prefixes, %d of them once" % (len(p), len(u), (c == 1).sum()))
    assert ("all_prefixes" in names) == ((k, pb) == (31, 16))
    # 3. hot and cold segments
    assert ("hot_cold" in names) == ("hot_last" in names) == ((k, pb) in ((31, 17), (21, 24), (31, 26)))
    if "hot_cold" in names:
        longest = 128 if pb >= 24 else 4097 // 2 + 1  # (PB = 17: a group has two prefixes, so a group of 4097 records has a bucket of 2049)
        p = _prefixes(k, pb, "hot_cold")
        cnt = np.bincount(_seg(C, p), minlength=256)
        nz = np.flatnonzero(cnt)
        assert len(nz) == 2 and nz[1] == nz[0] + 1 and cnt[nz].tolist() == [262143, 262144]
        assert cnt[nz[0]] < ps.GRP_COLD_MAX <= cnt[nz[1]] and len(p) < 800_000
        gc = np.bincount(_dig(C, p[_seg(C, p) == nz[1]], 0), minlength=256)
        assert set(gc.tolist()) >= NAMED_GROUPS and gc[0] == 0 and any(gc[i] == 0 and gc[i + 1] > 0 for i in range(1, 255))
        assert np.bincount(_dig(C, p[_seg(C, p) == nz[0]], 0), minlength=256).min() > 0
        assert np.unique(p, return_counts=True)[1].max() <= longest
        lines.append("hot_cold: segments %s of %s records; groups 0..5 of the hot one %s, the others %d..%d; longest bucket %d" % (
            nz.tolist(), cnt[nz].tolist(), gc[:6].tolist(), gc[6:].min(), gc[6:].max(), np.unique(p, return_counts=True)[1].max()))
        p = _prefixes(k, pb, "hot_last")
        assert (_seg(C, p) == 255).all() and len(p) == 262145 >= ps.GRP_COLD_MAX
        gc = np.bincount(_dig(C, p, 0), minlength=256)
        assert set(gc.tolist()) >= NAMED_GROUPS and gc[0] > 0 and gc[255] > 0 and any(gc[i] == 0 and gc[i + 1] > 0 for i in range(255))
        assert np.unique(p, return_counts=True)[1].max() <= longest
        lines.append("hot_last: segment 255 of %d records; groups 0..5 %s, group 255 %d" % (len(p), gc[:6].tolist(), gc[255]))
    # 4. split runs
    assert ("runs" in names) == (pb > 24)
    if "runs" in names:
        p = _prefixes(k, pb, "runs")
        nb = C["nb"]
        run = p >> C["xb"]
        supers, lens = np.unique(run, return_counts=True)
        assert set(lens.tolist()) == NAMED_RUNS and sorted(lens.tolist()) == sorted(ps.RUN_LENGTHS)
        assert {ps.split_tile(int(n)) for n in lens} == {512, 1024, 2048, 4096}
        assert any(n > ps.SPLIT_TILE and n % ps.SPLIT_TILE == 1 for n in lens)  # a last tile of one record
        assert supers[0] == 0 and supers[-1] == (1 << 24) - 1 and (np.diff(supers) == 1).any()
        met = {}
        for sp, n in zip(supers, lens):
            for f in _fills_of(p[run == sp] & (nb - 1), nb):
                met.setdefault(f, set()).add(n > ps.SPLIT_TILE)
        assert met == {f: {False, True} for f in ps.RUN_FILLS}, met  # every fill meets a one-tile and a multi-tile run
        if C["xb"] == 4:
            S = set(p.tolist())
            top = [int(sp) for sp in supers if (int(sp) << 4) & 63 == 48 and (int(sp) << 4 | 15) in S and (int(sp) + 1) << 4 in S]
            assert top and all(((sp + 1) << 4) & 63 == 0 for sp in top)
        lines.append("runs: " + "; ".join("%d@%#x %s" % (n, sp, "/".join(sorted(_fills_of(p[run == sp] & (nb - 1), nb)))) for sp, n in zip(supers, lens)))
    print("\nK=%d PB=%d: SB=%d nA=%d passes=%s xb=%d hi_bytes=%d" % (k, pb, C["sb"], C["nA"], C["passes"], C["xb"], C["hi_bytes"]))
    for ln in lines:
        print("  " + ln)


def _edge_tiles(C, p, edge):
    """the tile every record is in when the stage of `edge` reads it; -1: the edge does not apply to the record"""
    if edge == "A":  # pass A: tiles of the stream
        return np.arange(len(p)) // ps.TILE
    if edge == "seg":  # the first LSD pass: plain tiles of the segment, in stream order
        return pos_within(_seg(C, p)) // ps.TILE
    if edge == "group":  # the last LSD pass in a hot segment: tiles of the group
        cnt = np.bincount(_seg(C, p), minlength=C["nseg"])
        return np.where(cnt[_seg(C, p)] >= ps.GRP_COLD_MAX, pos_within(_grp(C, p)) // ps.TILE, -1)
    run = p >> C["xb"]  # k_prefix_split: tiles of a run longer than 2048 records
    assert edge == "split"
    _, inv, lens = np.unique(run, return_inverse=True, return_counts=True)
    return np.where(lens[inv] > ps.SPLIT_ONE_TILE[-1], pos_within(run) // ps.SPLIT_TILE, -1)


@pytest.mark.parametrize("k,pb,name", ps.CASES)
def test_some_vec_bucket_shows_the_order_across_every_edge_of_the_shape(k, pb, name):
    s, C, p = _shape(k, pb, name), ps.props(k, pb), _prefixes(k, pb, name)
    m = bs.shape(ps.model, k, pb, name)
    assert ("A" in s.edges) == (len(p) > ps.TILE) and ("group" in s.edges) == name.startswith("hot") and ("split" in s.edges) == (name == "runs")
    assert ("seg" in s.edges) == (C["npass"] > 0 and name in ("segments", "last_segment", "hot_cold", "hot_last", "runs"))
    assert all(kind == "vec" for kind, _ in m.buckets.values())
    if not s.edges:
        return
    seen, firsts = set(), []
    for i, w in enumerate(s.words):
        if w not in seen:
            seen.add(w)
            firsts.append(i)
    firsts = np.array(firsts)
    for edge in s.edges:
        t = _edge_tiles(C, p, edge)[firsts]
        fi, fp, t = firsts[t >= 0], p[firsts][t >= 0], t[t >= 0]
        order = np.argsort(fp, kind="stable")
        fi, fp, t = fi[order], fp[order], t[order]
        starts = np.flatnonzero(np.r_[True, fp[1:] != fp[:-1]])
        lo, hi = np.minimum.reduceat(t, starts), np.maximum.reduceat(t, starts)
        split = np.flatnonzero(lo < hi)
        assert len(split), (name, edge, "no Vec bucket has first occurrences in different tiles")
        a = starts[split[0]]
        b = starts[split[0] + 1] if split[0] + 1 < len(starts) else len(fp)
        i, j = int(fi[a:b][np.argmin(t[a:b])]), int(fi[a:b][np.argmax(t[a:b])])
        prefix = int(fp[a])
        assert m.buckets[prefix][0] == "vec" and s.words[i] >> s.sb == s.words[j] >> s.sb == prefix and s.words[i] != s.words[j]
        mine = [(x, w) for x, w in enumerate(s.words) if w >> s.sb == prefix]
        swapped = [s.words[j] if x == i else s.words[i] if x == j else w for x, w in mine]
        was = bs.serialize(bs.insert_batch(bs.model_of({}, k, pb), [w for _, w in mine]))
        now = bs.serialize(bs.insert_batch(bs.model_of({}, k, pb), swapped))
        assert was != now and len(was) == len(now), (name, edge)  # the bucket's bytes are the index's bytes at its place
        assert m.buckets[prefix][1] == bs.insert_batch(bs.model_of({}, k, pb), [w for _, w in mine]).buckets[prefix][1]


@pytest.mark.parametrize("k,pb,name", ps.CASES)
def test_model_equals_the_oracle_on_every_shape(k, pb, name):
    s = _shape(k, pb, name)
    m = bs.shape(ps.model, k, pb, name)
    assert all(0 <= w < 1 << (s.sb + pb) for w in s.words) and s.sb == pyref.params(k, pb)["SB"] and not s.resident
    o = Oracle(k, pb)
    o.load(bs.serialize(bs.model_of(s)))
    assert o.count() == 0
    o.insert_words(s.words)
    want = bs.serialize(m)
    assert o.serialize() == want and o.count() == m.count() == sum(n for n, _ in bs.table(m).values())
    if len(s.words) <= 70_000:  # the same words once more: nothing changes
        o.insert_words(s.words)
        assert o.serialize() == want
