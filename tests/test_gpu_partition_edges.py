"""The partition and the bucket directory (pipeline.hpp: partition_and_directory — pass A, the LSD passes with plain and group-cut tiles, the prefix
split; k_dir_gather, k_boundaries_cold, k_boundaries / k_boundaries_seg, k_split_table) on crafted words whose segments, groups and runs of equal
super-prefix sit exactly on every tile edge, on the hot / cold threshold and on every class edge of the split. The batches come from
tests/partition_shapes.py; tests/test_partition_shapes.py proves on the CPU that every named piece is in them, that a Vec bucket's bytes depend on
the order across every edge, and that the model equals the oracle. Every expectation is that closed-form model, never the GPU path; byte identity
has no tolerance.

Route evidence. A context created with profile=True counts the records every partition pass moved: stage_units()["radix_scatter"] must be
N x (1 + npass + (1 if xb else 0)) from the restated plan, which pins partition_shapes.lsd_plan to the C++ one. What this does NOT show: the counter
cannot tell a hot segment from a cold one, nor which class of k_split_classify a run took, nor which boundary kernel built the directory. That those
were exercised rests on the CPU test's proof of the crafted sizes (a segment of 262,143 records beside one of 262,144, runs of 512 | 513 .. 8192 | 8193
records) and on the constants that test reads from the code (RDX_TILE, GRP_COLD_MAX, seg_cold's `<`, the class edges of the split)."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402

import build_shapes as bs  # noqa: E402  (tests/)
import partition_shapes as ps  # noqa: E402  (tests/)

M64 = (1 << 64) - 1


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")


def _device_words(g, words):
    """(lo, hi) as insert_words_device and partition_words_device take them: hi is None, one byte or eight bytes per word (consts()["hi_bytes"])"""
    lo = torch.from_numpy(np.array([w & M64 for w in words], dtype=np.uint64).view(np.int64)).cuda()
    hb = g.consts()["hi_bytes"]
    hi = None
    if hb:
        a = np.array([w >> 64 for w in words], dtype=np.uint64)
        hi = torch.from_numpy(a.astype(np.uint8) if hb == 1 else a.view(np.int64)).cuda()
    return lo, hi


def _table(g):
    p, l, kd = g.bucket_table_np()
    return {int(a): (int(b), int(c)) for a, b, c in zip(p, l, kd)}


def _about(C):
    def about(p):
        d = dict(segment=ps.segment(p, C["pb"]))
        if C["npass"] == 2:
            d["group"] = ps.group(p, C["pb"])
        if C["xb"]:
            d.update(run=ps.run_of(p, C["pb"]), sub=ps.sub_of(p, C["pb"]))
        return d
    return about


def _same(g, m, want, what, about):
    """g holds the model's bytes, count, bucket table and is sound — or a message that names the buckets that differ and where they lie"""
    if g.serialize() != want:
        got = {p: ("trie" if kd else "vec", list(items)) for p, kd, items in g.buckets()}
        want_b = {p: (kind, list(items)) for p, (kind, items) in m.buckets.items()}
        bad = [p for p in sorted(set(got) | set(want_b)) if got.get(p) != want_b.get(p)]
        where = [(p, about(p), "got %s" % (got.get(p, ("absent", []))[0],), len(got.get(p, ("", []))[1]), "want %s" % (want_b.get(p, ("absent", []))[0],),
                  len(want_b.get(p, ("", []))[1])) for p in bad[:6]]
        pytest.fail(f"{what}: bytes differ in {len(bad)} buckets; (prefix, place, got kind, length, wanted kind, length): {where}")
    assert g.count() == m.count(), what
    assert _table(g) == bs.table(m), what
    assert g.validate(strict=False) == 0, what


@pytest.mark.parametrize("k,pb,name", ps.CASES)
def test_partition_and_directory_at_every_tile_and_run_edge(k, pb, name):
    """One crafted batch into an empty index, then the same batch into the index it left (the second partition feeds the merge with a non-empty
    index; nothing changes). Shapes, per configuration (tests/partition_shapes.py): n1 | n4095 | n4096 | n4097 records; segments of 0, 1, 4095 | 4096 |
    4097, 8192 | 8193 records with the first and the last among them and a ragged last tile of all-ones digits; every record in the last segment;
    buckets at prefix 0, 1, 63 | 64 | 65, 2^PB - 1, across a segment and a group edge, a segment (or a group and a column of the last pass) populated
    whole; (31, 16): all 65,536 prefixes; (31, 17), (21, 24), (31, 26): a cold segment of 262,143 records beside a hot one of 262,144 and a hot segment
    255 of 262,145, with groups of 0, 1, 4095 | 4096 | 4097 records; PB > 24: runs of 1, 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097, 8192 | 8193
    records under every fill of their sub-prefixes. See the module's docstring for what the pass counter shows and what it cannot."""
    _need_gpu()
    C = ps.props(k, pb)
    s = bs.shape(ps.craft, k, pb, name)
    m = bs.shape(ps.model, k, pb, name)
    want = bs.shape(model_bytes, k, pb, name)
    what = f"K={k} PB={pb} {name} (N={len(s.words)})"
    g = cbl_amd.CBL(k, pb, profile=True)
    try:
        assert g.consts()["suffix_bits"] == s.sb and g.consts()["hi_bytes"] == C["hi_bytes"], what
        lo, hi = _device_words(g, s.words)
        n = len(s.words)
        g.stage_times_reset()
        g.insert_words_device(lo, hi, n)
        units = g.stage_units()["radix_scatter"]
        _same(g, m, want, what, _about(C))
        assert units == n * (1 + C["npass"] + (1 if C["xb"] else 0)), (what, units)
        g.insert_words_device(lo, hi, n)
        _same(g, m, want, what + ", the same batch again", _about(C))
    finally:
        g.close()


def model_bytes(k, pb, name):
    return bs.serialize(bs.shape(ps.model, k, pb, name))


# ---- the destination partition of the multi-GPU exchange on crafted words --------------------------------------------------------------------------
DEST_CONFIGS = ((31, 24), (21, 24), (59, 28))
DEST_SIZES = (1, 4095, 4096, 4097, 65537)


def _dest_bounds(pb, b):
    """(nd, bounds): a bound of 0 (every record bound for the last destination) and of 2^PB - 1, a bound on a populated prefix b whose predecessor is
    populated too (`bounds[i] <= prefix`), runs of equal bounds (empty destinations)"""
    ones = (1 << pb) - 1
    return [(1, []), (2, [0]), (2, [ones]), (2, [b]), (2, [b + 1]), (16, [0] * 15), (16, [ones] * 15),
            (16, [0, 0, 1, b - 1, b, b, b, b + 1, b + 2, ones // 2, ones // 2, ones - 1, ones, ones, ones]),
            (16, [1, 2, 3, 4, 5, 6, 7, b, b + 1, b + 2, b + 3, b + 4, ones - 2, ones - 1, ones])]


@pytest.mark.parametrize("n", DEST_SIZES)
@pytest.mark.parametrize("k,pb", DEST_CONFIGS)
def test_partition_words_device_on_crafted_bounds(k, pb, n):
    """partition_words_device against numpy's stable partition by destination = #{i : bounds[i] <= prefix}, and the returned counts, at N = 1, 4095,
    4096, 4097 and 65537 records, for 1, 2 and 16 destinations. The words populate prefix 0, 1, b - 1, b, b + 1, 2^PB - 2 and 2^PB - 1 and a hundred
    random ones; every record keeps a suffix of its own, so the order inside a destination shows."""
    _need_gpu()
    C = ps.props(k, pb)
    rng = random.Random("dest %d/%d/%d" % (k, pb, n))
    ones = (1 << pb) - 1
    b = rng.randrange(1 << (pb - 2), (1 << (pb - 1)) - 8)
    populated = [b, b - 1, b + 1, 0, 1, ones - 1, ones] + rng.sample(range(1 << pb), 100)
    prefix = [populated[i] if i < len(populated) else rng.choice(populated) for i in range(n)]
    words = [(p << C["sb"]) | rng.getrandbits(C["sb"]) for p in prefix]
    pa = np.array(prefix, dtype=np.uint64)
    assert n < 7 or {0, b - 1, b, ones} <= set(prefix)
    g = cbl_amd.CBL(k, pb)
    try:
        lo, hi = _device_words(g, words)
        lo_np = lo.cpu().numpy()
        hi_np = None if hi is None else hi.cpu().numpy()
        for nd, bounds in _dest_bounds(pb, b):
            assert len(bounds) == nd - 1 and bounds == sorted(bounds)
            dest = np.searchsorted(np.array(bounds, dtype=np.uint64), pa, side="right")
            order = np.argsort(dest, kind="stable")
            out_lo = torch.zeros_like(lo)
            out_hi = None if hi is None else torch.zeros_like(hi)
            counts = g.partition_words_device(lo, hi, n, bounds, nd, out_lo, out_hi)
            what = (k, pb, n, nd, bounds)
            assert counts == np.bincount(dest, minlength=nd).tolist(), what
            assert np.array_equal(out_lo.cpu().numpy(), lo_np[order]), what
            assert hi is None or np.array_equal(out_hi.cpu().numpy(), hi_np[order]), what
            if bounds and bounds[-1] == 0:  # every record bound for the last destination
                assert counts[-1] == n, what
    finally:
        g.close()
