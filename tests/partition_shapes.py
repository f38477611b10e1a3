"""Crafted batches for the partition and the bucket directory (pipeline.hpp: partition_and_directory; kernels_radix.hpp): words whose
segments, groups and runs of equal super-prefix sit exactly on either side of every tile edge, of the hot / cold threshold of the group-cut
tiles and of every class of the prefix split. Pure CPU: `random` and `oracle.pyref`; a helper, not a test file. tests/test_partition_shapes.py
proves from the words themselves that every named piece is there and that the model equals the C++ oracle; tests/test_gpu_partition_edges.py
compares the GPU's bytes, bucket table and partition accounting with it.

The model is build_shapes.insert_batch (WordSet::insert_batch in closed form) on an empty index. What this file restates from pipeline.hpp:
  * lsd_plan: pass A sorts the top nA = min(8, PB) prefix bits into 2^nA segments; PB <= 24: npass = ceil((PB - nA) / 8) LSD passes inside the
    segments, pass i over prefix bits [8i, 8i + min(8, RB - 8i)); PB > 24: two passes of 8 bits over prefix bits [xb, xb + 16), xb = PB - 24, and
    k_prefix_split for the low xb bits of every run of equal 24-bit super-prefix;
  * with two LSD passes the last one runs on tiles cut at the GROUPS = segment x (the 8 bits the first pass sorted) in every segment of at least
    GRP_COLD_MAX = 64 tiles (hot); a cold segment keeps plain tiles;
  * k_split_classify: runs of up to 512 / 1024 / 2048 records are one tile of a small workgroup, longer ones go in tiles of 4096 and are
    counted first.

Stability witness. The index bytes show the order the partition left only through Vec buckets (a Vec stores first occurrences in stream order), so
every bucket here stays a Vec: a bucket of n records holds v = min(n, 1000) distinct suffixes, the j-th of them first appears at record
j * n // v of the bucket, the last one in its last record, repeats of earlier values between (bucket_stream). The buckets (split plans: the runs) of
a batch are dealt into the stream in proportion to their lengths (merge), so every bucket stretches over the whole batch and over every tile of
whatever holds it. Words are prefix << SUFFIX_BITS | suffix, as in build_shapes.py.
"""
from __future__ import annotations

import random
from collections import namedtuple

from oracle import pyref

import build_shapes as bs

TILE = 4096                 # kernels_radix.hpp: RDX_TILE = RDX_THREADS * RDX_ITEMS
GRP_COLD_MAX = 64 * TILE     # kernels_radix.hpp: GRP_COLD_MAX; seg_cold is `<`: 262,143 records cold, 262,144 hot
SPLIT_ITEMS = 8              # kernels_radix.hpp: SPLIT_ITEMS; k_split_classify: <= 64 / 128 / 256 * SPLIT_ITEMS records in one tile, else tiles of 512 * SPLIT_ITEMS
SPLIT_ONE_TILE = (64 * SPLIT_ITEMS, 128 * SPLIT_ITEMS, 256 * SPLIT_ITEMS)
SPLIT_TILE = 512 * SPLIT_ITEMS
VEC_DISTINCT = 1000          # distinct suffixes of a long bucket: below VEC_THRESHOLD = 1024, it stays a Vec

ROUTES = {
    "a_only_hi_is_digit": ((31, 4),),
    "a_only": ((31, 8), (21, 6), (59, 8)),
    "one_pass": ((31, 9), (31, 16)),
    "two_pass": ((31, 17), (31, 24), (21, 24), (59, 24)),
    "split": ((27, 25), (31, 26), (31, 28), (59, 28)),
}
CONFIGS = [(route, k, pb) for route, kp in ROUTES.items() for k, pb in kp]
HOT_CONFIGS = ((31, 17), (21, 24), (31, 26))
ALL_PREFIXES_CONFIG = (31, 16)


# ---- the plan and the places of a prefix, restated ---------------------------------------------------------------------------------------------
def lsd_plan(pb):
    """pipeline.hpp: lsd_plan with split_ok. passes: (first prefix bit, width) of every LSD pass in the order they run."""
    if pb > 24:
        xb = pb - 24
        return dict(nA=8, xb=xb, npass=2, passes=[(xb, 8), (xb + 8, 8)])
    nA = min(8, pb)
    rb = pb - nA
    npass = (rb + 7) // 8
    return dict(nA=nA, xb=0, npass=npass, passes=[(8 * i, min(8, rb - 8 * i)) for i in range(npass)])


def hi_bytes(k, pb):
    """ctx.hpp: hi_elem_size. No hi part up to 64 bits; one byte while k-mer and suffix fit 64 bits; else 8 bytes."""
    P = pyref.params(k, pb)
    return 0 if P["WB"] <= 64 else 1 if P["KB"] <= 64 and P["SB"] <= 64 else 8


def props(k, pb):
    P = pyref.params(k, pb)
    plan = lsd_plan(pb)
    return dict(k=k, pb=pb, sb=P["SB"], wb=P["WB"], hi_bytes=hi_bytes(k, pb), nseg=1 << plan["nA"], pps=1 << (pb - plan["nA"]), nb=1 << plan["xb"], **plan)


def segment(p, pb):
    """pass A's digit: the top nA prefix bits"""
    return p >> (pb - lsd_plan(pb)["nA"])


def digit(p, pb, i):
    sh, w = lsd_plan(pb)["passes"][i]
    return (p >> sh) & ((1 << w) - 1)


def group(p, pb):
    """two LSD passes: segment x the bits the first of them sorts. The last pass's tiles are cut at these in a hot segment."""
    plan = lsd_plan(pb)
    assert plan["npass"] == 2
    return (segment(p, pb) << plan["passes"][0][1]) | digit(p, pb, 0)


def run_of(p, pb):
    """PB > 24: the 24-bit super-prefix, one run of k_prefix_split"""
    return p >> lsd_plan(pb)["xb"]


def sub_of(p, pb):
    return p & ((1 << lsd_plan(pb)["xb"]) - 1)


def prefix_of(C, seg, d=0, low=0, sub=0):
    """two-pass and split plans: the prefix of (segment, last pass's digit, first pass's digit, sub-prefix)"""
    (sh0, w0), (sh1, w1) = C["passes"]
    assert seg < C["nseg"] and d < 1 << w1 and low < 1 << w0 and sub < C["nb"]
    return (seg << (C["pb"] - C["nA"])) | (d << sh1) | (low << sh0) | sub


def split_tile(n):
    """records per tile of the workgroup k_split_classify gives a run of n records"""
    for t in SPLIT_ONE_TILE:
        if n <= t:
            return t
    return SPLIT_TILE


# ---- streams -----------------------------------------------------------------------------------------------------------------------------------
def _values(rng, sb, v):
    seen = {}
    while len(seen) < v:
        seen.setdefault(rng.getrandbits(sb), None)
    return list(seen)


def bucket_stream(rng, sb, n, v=None):
    """n suffixes over v distinct values: value j first at record j * n // v, the last value first at record n - 1, earlier values repeated between"""
    v = min(n, VEC_DISTINCT) if v is None else v
    assert 1 <= v <= n and v <= VEC_DISTINCT
    vals = _values(rng, sb, v)
    if v == n:
        return vals
    first = {j * n // v: j for j in range(v - 1)}
    first[n - 1] = v - 1
    out, seen = [], 0
    for i in range(n):
        j = first.get(i)
        if j is None:
            out.append(vals[rng.randrange(seen)])
        else:
            out.append(vals[j])
            seen = j + 1
    return out


def _bucket(rng, sb, p, n):
    return [(p << sb) | s for s in bucket_stream(rng, sb, n)]


def merge(strands):
    """Deal the strands (lists of words, or (words, tail)) into one stream in proportion to their lengths, each in its own order: record i of a
    strand of n sits at (i + 0.5) / n of the batch. The last `tail` records of a strand come behind everything else."""
    keyed, tails = [], []
    for b, s in enumerate(strands):
        ws, tail = s if isinstance(s, tuple) else (s, 0)
        n = len(ws) - tail
        assert n >= 0
        keyed += [((i + 0.5) / n, b, w) for i, w in enumerate(ws[:n])]
        tails += ws[n:]
    keyed.sort()  # (position, strand) is unique: the words are never compared
    return [w for _, _, w in keyed] + tails


def _spread(n, m):
    return [n // m + (1 if i < n % m else 0) for i in range(m)]


Shape = namedtuple("Shape", "name k pb sb resident words edges")  # one batch into an empty index; edges: the tile edges its witness buckets straddle


def _shape(C, name, words, edges=()):
    edges = tuple(edges) + (("A",) if len(words) > TILE and "A" not in edges else ())
    return Shape(name, C["k"], C["pb"], C["sb"], {}, words, edges)


def _rng(C, name):
    return random.Random("partition %d/%d/%s" % (C["k"], C["pb"], name))


def _seg_buckets(C, seg, n):
    """(prefix, records) of a segment of n records: over its first prefix, its last and up to 14 evenly spaced between them, as far as it has them.
    With 16 prefixes a segment of 8193 records has buckets of 513 at the most: every record a value of its own, none a repeat whose loss no
    byte would show."""
    m = min(C["pps"], SEG_BUCKETS)
    picks = sorted({i * (C["pps"] - 1) // max(m - 1, 1) for i in range(m)})
    m = min(len(picks), n)
    return list(zip([seg * C["pps"] + x for x in picks[:m]], _spread(n, m))) if m else []


# ---- 1. batch and segment geometry ---------------------------------------------------------------------------------------------------------------
BATCH_SIZES = (1, 4095, 4096, 4097)
SEGMENT_SIZES = (4096, 0, 1, 0, 4095, 4097, 8192, 8193)  # segments 0 .. 7; the last segment holds 4097 more
LAST_SEGMENT_N = 8200
SEG_BUCKETS = 16


def craft_batch(k, pb, n):
    """A batch of exactly n records over the first segment, one in the middle and the last; n = 1: the word of prefix 2^PB - 1."""
    C = props(k, pb)
    rng = _rng(C, "n%d" % n)
    last = C["nseg"] - 1
    if n == 1:
        return _shape(C, "n1", _bucket(rng, C["sb"], (1 << pb) - 1, 1))
    sizes = _spread(n, 3)
    strands = [_bucket(rng, C["sb"], p, c) for seg, sz in zip((0, C["nseg"] // 2, last), sizes) for p, c in _seg_buckets(C, seg, sz)]
    return _shape(C, "n%d" % n, merge(strands))


def _with_ragged_tail(C, rng, buckets, total):
    """strands of (prefix, records); the bucket of prefix 2^PB - 1 keeps its last total % TILE records for the end of the stream"""
    ones = (1 << C["pb"]) - 1
    tail = total % TILE
    assert tail and sum(c for _, c in buckets) == total and dict(buckets)[ones] > tail
    return [(_bucket(rng, C["sb"], p, c), tail if p == ones else 0) for p, c in buckets]


def craft_segments(k, pb):
    """Segments 0 .. 7 of exactly 4096, 0, 1, 0, 4095, 4097, 8192, 8193 records and the last segment of 4097, whose ragged last tile — in pass A the
    last N % 4096 records of the stream, in an LSD pass the last record of the segment — holds records of prefix 2^PB - 1 (every digit all ones)."""
    C = props(k, pb)
    rng = _rng(C, "segments")
    last = C["nseg"] - 1
    buckets = [b for seg, n in enumerate(SEGMENT_SIZES) for b in _seg_buckets(C, seg, n)] + _seg_buckets(C, last, TILE + 1)
    total = sum(SEGMENT_SIZES) + TILE + 1
    return _shape(C, "segments", merge(_with_ragged_tail(C, rng, buckets, total)), ("seg",) if C["npass"] else ())


def craft_last_segment(k, pb):
    """every record in the last segment; the ragged last tile as in craft_segments"""
    C = props(k, pb)
    rng = _rng(C, "last_segment")
    buckets = _seg_buckets(C, C["nseg"] - 1, LAST_SEGMENT_N)
    return _shape(C, "last_segment", merge(_with_ragged_tail(C, rng, buckets, LAST_SEGMENT_N)), ("seg",) if C["npass"] else ())


# ---- 2. directory positions ----------------------------------------------------------------------------------------------------------------------
FULL_SEGMENT, FULL_LOW, EDGE_SEGMENT, EDGE_LOW = 9, 37, 5, 7
FULL_SEGMENT_MAX = 512  # prefixes per segment up to which one segment is populated whole; beyond, one group and one column of the last pass


def craft_directory(k, pb):
    """Buckets of three records at prefix 0, 1, 63, 64, 65 and 2^PB - 1 (those the configuration has); the last prefix of a segment and the first of
    the next; two-pass and split plans: the last prefix of a group (last pass's digit and sub-prefix all ones) and the first of the next group, inside
    a segment and across a segment edge; segment 9 with every prefix populated by one record — with more than 512 prefixes per segment one group
    of it (all values of the last pass's digit over one value of the first's) and one column of the last pass's table (one value of its digit
    over all 256 groups), the sub-prefix rotating."""
    C = props(k, pb)
    rng = _rng(C, "directory")
    want = {}
    for p in (0, 1, 63, 64, 65, (1 << pb) - 1):
        if p < 1 << pb:
            want[p] = 3
    mid = (C["nseg"] // 2) * C["pps"]
    want.update({mid - 1: 2, mid: 2})
    if C["npass"] == 2:
        dmax = (1 << C["passes"][1][1]) - 1
        for seg, low in ((EDGE_SEGMENT, EDGE_LOW), (EDGE_SEGMENT, 255)):
            want[prefix_of(C, seg, dmax, low, C["nb"] - 1)] = 2
            want[prefix_of(C, seg + (low == 255), 0, (low + 1) & 255, 0)] = 2
    if C["pps"] <= FULL_SEGMENT_MAX:
        full = [FULL_SEGMENT * C["pps"] + i for i in range(C["pps"])]
    else:
        nd = 1 << C["passes"][1][1]
        full = [prefix_of(C, FULL_SEGMENT, d, FULL_LOW, (d + FULL_LOW) % C["nb"]) for d in range(nd)]
        full += [prefix_of(C, FULL_SEGMENT, nd - 55, low, (nd - 55 + low) % C["nb"]) for low in range(256)]
    for p in full:
        want[p] = 1
    return _shape(C, "directory", merge([_bucket(rng, C["sb"], p, n) for p, n in sorted(want.items())]))


ALL_PREFIXES_WITNESS = (12345, 0xFFFF)


def craft_all_prefixes(k, pb):
    """Every prefix populated, in shuffled order: by one record, but for two buckets of 40 records over 20 values that carry the order."""
    C = props(k, pb)
    rng = _rng(C, "all_prefixes")
    once = [p for p in range(1 << pb) if p not in ALL_PREFIXES_WITNESS]
    rng.shuffle(once)
    strands = [[(p << C["sb"]) | rng.getrandbits(C["sb"]) for p in once]]
    strands += [[(p << C["sb"]) | s for s in bucket_stream(rng, C["sb"], 40, 20)] for p in ALL_PREFIXES_WITNESS]
    return _shape(C, "all_prefixes", merge(strands))


# ---- 3. hot and cold segments --------------------------------------------------------------------------------------------------------------------
COLD_SEGMENT, HOT_SEGMENT = 100, 101
# first pass's digit -> records of the group; the other groups share what is left of the segment
HOT_GROUPS = {0: 0, 1: 1, 2: 4095, 3: 4096, 4: 4097, 5: 0}                    # the first group empty; an empty group in front of a populated one
HOT_LAST_GROUPS = {0: 4097, 1: 1, 2: 0, 3: 4095, 4: 4096, 5: 0, 255: 4097}    # the first and the last group populated


def _group_sizes(total, named):
    rest = [g for g in range(256) if g not in named]
    sizes = dict(named)
    sizes.update(zip(rest, _spread(total - sum(named.values()), len(rest))))
    return sizes


def _group_buckets(C, seg, low, n):
    """(prefix, records) of a group of n records: spread evenly over min(n, all) of the group's prefixes, themselves evenly spaced"""
    (_, _), (_, w1) = C["passes"]
    P = (1 << w1) * C["nb"]
    m = min(n, P)
    return [(prefix_of(C, seg, (i * P // m) // C["nb"], low, (i * P // m) % C["nb"]), c) for i, c in enumerate(_spread(n, m))] if m else []


def _segment_of_groups(C, rng, seg, sizes):
    return [_bucket(rng, C["sb"], p, c) for low, n in sorted(sizes.items()) for p, c in _group_buckets(C, seg, low, n)]


def craft_hot_cold(k, pb):
    """Segment 100 of 262,143 records (cold: plain tiles, k_boundaries_cold) beside segment 101 of 262,144 (hot: tiles cut at its groups), whose groups
    0 .. 5 hold exactly 0, 1, 4095, 4096, 4097 and 0 records."""
    C = props(k, pb)
    rng = _rng(C, "hot_cold")
    strands = _segment_of_groups(C, rng, COLD_SEGMENT, _group_sizes(GRP_COLD_MAX - 1, {}))
    strands += _segment_of_groups(C, rng, HOT_SEGMENT, _group_sizes(GRP_COLD_MAX, HOT_GROUPS))
    return _shape(C, "hot_cold", merge(strands), ("seg", "group"))


def craft_hot_last(k, pb):
    """Segment 255 of 262,145 records and nothing else: the last group's end is the batch's (grp_tiled_size's n_total arm). Groups 0 .. 5 hold 4097, 1,
    0, 4095, 4096 and 0 records, group 255 holds 4097."""
    C = props(k, pb)
    rng = _rng(C, "hot_last")
    strands = _segment_of_groups(C, rng, 255, _group_sizes(GRP_COLD_MAX + 1, HOT_LAST_GROUPS))
    return _shape(C, "hot_last", merge(strands), ("seg", "group"))


# ---- 4. split runs -------------------------------------------------------------------------------------------------------------------------------
RUN_LENGTHS = (1, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 4097, 8192, 8193)  # the multi-tile lengths twice: five fills need five such runs
RUN_FILLS = ("first", "last", "interleaved", "blocks_desc", "all_but_one")
SUPER_48 = 0x5A5A5B  # xb = 4: (super-prefix << 4) & 63 == 48, the run's 16 bits end at the top of a bitvector word; its successor's begin the next word


def run_subs(n, nb, fill):
    """the sub-prefix of every record of a run, in stream order"""
    if fill == "first":
        return [0] * n
    if fill == "last":
        return [nb - 1] * n
    if fill == "interleaved":
        return [i % nb for i in range(n)]
    if fill == "blocks_desc":
        return [d for d, c in zip(range(nb - 1, -1, -1), _spread(n, nb)) for _ in range(c)]
    present = [d for d in range(nb) if d != nb // 2]
    return [present[i % len(present)] for i in range(n)]


def run_fills(xb):
    """fill of every run of RUN_LENGTHS: the run of one record holds the last sub-prefix; the others rotate, one-tile and multi-tile runs apart, from
    a start that depends on the configuration"""
    one = [i for i, n in enumerate(RUN_LENGTHS) if 1 < n <= SPLIT_TILE]
    many = [i for i, n in enumerate(RUN_LENGTHS) if n > SPLIT_TILE]
    fills = {0: "last"}
    for lst in (one, many):
        for j, i in enumerate(lst):
            fills[i] = RUN_FILLS[(j + xb) % len(RUN_FILLS)]
    return [fills[i] for i in range(len(RUN_LENGTHS))]


def craft_runs(k, pb):
    """Runs of equal super-prefix of exactly 1, 512 | 513, 1024 | 1025, 2048 | 2049, 4096 | 4097 and 8192 | 8193 records (4097 and 8193: a last tile of
    one record) at super-prefix 0, 2^24 - 1, 0x5A5A5B and its successor and at random ones; fills by run_fills."""
    C = props(k, pb)
    rng = _rng(C, "runs")
    fills = run_fills(C["xb"])
    idx = list(range(len(RUN_LENGTHS)))
    a = next(i for i in idx if RUN_LENGTHS[i] > SPLIT_TILE and fills[i] == "interleaved")  # holds the last sub-prefix: bit 63 of its word
    b = next(i for i in idx if i != a and fills[i] in ("first", "interleaved", "blocks_desc") and RUN_LENGTHS[i] > 1)  # holds the first: bit 0 of the next
    rest = [i for i in idx if i not in (a, b)]
    supers = {a: SUPER_48, b: SUPER_48 + 1, rest[0]: 0, rest[-1]: (1 << 24) - 1}
    free = rng.sample(range(1 << 20, 1 << 23), len(rest))
    for i, sp in zip(rest[1:-1], free):
        supers[i] = sp
    strands = []
    for i in idx:
        n, sp = RUN_LENGTHS[i], supers[i]
        subs = run_subs(n, C["nb"], fills[i])
        streams = {d: iter(bucket_stream(rng, C["sb"], subs.count(d))) for d in set(subs)}
        strands.append([((sp << C["xb"] | d) << C["sb"]) | next(streams[d]) for d in subs])
    return _shape(C, "runs", merge(strands), ("seg", "split"))


# ---- the shapes of a configuration ---------------------------------------------------------------------------------------------------------------
def shape_names(k, pb):
    names = ["n%d" % n for n in BATCH_SIZES] + ["segments", "last_segment", "directory"]
    if (k, pb) == ALL_PREFIXES_CONFIG:
        names.append("all_prefixes")
    if (k, pb) in HOT_CONFIGS:
        names += ["hot_cold", "hot_last"]
    if pb > 24:
        names.append("runs")
    return names


def craft(k, pb, name):
    if name[0] == "n" and name[1:].isdigit():
        return craft_batch(k, pb, int(name[1:]))
    return {"segments": craft_segments, "last_segment": craft_last_segment, "directory": craft_directory, "all_prefixes": craft_all_prefixes,
            "hot_cold": craft_hot_cold, "hot_last": craft_hot_last, "runs": craft_runs}[name](k, pb)


CASES = [(k, pb, name) for _, k, pb in CONFIGS for name in shape_names(k, pb)]


def model(k, pb, name):
    """the index the batch leaves behind (through build_shapes.shape: once per process, left unchanged by its users)"""
    s = bs.shape(craft, k, pb, name)
    return bs.insert_batch(bs.model_of(s), s.words)
