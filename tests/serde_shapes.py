"""Crafted indexes for the device serializer (cbl_amd/csrc/kernels_serde.hpp, driven by serialize_device in host_index.hpp): bucket tables whose
lengths, values, byte sizes and positions in the blob sit on either side of every edge of its size classes, its two kernel shapes per class, its
LDS staging, its split Tries and its chunked hand-over. Pure CPU: `random`, numpy and `oracle.pyref`; a helper, not a test file.
tests/test_serde_shapes.py shows on the CPU what every shape delivers and that the expected bytes (build_shapes.serialize of the model) equal the
C++ oracle's; tests/test_gpu_serde_edges.py installs the tables with install_buckets_device and compares the GPU's bytes with them.

A table is {prefix: (kind, [suffix, ...])}, kind "vec" (stored order) or "trie" (ascending). Every table is a valid index: distinct suffixes below
2^SB, prefixes below 2^PB. A Vec of more than 1024 words is what `|=` leaves; a Trie of 1024 words or fewer is what comes out of a file.

Where an entry lands. The blob's base is a pool block, i.e. a hipMalloc'd pointer (ctx.hpp: Pool::alloc rounds sizes to 256 bytes and hands out
hipMalloc's pointers unchanged, which are aligned to at least 256 bytes), and the body starts hs.pos = 1 + vlen(nb) bytes in (host_index.hpp:
serialize_device). So the `mis` of k_serde_bucket, the entry's address & 15, is (header_len + offset) & 15 relative to the blob start: layout()
below gives it exactly.

Widths. The four of build_shapes.CONFIGS (BYTES 6, 8, 11, 15), K = 15 / PB = 6 (BYTES 4) and K = 9 / PB = 15 (SB = 8, BYTES = 1: the root is the leaf
level). The issue names K = 9 / PB = 16 (SB = 7) and K = 6 / PB = 8 for BYTES = 1; K = 6 is refused by make_consts (K must be odd), and SB = 7 holds 128
suffixes only, so the neighbouring PB = 15 is taken: SB = 8 lets the leaf root have 250 | 251 | 255 | 256 children. "pb24" (K = 31, PB = 24, BYTES 6) exists
for the prefix varints alone: no other width has PB > 16.

What a width cannot hold, and where it is held instead. The top byte of a suffix has SB - 8 (BYTES - 1) bits: 2 in packed, 8 in narrow64, 1 in wide,
5 in radix, 5 in b4, 8 in b1. A root (or a split plan) with 250 | 251 | 255 | 256 present top bytes therefore exists in narrow64 and b1 only; the split
family runs in packed (4 sub-ranges), narrow64 (256) and radix (32, two-word suffixes). A Vec entry reaches the staging threshold only when
1 + BYTES >= 14 bytes per element, i.e. in radix (BYTES 15). A packed Trie of 2^21 words has 4 sub-ranges of 2^19 words, so it is classified as a
split Trie, found `bad` by the plan and emitted by the host like its neighbour of 2^21 + 1 words, which is classified for the host at once.
"""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np

from oracle import pyref

import build_shapes as bs
import setops_model as sm

# ---- the serializer's geometry, restated (tests/test_serde_shapes.py reads each out of the sources) ---------------------------------------------
SER_TINY = 32                      # kernels_serde.hpp:69   Vec buckets up to this length are written by one thread each
SER_CAP64 = 64 * 16                # kernels_serde.hpp:68
SER_CAP256 = 256 * 16              # kernels_serde.hpp:68
SER_CAP1024 = 1024 * 8             # kernels_serde.hpp:68
SER_SPLIT_MAX = 1 << 21            # kernels_serde.hpp:67
SER_CHUNKS = 32                    # kernels_serde.hpp:62
STAGE_PER_ELEMENT = 13             # kernels_serde.hpp:126  STAGE = CAP * 13 + 64
STAGE_SLACK = 64                   # kernels_serde.hpp:126
SIZING = {"c64": (64, 16), "c256": (256, 16), "c1024": (1024, 8)}      # host_index.hpp:215,219,221 (sub-ranges: 188,192,195)
EMITTING = {"c64": (256, 4), "c256": (1024, 4), "c1024": (1024, 8)}    # host_index.hpp:214,218,221 (sub-ranges: 187,191,195)
CHUNKED_MIN_BUCKETS = 4 * SER_CHUNKS  # host_index.hpp:347  chunked = on_chunk && nb >= 4 * SER_CHUNKS && blob.n >= chunk_min
WG_CLASSES = ("c64", "c256", "c1024")
CLASSES = ("tiny",) + WG_CLASSES + ("split", "host")


def vlen(v):
    """kernels_serde.hpp:24"""
    return 1 if v <= 250 else 3 if v < 1 << 16 else 5 if v < 1 << 32 else 9


def classify(kind, n, by):
    """k_serde_tiny, kernels_serde.hpp:81 and :105"""
    if kind == "vec" and n <= SER_TINY:
        return "tiny"                                               # :81
    if n <= SER_CAP64:
        return "c64"                                                # :105
    if n <= SER_CAP256:
        return "c256"
    if n <= SER_CAP1024:
        return "c1024"
    return "split" if kind == "trie" and n <= SER_SPLIT_MAX and by > 1 else "host"


def sub_class(c):
    """k_serde_split_plan, kernels_serde.hpp:335 (a sub-range of more than SER_CAP1024 words makes the bucket bad, :329)"""
    return None if c == 0 else "c64" if c <= SER_CAP64 else "c256" if c <= SER_CAP256 else "c1024" if c <= SER_CAP1024 else "over"


def split_plan(suffixes, by):
    """the 256 sub-range lengths of a bucket by top byte, their classes, and whether the plan hands the bucket to the host"""
    counts = [0] * 256
    sh = 8 * (by - 1)
    for s in suffixes:
        counts[s >> sh] += 1
    classes = [sub_class(c) for c in counts]
    return counts, classes, "over" in classes


def stage_bytes(cls):
    """STAGE of the emitting instance of a workgroup class"""
    th, it = EMITTING[cls]
    return th * it * STAGE_PER_ELEMENT + STAGE_SLACK


def chunk_of(r, nb):
    """k_serde_tiny, kernels_serde.hpp:106, with per from host_index.hpp:199"""
    per = max(1, -(-nb // SER_CHUNKS))
    return r // per, per


# ---- widths ----------------------------------------------------------------------------------------------------------------------------------
WIDTHS = dict(bs.CONFIGS, b4=(15, 6), b1=(9, 15))
ALL_WIDTHS = ("packed", "narrow64", "wide", "radix", "b4", "b1")
PB24 = (31, 24)
WIDTHS["pb24"] = PB24

Shape = namedtuple("Shape", "name width k pb sb by buckets marks")  # marks: {prefix: label of what the bucket is crafted for}
Entry = namedtuple("Entry", "rank prefix kind n cls offset size mis staged")


def geom(width):
    k, pb = WIDTHS[width]
    P = pyref.params(k, pb)
    return k, pb, P["SB"], P["BYTES"]


def top_bits(sb, by):
    return sb - 8 * (by - 1)


def _shape(name, width, buckets, marks):
    k, pb, sb, by = geom(width)
    assert all(0 <= p < 1 << pb for p in buckets) and all(items for _, items in buckets.values())
    return Shape(name, width, k, pb, sb, by, buckets, marks)


# ---- expected bytes, arrays, layout ------------------------------------------------------------------------------------------------------------
def model(shape):
    return sm.from_buckets(shape.k, shape.pb, False, shape.buckets)


def entry_bytes(shape, prefix, kind, items):
    """one entry of the body: the model's bytes of an index that holds this bucket alone, without its two header bytes"""
    return bs.serialize(sm.from_buckets(shape.k, shape.pb, False, {prefix: (kind, items)}))[2:]


def header(nb):
    return b"\x00" + pyref.PyCBL._varint(nb)


_entries = {}


def entries(shape):
    """the body's entries, ascending prefixes (computed once per shape)"""
    if shape.name not in _entries:
        _entries[shape.name] = [entry_bytes(shape, p, *shape.buckets[p]) for p in sorted(shape.buckets)]
    return _entries[shape.name]


def expected(shape):
    return header(len(shape.buckets)) + b"".join(entries(shape))


def layout(shape, sizes=None):
    """for every entry: rank, prefix, kind, length, class, offset in the body, size, mis = (header_len + offset) & 15, and whether its emitting
    instance stages it in LDS (kernels_serde.hpp:140: esz + mis <= STAGE); None for the classes that have no staging"""
    if sizes is None:
        sizes = [len(e) for e in entries(shape)]
    h = len(header(len(shape.buckets)))
    out, off = [], 0
    for r, (p, sz) in enumerate(zip(sorted(shape.buckets), sizes)):
        kind, items = shape.buckets[p]
        cls = classify(kind, len(items), shape.by)
        mis = (h + off) & 15
        out.append(Entry(r, p, kind, len(items), cls, off, sz, mis, sz + mis <= stage_bytes(cls) if cls in WG_CLASSES else None))
        off += sz
    return out


def suffix_bytes(items, by):
    """`by` little-endian bytes per suffix"""
    if by <= 8:
        return np.ascontiguousarray(np.array(items, dtype=np.uint64).view(np.uint8).reshape(-1, 8)[:, :by]).reshape(-1)
    return np.frombuffer(b"".join(s.to_bytes(by, "little") for s in items), dtype=np.uint8)


def arrays(shape):
    """the four flat arrays install_buckets_device takes: prefix uint32, count uint32, kind uint8, suffixes as BYTES little-endian bytes each,
    bucket-major, in stored order"""
    ps = sorted(shape.buckets)
    prefix = np.array(ps, dtype=np.uint32)
    count = np.array([len(shape.buckets[p][1]) for p in ps], dtype=np.uint32)
    kind = np.array([1 if shape.buckets[p][0] == "trie" else 0 for p in ps], dtype=np.uint8)
    parts = [suffix_bytes(shape.buckets[p][1], shape.by) for p in ps]
    suffix = np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint8)
    return prefix, count, kind, suffix


def locate(shape, offset):
    """what a failure message says about the byte at `offset` of the blob"""
    h = len(header(len(shape.buckets)))
    if offset < h:
        return "the header"
    for e in layout(shape):
        if offset - h < e.offset + e.size:
            d = dict(e._asdict(), at=offset - h - e.offset, mark=shape.marks.get(e.prefix), route={True: "staged", False: "direct", None: "-"}[e.staged])
            if e.cls == "split":
                counts, _, bad = split_plan(shape.buckets[e.prefix][1], shape.by)
                d.update(bad=bad, sub_ranges=[c for c in counts if c])
            return d
    return "past the end"


# ---- values ----------------------------------------------------------------------------------------------------------------------------------
def _rand(rng, sb, n, kind):
    v = sm.distinct(rng, n, sb)
    return sorted(v) if kind == "trie" else v


def _lvec(rng, v):
    """a Vec of more than 1024 words as `|=` leaves it: two ascending pieces"""
    cut = len(v) * 2 // 3
    return sorted(v[:cut]) + sorted(v[cut:])


def _store(rng, sb, n, kind):
    v = sm.distinct(rng, n, sb)
    if kind == "trie":
        return sorted(v)
    return _lvec(rng, v) if n > bs.THRESHOLD else v


def _filler(rng, sb):
    """an ordinary neighbour: a tiny Vec or a short Trie"""
    if sb <= 8:
        return ("vec", _rand(rng, sb, 5, "vec")) if rng.random() < 0.5 else ("trie", _rand(rng, sb, 20, "trie"))
    return ("vec", _rand(rng, sb, rng.randrange(1, 9), "vec")) if rng.random() < 0.5 else ("trie", _rand(rng, sb, rng.randrange(33, 80), "trie"))


def dense(rng, sb, n):
    """consecutive integers: 256 children near the leaves, single chains above"""
    if n >= 1 << sb:
        return list(range(1 << sb))
    if sb <= 16:
        base = rng.randrange(0, (1 << sb) - n)
    else:  # from 0x..10F0 on: an early carry out of byte 0, so nodes of 16 and of 256 children both occur; none out of byte 1 (n <= 8192)
        base = rng.getrandbits(sb - 17) << 16 | 0x10F0
    return list(range(base, base + n))


def sparse(rng, sb, by, n):
    """element i differs from every other as high as the width allows: in the top byte up to 2^(top bits) of them, then in the second byte, then in
    the third; below that byte each has a chain of its own"""
    tb = top_bits(sb, by)
    T = 1 << tb
    if by == 1:
        return sorted(rng.sample(range(T), min(n, T)))
    out = []
    low = 8 * max(by - 3, 0)
    for i in range(n):
        top, second, third = i % T, (i // T) % 256, i // (T * 256)
        assert third < 256 and by >= 2 and (third == 0 or by >= 3)
        v = top << (8 * (by - 1)) | second << (8 * (by - 2))
        if by >= 3:
            v |= third << (8 * (by - 3)) | rng.getrandbits(low) if low else third << (8 * (by - 3))
        out.append(v)
    assert len(set(out)) == n
    return sorted(out)


def only_byte(rng, sb, by, j, c):
    """c suffixes that differ in little-endian byte j only"""
    base = rng.getrandbits(sb) & ~(0xFF << (8 * j))
    vals = rng.sample(range(256 if j < by - 1 else 1 << top_bits(sb, by)), c)
    return sorted(base | v << (8 * j) for v in vals)


def fanout_root(rng, sb, by, c):
    """a root of exactly c children, one to three suffixes under each"""
    tops = rng.sample(range(1 << top_bits(sb, by)), c)
    if by == 1:
        return sorted(tops)
    out = set()
    for t in tops:
        for _ in range(rng.randrange(1, 4)):
            out.add(t << (8 * (by - 1)) | rng.getrandbits(8 * (by - 1)))
    return sorted(out)


def fanout_mid(rng, sb, by, c):
    """a root of one child whose node at level 1 has exactly c children, one to three suffixes under each"""
    assert by >= 2
    top = rng.randrange(1 << top_bits(sb, by)) << (8 * (by - 1))
    out = set()
    for s in rng.sample(range(256), c):
        for _ in range(rng.randrange(1, 4) if by > 2 else 1):
            out.add(top | s << (8 * (by - 2)) | (rng.getrandbits(8 * (by - 2)) if by > 2 else 0))
    return sorted(out)


# ---- a. length edges ---------------------------------------------------------------------------------------------------------------------------
# the issue's lengths, and 64 * ITEMS of the <1024, 8> instance where it is in use: 511 | 512 | 513 words into its second wave
LENGTHS = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 4607, 4608, 4609, 8191, 8192, 8193)


def lengths_for(width):
    sb = geom(width)[2]
    return tuple(n for n in LENGTHS if n <= 1 << sb)


def craft_lengths(width, kind):
    """one bucket of `kind` per length, each between two ordinary neighbours"""
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/lengths/%s/%s" % (width, kind))
    ns = lengths_for(width)
    ps = sorted(rng.sample(range(1 << pb), 2 * len(ns) + 1))
    buckets, marks = {}, {}
    for i, p in enumerate(ps):
        if i % 2 == 0:
            buckets[p] = _filler(rng, sb)
        else:
            n = ns[i // 2]
            buckets[p] = (kind, _store(rng, sb, n, kind))
            marks[p] = "length %d" % n
    return _shape("lengths/%s/%s" % (width, kind), width, buckets, marks)


# ---- b. Trie value patterns --------------------------------------------------------------------------------------------------------------------
PATTERN_LENGTHS = {"c64": 700, "c256": 3000, "c1024": 8192}  # 8192: ranks up to 8192 in the u16 s_ns
FANOUTS = (1, 2, 250, 251, 255, 256)


def craft_patterns(width):
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/patterns/%s" % width)
    tb = top_bits(sb, by)
    todo = []  # (label, items)
    for cls, n in PATTERN_LENGTHS.items():
        if n > 1 << sb:
            continue
        todo.append(("dense %s" % cls, dense(rng, sb, n)))
        todo.append(("sparse %s" % cls, sparse(rng, sb, by, n)))
        todo.append(("random %s" % cls, _rand(rng, sb, n, "trie")))
        todo.append(("sentinels %s" % cls, sorted(set(sm.distinct(rng, n - 2, sb - 1)) - {0} | {0, (1 << sb) - 1})))
        top = ((1 << tb) - 1) << (8 * (by - 1))
        if by > 1:
            todo.append(("top bits %s" % cls, sorted(top | v for v in sm.distinct(rng, n, 8 * (by - 1)))))
    if by == 1:
        todo.append(("dense all", list(range(1 << sb))))
        todo.append(("sentinels", sorted(set(rng.sample(range(1, 255), 60)) | {0, 255})))
    for c in FANOUTS:
        if c <= 1 << tb:
            todo.append(("fanout root %d" % c, fanout_root(rng, sb, by, c)))
        if by >= 2:
            todo.append(("fanout mid %d" % c, fanout_mid(rng, sb, by, c)))
    for j in sorted({0, 7, 8, by - 1}):
        if j < by and by > 1:
            c = 256 if j < by - 1 else 1 << tb
            todo.append(("only byte %d" % j, only_byte(rng, sb, by, j, c)))
            if c > 2:
                todo.append(("only byte %d, 2" % j, only_byte(rng, sb, by, j, 2)))
    ps = sorted(rng.sample(range(1 << pb), len(todo)))
    buckets = {p: ("trie", items) for p, (_, items) in zip(ps, todo)}
    marks = {p: label for p, (label, _) in zip(ps, todo)}
    return _shape("patterns/%s" % width, width, buckets, marks)


# ---- c. the staging threshold ------------------------------------------------------------------------------------------------------------------
def vec_size(prefix, n, by):
    return vlen(prefix) + 1 + vlen(n) + n * (1 + by)


def craft_stage_vecs():
    """radix (BYTES 15: 16 bytes per element). For every emitting instance and every mis 0 .. 15: a Vec with STAGE - 16 < esz + mis <= STAGE (staged) and
    one with STAGE < esz + mis <= STAGE + 16 (direct); a short dense Trie of 1 .. 16 words in front of each chooses its mis."""
    width = "radix"
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/stage/vecs")
    todo = [(cls, mis, side) for cls in WG_CLASSES for mis in range(16) for side in ("under", "over")]
    rng.shuffle(todo)
    ps = sorted(rng.sample(range(1 << pb), 2 * len(todo)))
    h = len(header(len(ps)))
    sh = Shape("stage/vecs", width, k, pb, sb, by, {}, {})
    off = 0
    for i, (cls, mis, side) in enumerate(todo):
        pf, pe = ps[2 * i], ps[2 * i + 1]
        lowest = rng.getrandbits(sb - 8) << 8 | 0x10
        base = list(range(lowest, lowest + 16))  # one leaf node: the filler's size grows by one byte per word
        for m in range(1, 17):
            e = entry_bytes(sh, pf, "trie", base[:m])
            if (h + off + len(e)) & 15 == mis:
                break
        else:
            raise AssertionError("no filler for mis %d" % mis)
        sh.buckets[pf] = ("trie", base[:m])
        off += len(e)
        stage = stage_bytes(cls)
        lo, hi = (stage - 16, stage) if side == "under" else (stage, stage + 16)
        n = [n for n in range(stage // 16 - 2, stage // 16 + 3) if lo < vec_size(pe, n, by) + mis <= hi]
        assert len(n) == 1 and classify("vec", n[0], by) == cls, (cls, mis, side, n)
        sh.buckets[pe] = ("vec", _store(rng, sb, n[0], "vec"))
        sh.marks[pe] = "stage %s mis %d %s" % (cls, mis, side)
        off += vec_size(pe, n[0], by)
    return sh


def craft_stage_tries(width):
    """For the c64 emitter, the Trie of the longest prefix of a seeded sparse list that is still staged at its place, and behind it the shortest
    prefix of another list that is not (found by bisection: the entry grows with every word)."""
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/stage/tries/%s" % width)
    ps = sorted(rng.sample(range(1 << pb), 5))
    sh = Shape("stage/tries/%s" % width, width, k, pb, sb, by, {}, {})
    h = len(header(5))
    off = 0
    stage = stage_bytes("c64")
    for i, p in enumerate(ps):
        if i % 2 == 0:
            sh.buckets[p] = _filler(rng, sb)
            off += len(entry_bytes(sh, p, *sh.buckets[p]))
            continue
        pool = sparse(rng, sb, by, SER_CAP64)
        rng.shuffle(pool)
        mis = (h + off) & 15
        size = lambda n: len(entry_bytes(sh, p, "trie", sorted(pool[:n])))
        lo, hi = 33, SER_CAP64  # size(lo) + mis <= stage < size(hi) + mis
        assert size(lo) + mis <= stage < size(hi) + mis
        while hi - lo > 1:
            mid = (lo + hi) // 2
            if size(mid) + mis <= stage:
                lo = mid
            else:
                hi = mid
        n = lo if i == 1 else hi
        sh.buckets[p] = ("trie", sorted(pool[:n]))
        sh.marks[p] = "stage trie %s" % ("under" if i == 1 else "over")
        off += size(n)
    return sh


# ---- d. split Tries ----------------------------------------------------------------------------------------------------------------------------
SPLIT_WIDTHS = ("packed", "narrow64", "radix")


def _sub(rng, sb, by, top, n):
    """n ascending suffixes whose top byte is `top`"""
    return sorted(top << (8 * (by - 1)) | v for v in sm.distinct(rng, n, 8 * (by - 1)))


def _split_bucket(rng, sb, by, plan):
    out = []
    for top in sorted(plan):
        out += _sub(rng, sb, by, top, plan[top])
    return out


def craft_split(width):
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/split/%s" % width)
    T = 1 << top_bits(sb, by)
    plans = []
    if T == 4:
        plans += [("sub-ranges a", {0: 1, 1: 1024, 2: 1025, 3: 8192}), ("sub-ranges b", {0: 4096, 1: 4097, 3: 1})]
    else:
        step = T // 8
        plans += [("sub-ranges", {0: 1, step: 1024, step + 1: 1025, 2 * step: 4096, 2 * step + 1: 4097, 6 * step: 8192, T - 1: 1})]  # a gap of absent bytes between
    if T == 256:
        for c0 in (250, 251, 256):
            tops = sorted(rng.sample(range(1, 255), c0 - 2) + [0, 255]) if c0 < 256 else list(range(256))
            plans.append(("present %d" % c0, {t: rng.randrange(33, 40) for t in tops}))
    plans.append(("bad alone", {T // 2: 8193}))  # one present top byte
    plans.append(("bad beside", {0: 8193, 1: 5, T - 1: 7}))
    plans.append(("random", None))
    ps = sorted(rng.sample(range(1 << pb), 2 * len(plans) + 1))
    buckets, marks = {}, {}
    for i, p in enumerate(ps):
        if i % 2 == 0:
            buckets[p] = _filler(rng, sb)
        else:
            label, plan = plans[i // 2]
            buckets[p] = ("trie", _rand(rng, sb, 9000, "trie") if plan is None else _split_bucket(rng, sb, by, plan))
            marks[p] = "split " + label
    return _shape("split/%s" % width, width, buckets, marks)


def craft_split_max():
    """packed: Tries of 2^21 and 2^21 + 1 random words between ordinary neighbours (see the module's docstring for the route they take)"""
    width = "packed"
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/split/max")
    g = np.random.default_rng(21)
    ps = sorted(rng.sample(range(1 << pb), 5))
    buckets, marks = {}, {}
    for i, p in enumerate(ps):
        if i % 2 == 0:
            buckets[p] = _filler(rng, sb)
            continue
        n = SER_SPLIT_MAX + (i == 3)
        v = np.unique(g.integers(0, 1 << sb, size=n + n // 64, dtype=np.uint64))
        assert len(v) >= n
        buckets[p] = ("trie", v[:n].tolist())
        marks[p] = "length %d" % n
    return _shape("split/max", width, buckets, marks)


# ---- e. prefix varints -------------------------------------------------------------------------------------------------------------------------
VARIANTS = ("tiny", "wvec", "wtrie", "split")


def varint_prefixes(pb):
    return sorted({p for p in (0, 250, 251, 65535, 65536, (1 << pb) - 1) if p < 1 << pb})


def craft_varints(width, variant):
    """a bucket of the variant's kind at every prefix on a varint edge (the split Trie at 250 | 251 only, tiny Vecs elsewhere)"""
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/varints/%s/%s" % (width, variant))
    buckets, marks = {}, {}
    for p in varint_prefixes(pb):
        if variant == "tiny":
            b = ("vec", _rand(rng, sb, 7, "vec"))
        elif variant == "wvec":
            b = ("vec", _rand(rng, sb, min(300, 1 << (sb - 1)), "vec"))
        elif variant == "wtrie":
            b = ("trie", _rand(rng, sb, min(300, 1 << (sb - 1)), "trie"))
        elif p in (250, 251):
            b = ("trie", _rand(rng, sb, 8500, "trie"))
        else:
            b = ("vec", _rand(rng, sb, 3, "vec"))
        buckets[p] = b
        marks[p] = "prefix %d %s" % (p, variant)
    return _shape("varints/%s/%s" % (width, variant), width, buckets, marks)


def varint_cases():
    out = []
    for w in ALL_WIDTHS + ("pb24",):
        k, pb, sb, by = geom(w)
        for v in VARIANTS:
            if v == "split" and (by == 1 or 251 >= 1 << pb):
                continue
            out.append((w, v))
    return out


# ---- f. chunk geometry -------------------------------------------------------------------------------------------------------------------------
CHUNK_WIDTHS = ("packed", "wide")
CHUNK_CASES = ("127", "128", "129", "1000", "tiny_chunk", "long_first", "empty")


def craft_chunks(width, case):
    """127 | 128 | 129 | 1000 buckets of mixed classes (the hand-over is chunked from 128 on; 129 and 1000 leave the last chunk short, 129 also leaves
    chunks with nothing in them); `tiny_chunk`: 128 buckets, all of chunk 3 tiny; `long_first`: 160 buckets, every workgroup bucket in chunk 0; `empty`."""
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/chunks/%s/%s" % (width, case))
    nb = {"tiny_chunk": 128, "long_first": 160, "empty": 0}.get(case) if case in ("tiny_chunk", "long_first", "empty") else int(case)
    ps = sorted(rng.sample(range(1 << pb), nb))
    buckets, marks = {}, {}
    for r, p in enumerate(ps):
        ch, per = chunk_of(r, nb)
        x = rng.random()
        if case == "tiny_chunk":
            tiny = ch == 3 or x < 0.3
        elif case == "long_first":
            tiny = ch != 0
        else:
            tiny = x < 0.4
        if tiny:
            buckets[p] = ("vec", _rand(rng, sb, rng.randrange(1, SER_TINY + 1), "vec"))
            continue
        y = rng.random()
        n = rng.randrange(33, 400) if y < 0.8 or nb == 1000 and y < 0.97 else rng.randrange(1025, 1500) if y < 0.9 else rng.randrange(4097, 4500) if y < 0.97 else 8300
        kind = "trie" if rng.random() < 0.6 or n > SER_CAP1024 else "vec"
        buckets[p] = (kind, _store(rng, sb, n, kind))
    return _shape("chunks/%s/%s" % (width, case), width, buckets, marks)


# ---- stale high bits: an index built by insertion, with buckets a later batch does not touch --------------------------------------------------------
STALE_WIDTHS = ("packed", "wide", "radix")
# a Vec (c64), Tries of the c256, c1024 and split classes; then the shortest buckets: k_classify (kernels_bucket.hpp:194) leaves a single new word in
# the slot the partition put it in, the one place where the code itself says a slot is not rewritten
STALE_LENGTHS = (500, 2000, 6000, 9000, 1, 1, 1, 2, 17, 33)


def craft_stale(width):
    """(first batch, second batch) of words prefix << SB | suffix; the second touches other prefixes only. High prefixes, so that the bits above SB
    are set in the words the first batch stores."""
    k, pb, sb, by = geom(width)
    rng = random.Random("serde/stale/%s" % width)
    hi = [p | 1 << (pb - 1) | 1 for p in rng.sample(range(1 << pb), 3 * len(STALE_LENGTHS))]
    hi = list(dict.fromkeys(hi))[: len(STALE_LENGTHS)]
    assert len(hi) == len(STALE_LENGTHS)
    first, second = [], []
    for p, n in zip(hi, STALE_LENGTHS):
        first += [(p << sb) | s for s in sm.distinct(rng, n, sb)]
    others = [p for p in range(1 << pb) if p not in hi]
    for p in rng.sample(others, 6):
        second += [(p << sb) | s for s in sm.distinct(rng, rng.choice((3, 50, 1200)), sb)]
    rng.shuffle(first)
    rng.shuffle(second)
    return first, second, hi


shape = bs.shape  # fn(*args), computed once per process
STAGE_TRIE_WIDTHS = ("wide", "radix")

FAMILIES = {
    "lengths": [(craft_lengths, w, kind) for w in ALL_WIDTHS for kind in ("vec", "trie")],
    "patterns": [(craft_patterns, w) for w in ALL_WIDTHS],
    "stage": [(craft_stage_vecs,)] + [(craft_stage_tries, w) for w in STAGE_TRIE_WIDTHS],
    "split": [(craft_split, w) for w in SPLIT_WIDTHS],
    "varints": [(craft_varints, w, v) for w, v in varint_cases()],
    "chunks": [(craft_chunks, w, c) for w in CHUNK_WIDTHS for c in CHUNK_CASES],
}
CASES = [c for f in FAMILIES.values() for c in f]  # every shape but craft_split_max, the one slow one


def case_id(case):
    return "-".join([case[0].__name__[6:]] + list(case[1:]))
