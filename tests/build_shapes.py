"""Crafted batches for the bucket stage of the build (k_classify and the kernels behind its classes) and of `|=` (k_classify_merge): buckets
whose run length — resident words plus arriving words, duplicates included — sits exactly on either side of every class edge. Pure CPU: `random`
and `oracle.pyref`; a helper, not a test file. tests/test_build_shapes.py shows on the CPU what every shape delivers and that the model below
equals the C++ oracle; tests/test_gpu_build_classes.py compares the GPU's bytes, bucket table and stage accounting with it.

The model of `WordSet::insert_batch` on a bucket (/root/reference/src/wordset/mod.rs:187-216, src/trievec/mod.rs:72-115), in closed form:
  * a Vec keeps its stored order and appends the first occurrence of every new suffix in stream order;
  * after a group that touches it, a Vec of more than 1024 words becomes an ascending Trie — also when the group brought nothing new
    (mod.rs:213-214 checks the length of every touched container), which is what happens to the long Vecs `|=` leaves behind;
  * a Trie stays a Trie, ascending, at any length (a short Trie only comes out of a file);
  * a bucket no word of the batch belongs to keeps its bytes.
A prefix that the stream visits in several groups ends the same way: whichever group takes a Vec past 1024 words, the last state is the
ascending Trie of everything, and below 1024 the order is first occurrence in the stream. So one pass over the batch with a dict per touched
prefix gives the result. `|=` is `PyCBL.merge` as it stands.

Words are crafted directly as prefix << SUFFIX_BITS | suffix; the kernels see the same (prefix, suffix) records whatever sequence they came from.
"""
from __future__ import annotations

import random
from collections import namedtuple

from oracle import pyref
from oracle.pyref import PyCBL

import setops_model as sm

VEC, TRIE = 0, 1           # kernels_bucket.hpp: KIND_VEC / KIND_TRIE
THRESHOLD = 1024           # common.hpp:30 VEC_THRESHOLD
SMALL_MAX = 32             # kernels_bucket.hpp: SMALL_MAX, all-pairs in a slice of a wave up to here
MED_ITEMS = 8              # kernels_bucket.hpp: MED_ITEMS, slots per lane of the counting-sort classes
BIG_MAX = 1 << 18          # kernels_bucket.hpp: BIG_MAX, longest run of the split path
BIG_SUB = 1024             # kernels_bucket.hpp: BIG_SUB, words per sub-range big_bits aims at
LDS_MAX = 4096             # bucket_stage.hpp: bucket_stage, k_classify's lds_max, the same for every suffix width
PK_BITS = 12               # kernels_bucket.hpp: PK_BITS, a packed element is suffix + 12-bit position in 64 bits
MSD_MAX_BITS = 128         # kernels_bucket.hpp: msd_takes, wide suffixes up to SB + 12 <= 128 take the counting sort, wider ones the radix kernel
DIRECT_UPTO = 512 * MED_ITEMS  # setops.hpp: merge_direct, direct_upto, both-sided buckets `|=` reads in place

BUILD_CLASSES = ("CLS_S16", "CLS_S32", "CLS_M16", "CLS_M32", "CLS_M64", "CLS_M128", "CLS_M256", "CLS_M512", "CLS_BIG", "CLS_HUGE")
MERGE_CLASSES = ("CLS_UNION", "CLS_M16", "CLS_M64", "CLS_M128", "CLS_M256", "CLS_M512", "CLS_BIG", "CLS_M1024", "CLS_HUGE")
MSD_CLASSES = ("CLS_M16", "CLS_M32", "CLS_M64", "CLS_M128", "CLS_M256", "CLS_M512")


def classify_build(rc, rkind, c, lds_max=LDS_MAX):
    """k_classify (kernels_bucket.hpp): resident count, resident kind, run length -> class, "untouched" or "single"."""
    if rc != 0 and c == rc:
        return "untouched"                                   # :191
    if c == 1 and rc == 0:
        return "single"                                      # :194
    if c <= SMALL_MAX and rkind != TRIE:
        return "CLS_S16" if c <= 16 else "CLS_S32"            # :197
    if c <= 16 * MED_ITEMS:
        return "CLS_M16"                                     # :198
    if c <= 32 * MED_ITEMS:
        return "CLS_M32"                                     # :199
    if c <= 64 * MED_ITEMS:
        return "CLS_M64"                                     # :200
    if c <= 128 * MED_ITEMS:
        return "CLS_M128"                                    # :201
    if c <= 256 * MED_ITEMS and c <= lds_max:
        return "CLS_M256"                                    # :202
    if c <= 512 * MED_ITEMS and c <= lds_max:
        return "CLS_M512"                                    # :203
    return "CLS_BIG" if c <= BIG_MAX else "CLS_HUGE"          # :204-205


def classify_merge(cs, co, ks, ko, wide, union_path=True):
    """k_classify_merge (kernels_bucket.hpp); med_max_threads is 512 for wide suffixes, 1024 otherwise (setops.hpp: merge_direct)."""
    c = cs + co
    if co == 0:
        return "self_only"                                   # :311
    if cs == 0:
        return "other_only"                                  # :312
    if union_path and ks == TRIE and ko == TRIE:
        return "CLS_UNION"                                   # :313
    if c <= 16 * MED_ITEMS:
        return "CLS_M16"                                     # :314
    if c <= 64 * MED_ITEMS:
        return "CLS_M64"                                     # :315
    if c <= 128 * MED_ITEMS:
        return "CLS_M128"                                    # :316
    if c <= 256 * MED_ITEMS:
        return "CLS_M256"                                    # :317
    if c <= 512 * MED_ITEMS:
        return "CLS_M512"                                    # :318
    if ks == TRIE and ko == TRIE and c <= BIG_MAX:
        return "CLS_BIG"                                     # :319
    if c <= 1024 * MED_ITEMS and not wide:
        return "CLS_M1024"                                   # :320
    return "CLS_HUGE"                                        # :321


def big_bits(c):
    """kernels_bucket.hpp: big_bits. A big run is cut into 2^bits sub-ranges; the count changes at 8193, 16385, ..."""
    b = 1
    while b < 8 and ((c - 1) >> b) >= BIG_SUB:
        b += 1
    return b


# ---- configurations, by property (tests/test_build_shapes.py confirms each with pyref.params) -----------------------------------------------
CONFIGS = {
    "packed": (23, 10),    # SB = 42: SB + PK_BITS <= 64, packed elements, the walk kernel, the pre-pass of the long runs (SB < 64)
    "narrow64": (35, 13),  # SB = 64: one-word suffix, not packed, no pre-pass
    "wide": (45, 16),      # SB = 81: two-word suffix the counting sort takes
    "radix": (59, 8),      # SB = 117 > 116: every class takes the LDS radix kernel, long runs the general kernel
}


def props(name):
    k, pb = CONFIGS[name]
    sb = pyref.params(k, pb)["SB"]
    wide = sb > 64                                           # common.hpp:26 wide_suffix
    return dict(k=k, pb=pb, sb=sb, wide=wide, packed=not wide and sb + PK_BITS <= 64,  # bucket_stage.hpp: with_packed
                msd=not wide or sb + 12 <= MSD_MAX_BITS,     # msd_takes
                prepass=not wide and sb < 64)                # bucket_stage.hpp: bucket_stage, the pre-pass of the long runs


# ---- the model -------------------------------------------------------------------------------------------------------------------------------
def insert_batch(c: PyCBL, words):
    """WordSet::insert_batch of `words` into c, in closed form (see the module's docstring). O(len(words))."""
    sb = c.P["SB"]
    mask = (1 << sb) - 1
    touched = {}
    for w in words:
        touched.setdefault(w >> sb, {}).setdefault(w & mask, None)
    for p, new in touched.items():
        b = c.buckets.setdefault(p, ["vec", []])
        if b[0] == "trie":
            b[1] = sorted(set(b[1]).union(new))
            continue
        have = set(b[1])
        b[1] += [s for s in new if s not in have]
        if len(b[1]) > THRESHOLD:
            b[0] = "trie"
            b[1].sort()
    return c


def serialize(c: PyCBL) -> bytes:
    """PyCBL.serialize()'s bytes (tests/test_build_shapes.py compares the two), quicker on long Tries of wide suffixes: the chain of nodes under a
    subtree that holds one element is written in a loop, not by one call per byte of the suffix."""
    by = c.P["BYTES"]
    vi = PyCBL._varint

    def trie(items, depth):
        if len(items) == 1:
            raw = items[0].to_bytes(by, "big")[depth:]
            return b"".join(b"\x01" + raw[i: i + 1] + b"\x01" for i in range(len(raw) - 1)) + b"\x01" + raw[-1:] + b"\x00"
        shift = 8 * (by - 1 - depth)
        groups = {}
        for s in items:
            groups.setdefault((s >> shift) & 0xFF, []).append(s)
        keys = sorted(groups)
        out = vi(len(keys)) + bytes(keys)
        if depth == by - 1:
            return out + vi(0)
        return out + vi(len(keys)) + b"".join(trie(groups[key], depth + 1) for key in keys)

    out = [bytes([1 if c.canonical else 0]), vi(len(c.buckets))]
    for p in sorted(c.buckets):
        kind, items = c.buckets[p]
        out.append(vi(p))
        if kind == "vec":
            lead = vi(by)
            out.append(vi(0) + vi(len(items)) + b"".join(lead + s.to_bytes(by, "little") for s in items))
        else:
            out.append(vi(1) + trie(sorted(items), 0) + vi(len(items)))
    return b"".join(out)


def table(c: PyCBL):
    """{prefix: (length, kind)} as CBL.bucket_table_np reports it"""
    return {p: (len(items), TRIE if kind == "trie" else VEC) for p, (kind, items) in c.buckets.items()}


def model_of(shape_or_buckets, k=None, pb=None):
    if k is None:
        return sm.from_buckets(shape_or_buckets.k, shape_or_buckets.pb, False, shape_or_buckets.resident)
    return sm.from_buckets(k, pb, False, shape_or_buckets)


# ---- values ----------------------------------------------------------------------------------------------------------------------------------
PATTERNS = ("random", "shared_top", "sentinels")


class Values:
    """Distinct suffixes of one bucket: `random`; `shared_top`: all share their top 16 bits, so one sub-bucket of the counting sort is crowded
    without a repeat; `sentinels`: the first two handed out are 0 and 2^SB - 1."""

    def __init__(self, rng, sb, pattern):
        self.rng, self.sb, self.pattern, self.seen = rng, sb, pattern, set()
        self.top = rng.getrandbits(16) << (sb - 16)
        self.pending = [0, (1 << sb) - 1] if pattern == "sentinels" else []

    def take(self, n):
        out = []
        while len(out) < n:
            if self.pending:
                v = self.pending.pop(0)
            elif self.pattern == "shared_top":
                v = self.top | self.rng.getrandbits(self.sb - 16)
            else:
                v = self.rng.getrandbits(self.sb)
            if v not in self.seen:
                self.seen.add(v)
                out.append(v)
        return out


FILLS = ("distinct", "present", "one_value", "three_values", "twice", "to_1024", "to_1025")
RKINDS = ("none", "vec", "trie", "lvec")  # lvec: a Vec of more than 1024 words, as `|=` leaves them

Run = namedtuple("Run", "prefix rkind rlen arriving c fill pattern resident stream distinct cls")


def final_distinct(rlen, a, fill):
    """the bucket's length after the batch, from the fill's definition"""
    return {"distinct": rlen + a, "present": rlen, "one_value": rlen + 1, "three_values": rlen + min(3, a), "twice": rlen + (a + 1) // 2,
            "to_1024": 1024, "to_1025": 1025}[fill]


def make_run(rng, sb, prefix, rkind, rlen, c, fill, pattern):
    """One bucket: `rlen` resident suffixes of kind `rkind` (stored order) and c - rlen arriving ones in stream order."""
    a = c - rlen
    assert a >= 1 and (rlen == 0) == (rkind == "none") and (rkind != "lvec" or rlen > THRESHOLD)
    vals = Values(rng, sb, pattern)
    resident = vals.take(rlen)
    if rkind == "trie":
        resident.sort()
    elif rkind == "lvec":  # what `|=` leaves: self's elements ascending, other's new ones ascending behind them
        cut = rlen * 2 // 3
        resident = sorted(resident[:cut]) + sorted(resident[cut:])
    else:
        rng.shuffle(resident)
    if fill == "distinct":
        stream = vals.take(a)
    elif fill == "present":
        assert rlen
        stream = rng.sample(resident, a) if a <= rlen else rng.choices(resident, k=a)
        if pattern == "sentinels" and a >= 2 and rlen >= 2:
            stream[0], stream[-1] = 0, (1 << sb) - 1
    elif fill == "one_value":
        stream = vals.take(1) * a
    elif fill == "three_values":
        v = vals.take(min(3, a))
        stream = [v[i % len(v)] for i in range(a)]
    elif fill == "twice":
        v = vals.take(a // 2)
        stream = v + vals.take(a & 1) + v
    else:
        need = final_distinct(rlen, a, fill) - rlen
        assert 0 <= need <= a and (need or rlen), (rlen, a, fill)
        v = vals.take(need)
        stream = v + rng.choices(v + resident, k=a - need)
        rng.shuffle(stream)
    kind = TRIE if rkind == "trie" else VEC
    return Run(prefix, rkind, rlen, a, c, fill, pattern, resident, stream, final_distinct(rlen, a, fill), classify_build(rlen, kind, c))


def describe(run):
    """what a failure message says about a bucket"""
    return dict(prefix=run.prefix, resident=(run.rkind, run.rlen), c=run.c, fill=run.fill, pattern=run.pattern, cls=run.cls)


# ---- build shapes ----------------------------------------------------------------------------------------------------------------------------
BUILD_LENGTHS = (1, 2, 16, 17, 32, 33, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 16384, 16385)
HUGE_LENGTHS = (BIG_MAX, BIG_MAX + 1)
COMPOSITIONS = ("alone", "beside_distinct", "beside_repeats", "interleaved")
_ROT = ("distinct", "present", "twice", "three_values", "one_value")
WITNESS_C = 100  # a CLS_M16 run: 33 .. 128 words


TRIE_OVER, LVEC_LEN, VEC_UNDER, FILE_TRIE = 1100, 1400, 500, 700  # resident lengths: a Trie / a long Vec past the threshold, a Vec / a Trie out of a file below it


def build_specs(c, i, comp):
    """(resident kind, resident length, fill, pattern) of the runs of length c in composition `comp`; i: index of c's edge pair, which rotates fills
    and patterns so that both sides of an edge get the same ones. One row per run: (the lengths it applies to, the compositions, the spec).
    Every composition gets the first four rows; `alone` carries the full set, thinned above 4097 and again above 8193 words, where a run costs most."""
    pat = lambda j: PATTERNS[(i + j) % 3]
    rot = lambda j: _ROT[(i + j) % 5]
    short = 2 <= c <= SMALL_MAX + 1  # a resident Trie of up to 32 words: the small classes must refuse it
    every, alone, beside, inter = COMPOSITIONS, ("alone",), ("alone", "beside_distinct", "beside_repeats"), ("interleaved",)
    rows = [
        (True, every, ("none", 0, "distinct", pat(0))),
        (c >= 2, every, ("vec", min(c // 2, THRESHOLD), rot(0), pat(1))),
        (short, every, ("trie", c - 1, rot(1), pat(2))),
        (c > SMALL_MAX + 1, every, ("trie", min(c // 2, TRIE_OVER), rot(1), pat(2))),
        (c >= 1025, beside, ("none", 0, "to_1024", pat(1))),
        (c >= 2048, inter, ("vec", VEC_UNDER, "to_1025", "random")),
        (1025 <= c <= 8193, alone, ("none", 0, "to_1025", pat(0))),
        (2048 <= c <= 8193, alone, ("lvec", LVEC_LEN, "present", pat(0))),  # nothing new: a Trie all the same
        (2 <= c <= 4097, alone, ("none", 0, ("twice", "three_values", "one_value")[i % 3], pat(2))),
        (2 <= c <= 4097, alone, ("vec", min(c - 1, THRESHOLD), rot(2), "random")),
        (short, alone, ("trie", max(1, c // 2), rot(3), pat(0))),
        (2048 <= c <= 4097, alone, ("vec", VEC_UNDER, ("to_1024", "to_1025")[i % 2], "shared_top")),
        (2048 <= c <= 4097, alone, ("lvec", LVEC_LEN, "distinct", pat(1))),
        (2048 <= c <= 4097, alone, ("trie", FILE_TRIE, rot(3), pat(0))),  # a short Trie out of a file under a long run
    ]
    return [spec for applies, comps, spec in rows if applies and comp in comps]


BuildShape = namedtuple("BuildShape", "name comp k pb sb resident batches runs")  # resident: {prefix: (kind, items)}; batches: [(words, [run index])]


def _resident_of(runs):
    return {r.prefix: ("trie" if r.rkind == "trie" else "vec", list(r.resident)) for r in runs if r.rlen}


def _interleave(rng, runs, sb):
    """the streams of the runs dealt into one batch in pieces of 1 .. 64 words, prefix after prefix, each run's own order kept"""
    at = [0] * len(runs)
    live = list(range(len(runs)))
    words = []
    while live:
        rng.shuffle(live)
        for j in list(live):
            r = runs[j]
            n = rng.randrange(1, 65)
            words += [(r.prefix << sb) | s for s in r.stream[at[j]: at[j] + n]]
            at[j] += n
            if at[j] >= r.arriving:
                live.remove(j)
    return words


def craft_build(name, comp, lengths=None):
    k, pb = CONFIGS[name]
    sb = pyref.params(k, pb)["SB"]
    rng = random.Random("%s/%s" % (name, comp))
    witness = comp in ("beside_distinct", "beside_repeats")
    if lengths is None:
        lengths = BUILD_LENGTHS
    todo = [(c, spec) for c in lengths for spec in build_specs(c, BUILD_LENGTHS.index(c) // 2, comp)]
    prefixes = rng.sample(range(1 << pb), len(todo) * (2 if witness else 1))
    runs, batches = [], []
    for (c, (rkind, rlen, fill, pattern)), p in zip(todo, prefixes):
        runs.append(make_run(rng, sb, p, rkind, rlen, c, fill, pattern))
    if comp == "interleaved":
        batches.append((_interleave(rng, runs, sb), list(range(len(runs)))))
    else:
        for j, r in enumerate(list(runs)):
            words = [(r.prefix << sb) | s for s in r.stream]
            mates = [j]
            if witness:  # a CLS_M16 run on a prefix of its own: distinct words, or one value (the counting sort gives up: repeat_mode)
                w = make_run(rng, sb, prefixes[len(todo) + j], "none", 0, WITNESS_C, "distinct" if comp == "beside_distinct" else "one_value", "random")
                runs.append(w)
                mates.append(len(runs) - 1)
                ww = [(w.prefix << sb) | s for s in w.stream]
                words = ww + words if j % 2 else words + ww
            batches.append((words, mates))
    return BuildShape(name, comp, k, pb, sb, _resident_of(runs), batches, runs)


def craft_huge(name):
    """Runs of 2^18 and 2^18 + 1 words, each alone in its batch: a fill of repeats that leaves a Vec of 1024 words, and a mostly distinct one on
    top of a resident Trie (resident Tries keep the oracle's check of these shapes fast: it scans a Vec linearly)."""
    k, pb = CONFIGS[name]
    sb = pyref.params(k, pb)["SB"]
    rng = random.Random("%s/huge" % name)
    runs, batches = [], []
    prefixes = rng.sample(range(1 << pb), 4)
    specs = [(c, spec) for c in HUGE_LENGTHS for spec in (("vec", 300, "to_1024", "random"), ("trie", 1500, "distinct", "random"))]
    for j, ((c, (rkind, rlen, fill, pattern)), p) in enumerate(zip(specs, prefixes)):
        r = make_run(rng, sb, p, rkind, rlen, c, fill, pattern)
        if fill == "distinct":  # mostly distinct: the last 5000 arrivals repeat the first 5000
            stream = r.stream[:-5000] + r.stream[:5000]
            r = r._replace(stream=stream, fill="mostly_distinct", distinct=rlen + r.arriving - 5000)
        runs.append(r)
        batches.append(([(p << sb) | s for s in r.stream], [j]))
    return BuildShape(name, "huge", k, pb, sb, _resident_of(runs), batches, runs)


# ---- `|=` shapes -----------------------------------------------------------------------------------------------------------------------------
MERGE_LENGTHS = (2, 128, 129, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
MERGE_GROUPS = ((2,), (128, 129), (512, 513), (1024, 1025), (2048, 2049), (4096, 4097), (8192, 8193))
# Thinning, and why. Up to 1025 words every feasible (self kind, other kind) pair is crafted at every edge. From 2048 words on the full product of
# 16 feasible pairs x 5 overlaps x 2 lengths would be 0.7 M words at 4096 | 4097 and 1.3 M at 8192 | 8193 per configuration, against about 60 k for a
# whole composition elsewhere; so each of those edges gets the four pairs that decide a class in k_classify_merge (Trie |= Trie, Vec |= Vec, a long
# Vec on either side of a Trie) and a rotating third of the others (kind_pairs), and every crafted pair gets ONE overlap by rotation. What that pins
# is printed and asserted by tests/test_build_shapes.py: per edge the pairs, across the edges every (kind, overlap) on either side — not every
# (self kind, other kind, overlap) triple at every edge. Both lengths of an edge get the same pairs and overlaps where both can hold them.
MKINDS = ("vec", "svec", "lvec", "trie", "strie")  # Vec shuffled / Vec ascending (both <= 1024), Vec > 1024, Trie, Trie of <= 32 words
_MRANGE = {"vec": (1, THRESHOLD), "svec": (1, THRESHOLD), "lvec": (THRESHOLD + 1, 1 << 30), "trie": (1, 1 << 30), "strie": (1, SMALL_MAX)}
OVERLAPS = ("disjoint", "contained", "interleaved", "below", "above")

Pair = namedtuple("Pair", "prefix ks ko cs co overlap self_items other_items")
MergeShape = namedtuple("MergeShape", "name group k pb sb a b pairs")  # a, b: {prefix: (kind, items)}


def is_trie(mk):
    return TRIE if mk in ("trie", "strie") else VEC


def split(c, ks, ko):
    """cs with cs + co = c inside both kinds' ranges, as near c / 2 as they allow (a Trie prefers more than 32 words); None: no such pair"""
    (ls, hs), (lo, ho) = _MRANGE[ks], _MRANGE[ko]
    a, b = max(ls, c - ho), min(hs, c - lo)
    if a > b:
        return None
    return min(max(c // 2, a), b)


def _store(rng, mk, items):
    items = sorted(items)
    if mk == "vec":
        rng.shuffle(items)
    elif mk == "lvec":
        odd = items[1::2]
        items = items[0::2] + odd  # two ascending pieces that interleave
    return ["trie" if is_trie(mk) else "vec", items]


def _overlap(rng, sb, cs, co, overlap):
    pool = sorted(sm.distinct(rng, cs + co, sb))
    if overlap == "below":
        return pool[co:], pool[:co]
    if overlap == "above":
        return pool[:cs], pool[cs:]
    rng.shuffle(pool)
    s, o = pool[:cs], pool[cs:]
    if overlap == "contained":  # all of other in self (or, other being the longer, all of self in other)
        if co <= cs:
            o = rng.sample(s, co)
        else:
            o = s + o[: co - cs]
    elif overlap == "interleaved":
        n = (min(cs, co) + 1) // 2
        o = rng.sample(s, n) + o[: co - n]
    return s, o


def kind_pairs(c, gi):
    """The (self kind, other kind) pairs of a merge edge: all that have a split up to 1025 words; beyond, the four that decide a class (Trie |= Trie,
    Vec |= Vec, long Vec on either side of a Trie) and a third of the others, rotating with the edge pair so that 2048 .. 8193 cover them all."""
    feasible = [(i, j) for i in range(5) for j in range(5) if split(c, MKINDS[i], MKINDS[j]) is not None]
    if c <= 1025:
        return feasible
    forced = {(3, 3), (0, 0), (2, 3), (3, 2)}
    return [(i, j) for i, j in feasible if (i, j) in forced or (i * 5 + j + gi) % 3 == 0]


def craft_merge(name, gi):
    k, pb = CONFIGS[name]
    sb = pyref.params(k, pb)["SB"]
    rng = random.Random("%s/merge/%d" % (name, gi))
    todo = [(c, i, j) for c in MERGE_GROUPS[gi] for i, j in kind_pairs(c, gi)]
    prefixes = rng.sample(range(1 << pb), len(todo) + 10)
    a, b, pairs = {}, {}, []
    for n, ((c, i, j), p) in enumerate(zip(todo, prefixes)):
        ks, ko = MKINDS[i], MKINDS[j]
        cs = split(c, ks, ko)
        ov = OVERLAPS[(i + 2 * j + 3 * gi) % 5]  # (every kind on either side meets every overlap)
        s, o = _overlap(rng, sb, cs, c - cs, ov)
        a[p], b[p] = _store(rng, ks, s), _store(rng, ko, o)
        pairs.append(Pair(p, ks, ko, cs, c - cs, ov, a[p][1], b[p][1]))
    sizes = {"vec": 40, "svec": 40, "lvec": 1100, "trie": 1100, "strie": 7}
    for n, mk in enumerate(MKINDS):  # buckets only one side holds, of every kind
        for side, p in ((a, prefixes[len(todo) + 2 * n]), (b, prefixes[len(todo) + 2 * n + 1])):
            side[p] = _store(rng, mk, sm.distinct(rng, sizes[mk], sb))
    return MergeShape(name, gi, k, pb, sb, a, b, pairs)


def craft_merge_huge(name):
    """One Trie |= Trie pair of 2^18 and one of 2^18 + 1 words: CLS_UNION, and CLS_BIG / CLS_HUGE with the union route off."""
    k, pb = CONFIGS[name]
    sb = pyref.params(k, pb)["SB"]
    rng = random.Random("%s/merge/huge" % name)
    a, b, pairs = {}, {}, []
    for c, p in zip(HUGE_LENGTHS, rng.sample(range(1 << pb), 2)):
        cs = c // 2 + 1000
        s, o = _overlap(rng, sb, cs, c - cs, "interleaved")
        a[p], b[p] = _store(rng, "trie", s), _store(rng, "trie", o)
        pairs.append(Pair(p, "trie", "trie", cs, c - cs, "interleaved", a[p][1], b[p][1]))
    return MergeShape(name, "huge", k, pb, sb, a, b, pairs)


def merge_classes(shape, union_path):
    wide = shape.sb > 64
    return [classify_merge(pr.cs, pr.co, is_trie(pr.ks), is_trie(pr.ko), wide, union_path) for pr in shape.pairs]


def merge_units(shape, union_path, direct, result):
    """The words cblx_stage_units reports for one `|=` (setops.hpp: merge_direct, `prof`), from the restated classification; `result`: the merged model."""
    wide = shape.sb > 64
    direct = direct and (not wide or shape.sb + 12 <= MSD_MAX_BITS)  # setops.hpp: merge_direct, `direct`
    un = {"merge_gather": 0, "bucket_medium": 0, "bucket_huge": 0, "bucket_big": 0}
    for p in set(shape.a) | set(shape.b):
        cs, co = len(shape.a.get(p, (0, ()))[1]), len(shape.b.get(p, (0, ()))[1])
        ks = TRIE if p in shape.a and shape.a[p][0] == "trie" else VEC
        ko = TRIE if p in shape.b and shape.b[p][0] == "trie" else VEC
        cls = classify_merge(cs, co, ks, ko, wide, union_path)
        c = cs + co
        if cls in ("self_only", "other_only"):
            un["merge_gather"] += c
        elif cls == "CLS_UNION":
            un["bucket_big"] += len(result.buckets[p][1])  # priced on what the union writes
        elif cls == "CLS_BIG":
            un["bucket_big"] += c
            un["merge_gather"] += c
        elif cls == "CLS_HUGE":
            un["bucket_huge"] += c
            un["merge_gather"] += c
        else:
            un["bucket_medium"] += c
            if cls == "CLS_M1024" or not direct:
                un["merge_gather"] += c
    return un


_cache = {}


def shape(fn, *args):
    """fn(*args), computed once per process and left unchanged by its users"""
    key = (fn.__name__,) + args
    if key not in _cache:
        _cache[key] = fn(*args)
    return _cache[key]
