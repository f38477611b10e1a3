"""k_bucket_sorted at every run length where one of its straight-line phases changes shape: crafted words through insert_words_device into single
buckets, index bytes, count and bucket table against the closed-form model of tests/build_shapes.py (or PyCBL.merge), no tolerance.

The offsets table is scanned in a fixed layout — thread t owns entries [8 t, 8 t + 8) whatever NB is, read and written as one 16-byte word, the whole
table zeroed up front — and the phases around the walk (counting, placement, put-back, heads, both store loops) mask a lane's eight slots one by
one. What can go wrong is at the edges: the last lane's partly owned slots (c = k THREADS +- 1 around every value of `per`), a class's first and
last length, the table's entries behind NB (c just above a power of two, short runs of a class above their length), the sorted order's first and
last slot (a repeat of the smallest / the greatest suffix), and a sub-bucket on either side of the crowding limit."""
import random

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from oracle import pyref  # noqa: E402

import build_shapes as bs  # noqa: E402  (tests/)

M64 = (1 << 64) - 1
PACKED = bs.CONFIGS["packed"]  # SB + 12 <= 64: the walk kernel's narrow elements
WIDE = (59, 16)                # 64 < SB, SB + 12 <= 128: its 16-byte elements
MSD_LIMIT = 48                 # kernels_bucket.hpp: a sub-bucket of more entries is handed on

LENGTHS_2048 = (1025, 1026, 1279, 1280, 1281, 1535, 1536, 1537, 1791, 1792, 1793, 2047, 2048)  # 256 threads: per = 5 | 6 | 7 | 8
LENGTHS_4096 = (2049, 2559, 2560, 2561, 3071, 3072, 3073, 3583, 3584, 3585, 4095, 4096)        # 512 threads
VARIANTS = ("no_repeat", "repeat_adjacent", "repeat_far", "repeat_of_smallest", "repeat_of_greatest", "stays_vec", "sub_bucket_48", "sub_bucket_49",
            "lowest_bit", "highest_bit_below_sub", "second_insert_into_trie")


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


def _same(g, m, what):
    want = bs.serialize(m)
    if g.serialize() != want:
        got = {p: ("trie" if kd else "vec", list(items)) for p, kd, items in g.buckets()}
        bad = []
        for p in sorted(set(got) | set(m.buckets)):
            gk, gi = got.get(p, ("absent", []))
            wk, wi = m.buckets.get(p, ["absent", []])
            if (gk, gi) != (wk, list(wi)):
                first = next((i for i, (x, y) in enumerate(zip(gi, wi)) if x != y), min(len(gi), len(wi)))
                bad.append((p, gk, len(gi), wk, len(wi), "first difference at slot %d" % first))
        pytest.fail(f"{what}: bytes differ; (prefix, got kind, length, wanted kind, length): {bad[:4]}")
    assert g.count() == m.count(), what
    assert _table(g) == bs.table(m), what
    assert g.validate(strict=False) == 0, what


def _sb(k, pb):
    return pyref.params(k, pb)["SB"]


def _nbits(c, sb):
    return min(max((c - 1).bit_length(), 0) or 1, sb)  # the kernel's ceil(log2 c), at most SB


def _distinct(rng, n, sb, avoid_top=None, nbits=0):
    out, seen = [], set()
    while len(out) < n:
        v = rng.getrandbits(sb)
        if v in seen or (avoid_top is not None and v >> (sb - nbits) == avoid_top):
            continue
        seen.add(v)
        out.append(v)
    return out


def _run_one(k, pb, batches, what):
    """every batch of (prefix, suffixes in stream order) into a fresh index and the model; compared after each"""
    _need_gpu()
    sb = _sb(k, pb)
    g = cbl_amd.CBL(k, pb)
    assert g.consts()["suffix_bits"] == sb
    m = bs.model_of({}, k, pb)
    for bi, (prefix, stream) in enumerate(batches):
        words = [(prefix << sb) | s for s in stream]
        bs.insert_batch(m, words)
        _insert_words(g, words)
        _same(g, m, f"{what}, batch {bi} of {len(stream)} words")
    g.close()
    return m


# ---- a. distinct words at every length where `per`, the last lane's share or NB moves ---------------------------------------------------------
@pytest.mark.parametrize("c", LENGTHS_2048 + LENGTHS_4096)
def test_distinct_run_at_every_per_edge(c):
    """One bucket of c distinct words on an empty index: c = 1025, 1026 and 2049 (a class's first lengths, NB just doubled), 256 k - 1 | 256 k |
    256 k + 1 for per = 5 .. 8 of the 2048-slot class, 512 k - 1 | 512 k | 512 k + 1 of the 4096-slot class, and both classes' last two lengths."""
    k, pb = PACKED
    rng = random.Random(f"distinct {c}")
    m = _run_one(k, pb, [(rng.randrange(1 << pb), _distinct(rng, c, _sb(k, pb)))], f"c = {c}")
    assert set(bs.table(m).values()) == {(c, bs.TRIE)}


# ---- b. the shapes of a run, at c = 1300 (per = 6 of 8, NB = 2048) and c = 3000 (per = 6 of 8, NB = 4096) ---------------------------------------
def _variant(rng, variant, c, sb):
    """-> (batches of suffixes, expected (length, kind))"""
    nbits = _nbits(c, sb)
    if variant == "no_repeat":
        return [_distinct(rng, c, sb)], (c, bs.TRIE)
    if variant in ("repeat_adjacent", "repeat_far"):
        v = _distinct(rng, c - 1, sb)
        at, to = (c // 2, c // 2 + 1) if variant == "repeat_adjacent" else (3, c - 5)
        v.insert(to, v[at])
        return [v], (c - 1, bs.TRIE)
    if variant in ("repeat_of_smallest", "repeat_of_greatest"):
        v = _distinct(rng, c - 1, sb)
        if variant == "repeat_of_smallest":  # the two copies are the sorted order's slots 0 and 1; the first copy is the stream's first word
            x = min(v)
            v.remove(x)
            v = [x] + v[: c // 2] + [x] + v[c // 2:]
        else:                                # ... its last two slots; the second copy is the stream's last word
            x = max(v)
            v.append(x)
        return [v], (c - 1, bs.TRIE)
    if variant == "stays_vec":  # more than 1024 words, at most 1024 distinct: handed on before anything is written
        d = _distinct(rng, 1024, sb)
        v = d + [d[rng.randrange(1024)] for _ in range(c - 1024)]
        rng.shuffle(v)
        return [v], (1024, bs.VEC)
    if variant in ("sub_bucket_48", "sub_bucket_49"):  # one sub-bucket (top nbits of the suffix) at the limit: kept | handed on; the rest sparse
        n = MSD_LIMIT + (variant == "sub_bucket_49")
        top = rng.randrange(1, (1 << nbits) - 1)
        low = sb - nbits
        crowd = [(top << low) | x for x in _distinct(rng, n, low)]
        v = crowd + _distinct(rng, c - n, sb, avoid_top=top, nbits=nbits)
        rng.shuffle(v)
        return [v], (c, bs.TRIE)
    if variant in ("lowest_bit", "highest_bit_below_sub"):  # pairs that differ in one bit only, inside one sub-bucket
        bit = 1 if variant == "lowest_bit" else 1 << (sb - nbits - 1)
        half = [x & ~bit for x in _distinct(rng, c, sb)]
        half = list(dict.fromkeys(half))[: c // 2]
        v = half + [x | bit for x in half]
        v += _distinct(rng, c, sb)[: c - len(v)]
        v = list(dict.fromkeys(v))
        rng.shuffle(v)
        return [v], (len(v), bs.TRIE)
    if variant == "second_insert_into_trie":  # the run is the resident Trie plus the arriving words, some of them present
        first = _distinct(rng, c - c // 6, sb)
        a = c - len(first)
        fresh = [x for x in _distinct(rng, a, sb) if x not in set(first)][: a - a // 2]
        second = fresh + rng.sample(first, a - len(fresh))
        rng.shuffle(second)
        return [first, second], (len(first) + len(fresh), bs.TRIE)
    raise AssertionError(variant)


@pytest.mark.parametrize("c", [1300, 3000])
@pytest.mark.parametrize("variant", VARIANTS)
def test_run_shapes(variant, c):
    """no repeat (nothing compacted); one repeated suffix, its copies adjacent in the stream or far apart (the compacting store); a repeat of the
    smallest suffix, first word of the stream, and of the greatest, last word of the stream (the heads phase's slot 0 and its last slot); more than
    1024 words of 1024 distinct ones (stays a Vec: handed to the claim table); a sub-bucket of exactly 48 and of 49 entries (kept | handed on); pairs
    that differ only in their lowest bit, and in the highest bit below the sub-bucket bits; a second insert into a bucket that is a Trie already."""
    k, pb = PACKED
    sb = _sb(k, pb)
    assert sb + bs.PK_BITS <= 64
    rng = random.Random(f"{variant} {c}")
    batches, want = _variant(rng, variant, c, sb)
    assert sum(len(b) for b in batches) == c or variant in ("lowest_bit", "highest_bit_below_sub")
    prefix = rng.randrange(1 << pb)
    m = _run_one(k, pb, [(prefix, b) for b in batches], f"{variant}, c = {c}")
    assert bs.table(m) == {prefix: want}


@pytest.mark.parametrize("c,distinct", [(2000, 1100), (4000, 1100), (4000, 2100)])
def test_short_run_in_the_4096_slot_class(c, distinct):
    """A run full of repeats with more than 1024 distinct words: one value fills a sub-bucket past the limit, the claim table removes the repeats and
    hands the distinct words on to the 4096-slot instantiation at their new length — 1100 words there have NB = 2048 of 4096 entries and per = 3,
    2100 have NB = 4096 and per = 5: the scan's entries behind NB and the walk's `per <= 4` arm."""
    k, pb = PACKED
    sb = _sb(k, pb)
    rng = random.Random(f"retry {c} {distinct}")
    d = _distinct(rng, distinct, sb)
    v = d + [d[7]] * (c - distinct)
    rng.shuffle(v)
    prefix = rng.randrange(1 << pb)
    m = _run_one(k, pb, [(prefix, v)], f"retry, c = {c}, {distinct} distinct")
    assert bs.table(m) == {prefix: (distinct, bs.TRIE)}


# ---- c. wide elements ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,repeat", [(1025, False), (1300, False), (1300, True), (2049, False), (2049, True)])
def test_wide_elements(c, repeat):
    """K = 59: two-word suffixes in 16-byte elements; c distinct words, or c - 1 and one adjacent repeat."""
    k, pb = WIDE
    sb = _sb(k, pb)
    assert sb > 64 and sb + bs.PK_BITS <= bs.MSD_MAX_BITS
    rng = random.Random(f"wide {c} {repeat}")
    v = _distinct(rng, c - repeat, sb)
    if repeat:
        v.insert(c // 2, v[c // 2])
    prefix = rng.randrange(1 << pb)
    m = _run_one(k, pb, [(prefix, v)], f"wide, c = {c}, repeat = {repeat}")
    assert bs.table(m) == {prefix: (c - repeat, bs.TRIE)}


# ---- d. `|=` ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("union_env", [None, "0"])
@pytest.mark.parametrize("kinds", ["trie", "vec"])
@pytest.mark.parametrize("c", [1300, 3000])
def test_merge_of_both_sided_buckets(c, kinds, union_env, monkeypatch):
    """`a |= b` on one shared prefix of cs + co = c words, a tenth of them on both sides: Trie |= Trie (by the merge path, and through the length
    classes with CBLX_MERGE_UNION=0) and Vec |= Vec (Vecs of more than 1024 words at c = 3000, as `|=` leaves them), against PyCBL.merge."""
    _need_gpu()
    if union_env is None:
        monkeypatch.delenv("CBLX_MERGE_UNION", raising=False)
    else:
        monkeypatch.setenv("CBLX_MERGE_UNION", union_env)
    k, pb = PACKED
    sb = _sb(k, pb)
    rng = random.Random(f"merge {c} {kinds}")
    cs = c // 2
    co = c - cs
    shared = c // 10
    pool = _distinct(rng, c - shared, sb)
    mk = "trie" if kinds == "trie" else ("vec" if cs <= bs.THRESHOLD else "lvec")
    prefix = rng.randrange(1 << pb)
    a = {prefix: bs._store(rng, mk, pool[:cs])}
    b = {prefix: bs._store(rng, mk, pool[cs - shared:])}
    assert len(a[prefix][1]) == cs and len(b[prefix][1]) == co
    ma, mb = bs.model_of(a, k, pb), bs.model_of(b, k, pb)
    ga, gb = cbl_amd.CBL(k, pb), cbl_amd.CBL(k, pb)
    ga.load(bs.serialize(ma))
    gb.load(bs.serialize(mb))
    ga |= gb
    ma.merge(mb)
    what = f"{kinds} |= {kinds}, c = {c}, CBLX_MERGE_UNION={union_env}"
    _same(ga, ma, what + ": self")
    _same(gb, mb, what + ": other")
    assert ma.count() == c - shared
    ga.close()
    gb.close()
