"""tests/removal_model.py against itself and against the reference's own removal tests (no GPU): the literal replay of `TrieVec::remove` / `remove_batch` /
`remove_seq` against the closed forms the device path computes, and the command line's `remove` subcommand."""
import itertools
import random
import subprocess
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
ROOT = Path(__file__).resolve().parent.parent

from oracle.pyref import THRESHOLD, PyCBL, seq_words  # noqa: E402

import removal_model as rm  # noqa: E402  (tests/)
import setops_model as sm  # noqa: E402  (tests/)

K, PB = 11, 6  # SUFFIX_BITS 21
SB = 21


def _both(buckets, batches, canonical=False):
    """the literal replay and the closed form on copies of one crafted index; returns the model after the literal replay"""
    a = sm.from_buckets(K, PB, canonical, buckets)
    assert a.P["SB"] == SB
    b = rm.copy_cbl(a)
    before = sm.words(a)
    for words in batches:
        rm.remove_batch(a, words)
    rm.remove_batches_closed(b, batches)
    assert a.buckets == b.buckets
    assert a.serialize() == b.serialize()
    assert sm.words(a) == before - {w for ws in batches for w in ws}  # the set is old - removed
    assert all(bk[1] for bk in a.buckets.values())  # no empty bucket stays
    return a


def _w(p, s):
    return (p << SB) | s


# ---------------------------------------------------------------- Vecs of up to 6 words, every removal sequence
@pytest.mark.parametrize("L", range(1, 7))
def test_every_sequence_over_a_small_vec(L):
    items = [7 * i + 3 for i in range(L)]
    alphabet = items + [1]  # one absent word
    longest = L + 1 if L <= 5 else 6
    for n in range(1, longest + 1):
        for seq in itertools.product(alphabet, repeat=n):
            lit = ["vec", list(items)]
            for x in seq:
                rm.trievec_remove(lit, x)
            kind, got = rm.replay_bucket("vec", items, [(o, 1 + o // 2, x) for o, x in enumerate(seq)])  # groups do not matter to a Vec
            assert kind == "vec" and got == lit[1], (items, seq)
    if L == 6:  # the orders that empty it, with one repeat and one absent word somewhere
        for perm in itertools.permutations(items):
            seq = list(perm[:3]) + [perm[0], 1] + list(perm[3:])
            lit = ["vec", list(items)]
            for x in seq:
                rm.trievec_remove(lit, x)
            assert lit[1] == [] and rm.replay_bucket("vec", items, [(o, 1, x) for o, x in enumerate(seq)]) == ("vec", [])


def test_flags_are_the_return_values_of_remove():
    rng = random.Random(5)
    for _ in range(50):
        items = sm.distinct(rng, rng.randint(1, 40), 8)
        kind = rng.choice(["vec", "trie"])
        a = sm.from_buckets(K, PB, False, {3: (kind, sorted(items) if kind == "trie" else items)})
        b = rm.copy_cbl(a)
        words = [_w(rng.choice([3, 4]), rng.getrandbits(8)) for _ in range(120)]
        want = [rm.remove_word(a, w) for w in words]
        got = rm.remove_batches_closed(b, [[w] for w in words])  # every call a group of its own
        assert got == want and a.buckets == b.buckets


# ---------------------------------------------------------------- random sequences, several buckets, several batches
@pytest.mark.parametrize("seed", range(12))
def test_random_sequences(seed):
    rng = random.Random(seed)
    buckets = {}
    for p in rng.sample(range(1 << PB), 5):
        n = rng.choice([1, 5, 60, 1000, 1024, 1025, 1030, 1300, 2100])
        items = sm.distinct(rng, n, 12)  # a small universe: the batches hit often
        kind = rng.choice(["vec", "trie"])
        buckets[p] = (kind, sorted(items) if kind == "trie" else items)
    prefixes = list(buckets) + [p for p in range(1 << PB) if p not in buckets][:2]
    batches = []
    for _ in range(rng.randint(1, 4)):
        words = []
        while len(words) < rng.randint(1, 1500):
            p = rng.choice(prefixes)
            words += [_w(p, rng.getrandbits(12)) for _ in range(rng.choice([1, 2, 30, 400]))]  # runs of one prefix: groups
        batches.append(words[:1500])
    _both(buckets, batches)


# ---------------------------------------------------------------- the conversion of a Trie
def _trie(n, rng):
    return sorted(sm.distinct(rng, n, SB))


def test_trie_of_1026_words_in_one_or_two_groups():
    rng = random.Random(1)
    items = _trie(1026, rng)
    x1, x2, x3 = items[10], items[500], items[700]
    p, q = 5, 9
    two = _both({p: ("trie", items), q: ("vec", [1])}, [[_w(p, x1), _w(p, x2), _w(q, 77), _w(p, x3)]])
    one = _both({p: ("trie", items), q: ("vec", [1])}, [[_w(p, x1), _w(p, x2), _w(p, x3)]])
    rest = [x for x in items if x not in (x1, x2)]
    swapped = list(rest)
    swapped[swapped.index(x3)] = swapped[-1]
    swapped.pop()
    assert two.buckets[p] == ["vec", swapped]  # the ascending 1024 with the last word in x3's slot
    assert one.buckets[p] == ["vec", [x for x in rest if x != x3]]  # the ascending 1023
    assert two.buckets[p] != one.buckets[p]


def test_tries_that_stay_and_tries_that_shrink():
    rng = random.Random(2)
    items = _trie(1026, rng)
    p, q = 5, 9
    assert _both({p: ("trie", items)}, [[_w(p, items[3])]]).buckets[p][0] == "trie"  # 1025 left
    t1025 = items[:1025]
    absent = [x for x in range(50) if x not in t1025][:4]
    assert _both({p: ("trie", t1025)}, [[_w(p, a) for a in absent]]).buckets[p] == ["trie", t1025]
    for n in (1024, 5):  # short Tries (the assigning set operations leave them) shrink at the first group that visits them, hit or no hit
        m = _both({p: ("trie", items[:n]), q: ("trie", items[:n])}, [[_w(p, absent[0])]])
        assert m.buckets[p] == ["vec", items[:n]] and m.buckets[q] == ["trie", items[:n]]
    long_vec = items[::-1]
    assert _both({p: ("vec", long_vec)}, [[_w(p, absent[0])]]).buckets[p] == ["vec", long_vec]  # a Vec longer than 1024 stays a Vec


def test_trie_of_5000_words():
    rng = random.Random(3)
    items = _trie(5000, rng)
    order = list(items)
    rng.shuffle(order)
    p, q = 2, 3
    first, then = [_w(p, x) for x in order[:3976]], [_w(p, x) for x in order[3976:3986]]
    a = _both({p: ("trie", items)}, [first + [_w(q, 0)] + then])  # two groups of one call
    b = _both({p: ("trie", items)}, [first, then])  # two calls
    assert a.buckets == b.buckets and a.buckets[p][0] == "vec" and len(a.buckets[p][1]) == 1014
    assert a.buckets[p][1] != sorted(a.buckets[p][1])  # the ten later removals swapped
    c = _both({p: ("trie", items)}, [[_w(p, x) for x in order[:4000]]])
    assert c.buckets[p] == ["vec", sorted(order[4000:])]
    assert _both({p: ("trie", items)}, [[_w(p, x) for x in order]]).buckets == {}
    # converts in the first of three groups, the next two swap_remove from the new Vec
    d = _both({p: ("trie", items)}, [first + [_w(q, 0)] + then[:5] + [_w(q, 0)] + then[5:]])
    assert d.buckets == a.buckets


# ---------------------------------------------------------------- the reference's own tests (src/cbl.rs:664-683, 726-760)
def _random_seq(rng, n):
    return bytes(rng.choice(b"ACGT") for _ in range(n))


@pytest.mark.parametrize("canonical", [False, True])
def test_batch_operations(canonical):
    rng = random.Random(9)
    seq = _random_seq(rng, 6000)  # three chunks
    c = PyCBL(K, PB, canonical)
    c.insert_seq(seq)
    words = set(seq_words(seq, c.P, canonical))
    assert sm.words(c) == words and any(b[0] == "trie" for b in c.buckets.values())
    d = rm.copy_cbl(c)
    rm.remove_seq(c, seq)
    assert c.buckets == {} and c.count() == 0 and c.serialize() == PyCBL(K, PB, canonical).serialize()
    rm.remove_batches_closed(d, rm.seq_batches(d, seq))
    assert d.buckets == {}


@pytest.mark.parametrize("canonical", [False, True])
def test_remove_seq_of_half_the_reads(canonical):
    rng = random.Random(10)
    seqs = [_random_seq(rng, 2500) for _ in range(6)]
    c = PyCBL(K, PB, canonical)
    for s in seqs:
        c.insert_seq(s)
    d = rm.copy_cbl(c)
    for s in seqs[3:]:
        rm.remove_seq(c, s)
    rm.remove_batches_closed(d, [b for s in seqs[3:] for b in rm.seq_batches(d, s)])
    assert c.buckets == d.buckets
    gone = {w for s in seqs[3:] for w in seq_words(s, c.P, canonical)}
    assert sm.words(c) == {w for s in seqs[:3] for w in seq_words(s, c.P, canonical)} - gone
    with pytest.raises(ValueError):
        rm.remove_seq(c, b"ACGT")


# ---------------------------------------------------------------- the command line
def test_cli_remove_parses():
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "remove", "--help"], cwd=str(ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "index" in r.stdout and "input" in r.stdout and "--output" in r.stdout


def test_threshold_is_the_reference_value():
    assert THRESHOLD == 1024
