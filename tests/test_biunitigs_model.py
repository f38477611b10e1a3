"""Bidirected unitigs on the CPU: the sequential walk of tests/biunitigs_model.py (the definition, degrees counted from the set) against the restatement
of the device's route (links from the neighbour masks, unitigs_model.jump_model on 2 n ids, tails / keep / number) on random canonical sets and on every
crafted input of the GPU tests; the identities of the definition; the text and its way back to the set."""
import random

import numpy as np
import pytest

from oracle import Oracle

import biunitigs_model as bm
import neighbors_model as nm
import unitigs_model as um


def _both(kmers, k, masks=None):
    walk, route = bm.walk_model(kmers, k), bm.route_model(kmers, k, masks)
    assert bm.same_table(walk, route), "the route's restatement differs from the walk"
    assert walk["n_simple"] == route["n_simple"]
    n = len(kmers)
    bm.check_identities(walk, n)  # every ordinal once as (unitig, offset); the lengths add up to n; U = n - L + circular; heads ascend
    bm.check_identities(route, n)
    text = bm.text_model(kmers, walk, k)
    assert sorted(bm.stored_kmers_of_text(text, k)) == sorted(kmers)  # the k-mers of the lines, canonicalised, are exactly S, each once
    return walk, route, text


def _oracle_order(reads, k, pb, flushes=None):
    o = Oracle(k, pb, True)
    for batch in (flushes or [reads]):
        o.insert_seqs(*nm.Graph.arrays(batch))
    return o, nm.oracle_kmers(o)


@pytest.mark.parametrize("k", [3, 5, 7])
def test_walk_equals_route_on_random_canonical_sets(k):
    """Random canonical sets of every density: at K = 3 (below the oracle's smallest K) a shuffled list is the iteration order, at K = 5 and 7 the oracle's
    own order."""
    rng = random.Random(k)
    space = 1 << (2 * k)
    stored = [x for x in range(space) if bm.is_fwd(x)]
    assert len(stored) == space // 2
    for trial in range(60):
        n = rng.randrange(1, min(len(stored), 300) + 1)
        kmers = rng.sample(stored, n)
        if k >= 5 and trial % 2 == 0:
            o, order = _oracle_order([nm.unpack(x, k).encode() for x in kmers], k, 4)
            assert sorted(order) == sorted(kmers)
            masks = bm.masks_of_set(order, k)
            if trial < 4:
                assert np.array_equal(masks, nm.masks_model(o, order, k))  # the masks of the model are section 6j's
            kmers = order
        _both(kmers, k)
    # sets made of cycles: the rotations of random strings in either strand, plus loose k-mers
    circular = 0
    for trial in range(60):
        held = set()
        for _ in range(rng.randrange(1, 4)):
            s = nm._rand(rng, rng.randrange(1, 20))
            r = s * (k // len(s) + 2)
            held |= {bm.canon(nm.pack(r[i: i + k]), k)[0] for i in range(len(s))}
        held |= {bm.canon(rng.getrandbits(2 * k), k)[0] for _ in range(rng.randrange(0, 4))}
        kmers = list(held)
        rng.shuffle(kmers)
        circular += _both(kmers, k)[0]["n_circular"]
    assert circular > 0 or k == 3  # the cycle cut, on a cycle and its mirror, was exercised (at K = 3 a cycle this short meets its own mirror)


CRAFTED, _crafted = bm.CRAFTED, bm.crafted


_seen = {}


@pytest.mark.parametrize("name", CRAFTED)
def test_walk_equals_route_on_crafted_sets(name):
    k, pb, flushes = _crafted(name)
    _, kmers = _oracle_order(None, k, pb, flushes)
    walk, route, text = _both(kmers, k)
    _seen[name] = bm.features(kmers, k, walk)
    lengths = walk["length"].tolist()
    if name.startswith("edges"):
        # every path length is there; the pure cycles stay circular, the cycle with a read running into it comes out linear
        assert all(ln in lengths for ln in um.PATH_LENGTHS)
        assert sorted(walk["length"][walk["flags"] == 1].tolist()) == sorted(um.CYCLE_LENGTHS) and walk["n_circular"] == 3
    if name == "cycles":
        assert sorted(walk["length"][walk["flags"] == 1].tolist()) == [2, 7, 40] and len(lengths) == 3
    if name == "hairpin":
        # u + rc(u): the k-mers of rc(u) are those of u, and the k-mers across the junction pair up with their mirrors: the walk turns round
        assert len(kmers) == (3 * k - k + 1) + (k - 1) // 2 and _seen[name]["hairpin"]
    if name == "strands":
        assert len(lengths) == 1 and lengths[0] == 201 and walk["n_circular"] == 0
    if name == "overlap":
        assert len(lengths) == 1 and lengths[0] == 60 + 2 * k + 60 - k + 1 and _seen[name]["reversed"]
        assert 0 < int(walk["reversed"].sum()) < len(kmers)
    if name == "branch":
        assert sorted(lengths) == [21, 149, 151]
    if name == "homopolymers":
        # poly-A / poly-T and poly-C / poly-G are one stored k-mer each; the loop on itself counts in the degrees and is never simple: not circular
        assert len(kmers) == 2 and lengths == [1, 1] and walk["n_circular"] == 0 and text.count(b"\n") == 2
    if name == "at":
        assert len(kmers) == 1 and lengths == [1] and walk["n_circular"] == 0 and _seen[name]["hairpin"] and _seen[name]["shared"]


def test_the_case_list_covers_what_the_definition_turns_on():
    """The crafted cases hold at least one circular unitig of length >= 2, one hairpin edge, one unitig of length >= 2 with a reversed member, and one stored
    k-mer whose out- and in-nibble name the same stored neighbour."""
    for name in CRAFTED:
        if name not in _seen:
            k, pb, flushes = _crafted(name)
            _, kmers = _oracle_order(None, k, pb, flushes)
            _seen[name] = bm.features(kmers, k, bm.walk_model(kmers, k))
    for what in ("circular", "hairpin", "reversed", "shared"):
        assert any(f[what] for f in _seen.values()), what


def test_long_path_and_edge_cases():
    k = 31
    _, kmers = _oracle_order(um.long_path_reads(k), k, 24)
    walk, route, text = _both(kmers, k)
    assert len(kmers) == 70000 and len(walk["head"]) == 1 and walk["n_circular"] == 0 and len(text) == 70000 + 31
    assert route["rounds"] == 18  # as section 6k: both images are paths of 70 000
    for k in (15, 31, 33):
        walk, _, text = _both([], k)
        assert len(walk["head"]) == 0 and text == b""
        lone = bm.canon(nm.pack(nm._rand(random.Random(k), k)), k)[0]
        walk, _, text = _both([lone], k)
        assert len(walk["head"]) == 1 and walk["n_circular"] == 0 and text == nm.unpack(lone, k).encode() + b"\n" and walk["reversed"].tolist() == [0]
