"""Links between unitigs and the GFA text on the CPU: the definition of tests/gfa_model.py (every edge of the set, classified against the walk's table)
against the restatement of the device's route, on random sets and on every crafted input of the GPU tests in both forms; the identities of the link
set; the text and its way back to the edge set; and what the case list must hold."""
import random

import numpy as np
import pytest

from oracle import Oracle

import biunitigs_model as bm
import gfa_model as gm
import neighbors_model as nm

FORMS = (True, False)  # canonical (bidirected unitigs), non-canonical (plain unitigs)


def _check(kmers, k, canonical):
    """Definition = route, the identities, the text and its way back. Returns (table, link table, text)."""
    t = gm.walk_model(kmers, k, canonical)
    masks = gm.masks_of_set(kmers, k, canonical)
    lt = gm.definition_model(kmers, k, canonical, t)  # asserts tail -> head, and that no two links share both end slots
    route = gm.route_model(kmers, k, canonical, t, masks)
    assert gm.same_links(lt, route), "the route's restatement differs from the definition"
    n, nu, nl = len(kmers), len(t["head"]), lt["n_links"]
    pairs = gm.slot_pairs(lt)
    if canonical:
        e2 = sum(bin(int(m)).count("1") for m in masks)
        assert nl == e2 - 2 * n + 2 * nu
        held = set(pairs)
        assert all((b ^ 1, a ^ 1) in held for a, b in pairs)  # mirror closure
        self_mirror = sum(1 for a, b in pairs if b == a ^ 1)
        assert 2 * gm.n_l_lines(lt, True) == nl + self_mirror
    else:
        e = sum(bin(int(m) & 15).count("1") for m in masks)
        assert nl == e - n + nu
        assert all(a % 2 == 0 and b % 2 == 0 for a, b in pairs) and gm.n_l_lines(lt, False) == nl
    for u in np.flatnonzero(t["flags"] & 1).tolist():  # a circular unitig: its cut edge is the self link u+ -> u+, and u- -> u- of its mirror
        assert (2 * u, 2 * u) in pairs and (not canonical or (2 * u + 1, 2 * u + 1) in pairs)
    text = gm.gfa_model(kmers, k, canonical, t, lt)
    assert text.count(b"\nS\t") == nu and text.count(b"\nL\t") == gm.n_l_lines(lt, canonical)
    assert gm.k1mers_of_gfa(text, k, canonical) == gm.k1mers_of_set(kmers, k, canonical)  # the text spells the edge set of S, nothing else
    return t, lt, text


def _oracle_order(k, pb, flushes, canonical):
    o = Oracle(k, pb, canonical)
    for batch in flushes:
        o.insert_seqs(*nm.Graph.arrays(batch))
    return nm.oracle_kmers(o)


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_definition_equals_route_on_random_sets(k, canonical):
    """Random sets of every density (a shuffled list is the iteration order, at K = 5 and 7 every other one is the oracle's), and sets made of cycles."""
    rng = random.Random(100 * k + canonical)
    space = 1 << (2 * k)
    pool = [x for x in range(space) if bm.is_fwd(x)] if canonical else list(range(space))
    for trial in range(60):
        kmers = rng.sample(pool, rng.randrange(1, min(len(pool), 300) + 1))
        if k >= 5 and trial % 2 == 0:
            order = _oracle_order(k, 4, [[nm.unpack(x, k).encode() for x in kmers]], canonical)
            assert sorted(order) == sorted(kmers)
            kmers = order
        _check(kmers, k, canonical)
    circular = 0
    for trial in range(40):
        held = set()
        for _ in range(rng.randrange(1, 4)):
            s = nm._rand(rng, rng.randrange(1, 20))
            r = s * (k // len(s) + 2)
            words = [nm.pack(r[i: i + k]) for i in range(len(s))]
            held |= {bm.canon(x, k)[0] for x in words} if canonical else set(words)
        kmers = list(held)
        rng.shuffle(kmers)
        circular += _check(kmers, k, canonical)[0]["n_circular"]
    assert circular > 0 or (canonical and k == 3)
    t, lt, text = _check([], k, canonical)
    assert lt["n_links"] == 0 and lt["link_start"].tolist() == [0] and text == gm.HEADER and len(text) == 11


_done = {}


def _crafted(name, canonical):
    key = (name, canonical)
    if key not in _done:
        k, pb, flushes = bm.crafted(name)
        kmers = _oracle_order(k, pb, flushes, canonical)
        _done[key] = (k, kmers) + _check(kmers, k, canonical)
    return _done[key]


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", bm.CRAFTED)
def test_definition_equals_route_on_crafted_sets(name, canonical):
    k, kmers, t, lt, text = _crafted(name, canonical)
    if name == "hairpin" and canonical:
        assert lt["n_links"] == 1
    if name == "dense":
        assert (len(kmers), lt["n_unitigs"], lt["n_links"]) == ((36292, 24551, 103027) if canonical else (39344, 16927, 32406))


def _pairs(name, canonical):
    return gm.slot_pairs(_crafted(name, canonical)[3])


def test_the_case_list_holds_every_kind_of_link():
    # cross-unitig links of all four sign kinds
    kinds = {(a & 1, b & 1) for a, b in _pairs("graph15", True) if a >> 1 != b >> 1}
    assert kinds == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # a circular self link: the cut edge of a circular unitig of length >= 2, in both forms
    for canonical in FORMS:
        t = _crafted("cycles", canonical)[2]
        circ = np.flatnonzero((t["flags"] & 1) & (t["length"] >= 2)).tolist()
        assert circ and all((2 * u, 2 * u) in _pairs("cycles", canonical) for u in circ)
    # a link that is its own mirror, and it is the only link of the hairpin
    assert [b == a ^ 1 for a, b in _pairs("hairpin", True)] == [True]
    # u+ -> u- and u- -> u+ of one unitig
    at = _pairs("at", True)
    assert (0, 1) in at and (1, 0) in at
    # homopolymer self-loops are links of unitigs that are not circular (bidirected), and the cut edge of a circular unitig of length 1 (plain)
    t = _crafted("homopolymers", True)[2]
    assert t["n_circular"] == 0 and all(any(a >> 1 == u and b >> 1 == u for a, b in _pairs("homopolymers", True)) for u in range(len(t["head"])))
    tp = _crafted("homopolymers", False)[2]
    assert len(tp["head"]) == 4 and sorted(_pairs("homopolymers", False)) == [(2 * u, 2 * u) for u in range(4)]
    # a slot with 4 links and one with 0, in both forms
    for canonical in FORMS:
        per_slot = set()
        for name in bm.CRAFTED:
            start = _crafted(name, canonical)[3]["link_start"].astype(np.int64)
            per_slot |= set(np.diff(start)[:: 1 if canonical else 2].tolist())
        assert {0, 4} <= per_slot, (canonical, per_slot)
    # unitig numbers of 1 to 5 digits on both ends of L lines, and more than 100 000 links
    for canonical in FORMS:
        lt, text = _crafted("dense", canonical)[3:]
        assert lt["n_unitigs"] > 10000 and (lt["n_links"] > 100000 or not canonical)
        rows = [r.split(b"\t") for r in text.split(b"\n") if r.startswith(b"L")]
        assert {len(r[1]) for r in rows} == {1, 2, 3, 4, 5} and {len(r[3]) for r in rows} == {1, 2, 3, 4, 5}


def test_link_tuples_of_the_python_surface():
    """CBL.gfa_link_tuples is host-only: on the model's table it names the slots as the text does."""
    import cbl_amd

    for canonical in FORMS:
        k, kmers, t, lt, text = _crafted("graph15", canonical)
        tuples = list(cbl_amd.CBL.gfa_link_tuples(lt["link_start"], lt["link_to"], lt["link_rev"]))
        assert tuples == [(a >> 1, "+-"[a & 1], b >> 1, "+-"[b & 1]) for a, b in gm.slot_pairs(lt)]
        kept = [b"L\t%d\t%s\t%d\t%s\t%dM" % (u, a.encode(), v, b.encode(), k - 1) for (u, a, v, b), p in zip(tuples, gm.slot_pairs(lt)) if gm.written(p, canonical)]
        assert kept == [r for r in text.split(b"\n") if r.startswith(b"L")]
