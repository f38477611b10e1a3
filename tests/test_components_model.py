"""Connected components on the CPU: the definition of tests/components_model.py (a union-find on the k-mers) against the route the device takes (the link
table, hook and compress), the identities of every table, filter_model, and what the case list must hold; on the crafted read sets of the GPU tests and on
random sets, in both forms."""
import random

import numpy as np
import pytest

import biunitigs_model as bm
import components_model as cm
import gfa_model as gm
import neighbors_model as nm
import removal_model as rm
import tips_model as tm

FORMS = (True, False)  # canonical (bidirected unitigs), non-canonical (plain unitigs)

_done = {}


def _case(name, canonical):
    """(k, the model index, its k-mers in iteration order, the walk's table, the link table, the route's table) of a crafted case."""
    key = (name, canonical)
    if key not in _done:
        k, pb, flushes = cm.crafted(name)
        _, m, kmers = cm.build_case(k, pb, canonical, flushes)
        t = gm.walk_model(kmers, k, canonical)
        lt = gm.definition_model(kmers, k, canonical, t)
        _done[key] = (k, m, kmers, t, lt, cm.route_model(kmers, k, canonical, t, lt))
    return _done[key]


def _check(kmers, k, canonical, t=None, lt=None, table=None):
    t = gm.walk_model(kmers, k, canonical) if t is None else t
    lt = gm.definition_model(kmers, k, canonical, t) if lt is None else lt
    table = cm.route_model(kmers, k, canonical, t, lt) if table is None else table
    want = cm.definition_model(kmers, k, canonical, t, lt)
    assert cm.same_table(table, want, rounds=False)  # definition = route
    cm.check_identities(table, lt)
    assert (table["rounds"] == 0) == (len(kmers) == 0) and table["rounds"] < cm.MAX_ROUNDS
    return table


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", cm.CRAFTED + cm.OLD)
def test_definition_equals_route_on_crafted_cases(name, canonical):
    k, m, kmers, t, lt, table = _case(name, canonical)
    _check(kmers, k, canonical, t, lt, table)
    if name == "comb":  # a chain of unitigs at least 2 000 long in one component: a rule that walks the diameter would show here
        assert table["components"] == 1 and table["unitigs_n"] >= 4000 and table["rounds"] <= 32, table["rounds"]
    if name == "strands":
        assert table["components"] == (1 if canonical else 2)
    if name in ("arch64", "arch256", "arch257"):
        assert table["unitigs_n"] == table["components"] == int(name[4:])
    if name == "one":
        assert cm.counts_of(table) == (1, 1, 0, 1, 1, 1)
    if name == "empty":
        assert cm.counts_of(table) == (0, 0, 0, 0, 0, 0) and all(len(table[key]) == 0 for key in cm.ARRAYS)


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("k", (3, 5, 7))
def test_definition_equals_route_on_random_sets(k, canonical):
    rng = random.Random(100 * k + canonical)
    for trial in range(30 if k < 7 else 12):
        space = 4 ** k
        want = rng.choice((1, 2, space // 8, space // 3, space // 2)) if k < 7 else rng.choice((40, 400, 2500))
        xs = {rng.randrange(space) for _ in range(max(1, want))}
        kmers = sorted({bm.canon(x, k)[0] for x in xs}) if canonical else sorted(xs)
        rng.shuffle(kmers)
        _check(kmers, k, canonical)


def test_the_case_list_holds_every_feature():
    seen = {}
    for name in cm.CRAFTED + cm.OLD:
        for canonical in FORMS:
            k, m, kmers, t, lt, table = _case(name, canonical)
            seen[(name, canonical)] = cm.features(table, lt)
    assert any(f["single_with_self_link"] for f in seen.values())  # a component of one unitig with a self link
    assert any(f["slot_of_4"] for f in seen.values())  # a slot of 4 links
    assert any(f["one_component"] for f in seen.values()) and any(f["all_singletons"] for f in seen.values())  # C = 1 and C = U
    views = set().union(*(f["views"] for f in seen.values()))
    assert {1, 2, 64} <= views, views  # what a wave of k_cc_sizes sees
    assert 1 in seen[("comb", False)]["views"] and 64 in seen[("arch257", True)]["views"]
    for name in ("arch15", "arch31"):
        for canonical in FORMS:
            k, m, kmers, t, lt, table = _case(name, canonical)
            mk, sizes = cm.MIN_KMERS[name], table["kmers"].tolist()
            assert {mk - 1, mk, mk + 1} <= set(sizes) and sizes.count(max(sizes)) == 2 and max(sizes) == 12 * mk  # the edges of the filter; two equal largest
            assert table["unitigs_n"] > 257 and (table["unitigs"] > 1).any() and len(set(cm.wave_views(table))) > 1


def test_a_hairpin_alone_holds_a_component_together():
    """u + rc(u) in the non-canonical form: the two strands are one component through the K - 1 k-mers across the junction, and two without them."""
    k = 31
    read = bm.hairpin_reads(k)[0].decode()
    half = len(read) // 2
    def packed(s):
        return [nm.pack(s[i: i + k]) for i in range(len(s) - k + 1)]
    whole = list(dict.fromkeys(packed(read)))
    halves = list(dict.fromkeys(packed(read[:half]) + packed(read[half:])))
    assert len(whole) == len(halves) + k - 1
    assert _check(whole, k, False)["components"] == 1 and _check(halves, k, False)["components"] == 2
    both = sorted({bm.canon(x, k)[0] for x in whole})
    table = _check(both, k, True)  # the canonical form: one unitig whose one end links to itself
    assert table["components"] == 1 and cm.features(table, gm.definition_model(both, k, True))["single_with_self_link"]


def _filter(m, **rule):
    mm, trace = rm.copy_cbl(m), []
    st = cm.filter_model(mm, trace=trace, **rule)
    kmers, table, sel = trace[0]
    after = [tm.kmer_of_word(w, mm.P) for w in tm.iteration_words(mm)]
    assert set(after) == {x for x, f in zip(kmers, sel.tolist()) if not f} and len(after) == st["kmers_left"] == len(kmers) - st["removed_kmers"]
    drop = cm.dropped(table, **rule)
    left = _check(after, m.P["K"], m.canonical)
    assert sorted(left["kmers"].tolist()) == sorted(table["kmers"][~drop].tolist())  # the multiset of component sizes is the kept one
    assert st["components"] == table["components"] and st["removed_components"] == int(drop.sum()) and st["largest_kmers"] == table["largest_kmers"]
    return mm, st, table


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", ["arch15", "arch31", "strands", "islands", "branch", "one", "empty"])
def test_filter_model(name, canonical):
    k, m, kmers, t, lt, table = _case(name, canonical)
    blob = m.serialize()
    mm, st, _ = _filter(m, min_kmers=1)  # the identity
    assert mm.serialize() == blob and st["removed_kmers"] == 0 and st["kmers_left"] == len(kmers)
    mm, st, _ = _filter(m, min_kmers=table["largest_kmers"] + 1)  # above the largest component: nothing is left
    assert mm.count() == 0 and not mm.buckets and st["removed_components"] == table["components"]
    mm, st, _ = _filter(m, largest=True)
    assert st["kmers_left"] == table["largest_kmers"] and st["removed_components"] == max(table["components"] - 1, 0)
    if table["components"]:
        kept = {x for x, c in zip(kmers, table["kmer_component"].tolist()) if c == cm.largest_of(table)}
        assert {tm.kmer_of_word(w, mm.P) for w in tm.iteration_words(mm)} == kept
    if name in cm.MIN_KMERS:
        mk, seen = cm.MIN_KMERS[name], []
        assert cm.largest_of(table) == int(np.flatnonzero(table["kmers"] == table["largest_kmers"])[0])  # the tie: the lower number
        for v in (mk - 1, mk, mk + 1, mk + 2):
            mm, st, _ = _filter(m, min_kmers=v)
            seen.append(st["removed_components"])
            if v == mk:
                assert len(mm.buckets) < len(m.buckets)  # a bucket that the filter empties
        assert seen[0] < seen[1] < seen[2] < seen[3]
        assert _filter(m, min_kmers=int(table["kmers"].min()))[1]["removed_kmers"] == 0
    assert m.serialize() == blob
