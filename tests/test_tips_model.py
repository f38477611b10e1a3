"""Tip clipping on the CPU: the ends of tests/tips_model.py against the link table of gfa_model.definition_model (no shared code path), the marks, and
clip_model's rounds on the crafted read sets of the GPU tests, on crafted sets of tests/biunitigs_model.py and on random sets, in both forms; and what the
case list must hold."""
import random

import numpy as np
import pytest

import cbl_amd
from oracle import Oracle

import biunitigs_model as bm
import gfa_model as gm
import neighbors_model as nm
import removal_model as rm
import tips_model as tm

FORMS = (True, False)  # canonical (bidirected unitigs), non-canonical (plain unitigs)
OLD = ["dense", "branch", "graph15", "cycles", "hairpin", "homopolymers", "at"]  # of biunitigs_model.crafted, at max_kmers = K - 1


def _check_marks(kmers, k, canonical, max_kmers):
    """The ends against the link counts of the definition; no circular unitig is marked; CBL.tip_kinds restates the rule. Returns the marks."""
    marks = tm.marks_of_set(kmers, k, canonical, max_kmers)
    t, left, right, kind = marks["table"], marks["left"], marks["right"], marks["kind"]
    lt = gm.definition_model(kmers, k, canonical, t)
    start = lt["link_start"].astype(np.int64)
    nu = len(t["head"])
    assert np.array_equal(right, (start[1::2] - start[0:-1:2]).astype(np.uint8))
    if canonical:
        assert np.array_equal(left, (start[2::2] - start[1::2]).astype(np.uint8))
    else:
        assert np.array_equal(left, np.bincount(lt["link_to"].astype(np.int64), minlength=nu).astype(np.uint8))
        assert not (start[2::2] - start[1::2]).any()
    circular = (t["flags"] & 1).astype(bool)
    assert (left[circular] >= 1).all() and (right[circular] >= 1).all() and not kind[circular].any()
    assert np.array_equal(cbl_amd.CBL.tip_kinds(t["length"], t["flags"], left, right, max_kmers), kind)
    c = marks["counts"]
    assert c == (int((kind == 1).sum()), int(t["length"][kind == 1].sum()), int((kind == 2).sum()), int(t["length"][kind == 2].sum()))
    return marks


def _check_clip(m, max_kmers, isolated, rounds):
    """clip_model on a copy of m: every round removes exactly the selected k-mers, the stats add up, a fixpoint holds no tip. Returns (index, stats)."""
    k, canonical = m.P["K"], m.canonical
    mm, trace = rm.copy_cbl(m), []
    st = tm.clip_model(mm, max_kmers, isolated, rounds, trace)
    assert st["rounds"] == len(trace) and (rounds == 0 or st["rounds"] <= rounds) and st["kmers_left"] == mm.count()
    for r, (kmers, sel, marks) in enumerate(trace):
        after = trace[r + 1][0] if r + 1 < len(trace) else [tm.kmer_of_word(w, mm.P) for w in tm.iteration_words(mm)]
        assert len(set(after)) == len(after) and set(after) == {x for x, f in zip(kmers, sel.tolist()) if not f}
        assert sel.any() or r + 1 == len(trace)
    removing = sum(1 for _, sel, _ in trace if sel.any())
    assert st["tip_kmers"] + st["isolated_kmers"] == m.count() - mm.count() and st["fixpoint"] == (removing < len(trace))
    if st["fixpoint"]:
        left = _check_marks([tm.kmer_of_word(w, mm.P) for w in tm.iteration_words(mm)], k, canonical, max_kmers)
        assert not (left["kind"] == 1).any() and not (isolated and (left["kind"] == 2).any())
    return mm, st, removing


_done = {}


def _case(name, canonical):
    """(k, max_kmers, the model index, its k-mers in iteration order) of a crafted case, built through the oracle."""
    key = (name, canonical)
    if key not in _done:
        if name in tm.CRAFTED:
            k, pb, flushes, mk = tm.crafted(name)
        else:
            k, pb, flushes = bm.crafted(name)
            mk = k - 1
        o = Oracle(k, pb, canonical)
        for batch in flushes:
            o.insert_seqs(*nm.Graph.arrays(batch))
        words = o.iter_words()
        m = tm.model_of_words(k, pb, canonical, words)
        assert m.serialize() == o.serialize() and tm.iteration_words(m) == words
        kmers = [tm.kmer_of_word(w, m.P) for w in words]
        assert kmers == nm.oracle_kmers(o) and all(tm.word_of_kmer(x, m.P) == w for x, w in list(zip(kmers, words))[:64])
        _done[key] = (k, mk, m, kmers)
    return _done[key]


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_random_sets(k, canonical):
    rng = random.Random(200 * k + canonical)
    space = 1 << (2 * k)
    pool = [x for x in range(space) if bm.is_fwd(x)] if canonical else list(range(space))
    P = tm.PyCBL(k, 4, canonical).P
    marked = 0
    for trial in range(40):
        held = rng.sample(pool, rng.randrange(1, min(len(pool), 200) + 1))
        m = tm.model_of_words(k, 4, canonical, sorted(tm.word_of_kmer(x, P) for x in held))
        kmers = [tm.kmer_of_word(w, P) for w in tm.iteration_words(m)]
        assert sorted(kmers) == sorted(held)
        mk = rng.randrange(1, 6)
        marked += int(_check_marks(kmers, k, canonical, mk)["kind"].astype(bool).sum())
        _check_clip(m, mk, bool(trial & 1), (1, 2, 0)[trial % 3])
    assert marked > 0
    assert _check_marks([], k, canonical, 3)["counts"] == (0, 0, 0, 0)
    st = tm.clip_model(tm.PyCBL(k, 4, canonical), 3, True, 0)
    assert (st["rounds"], st["fixpoint"], st["kmers_left"]) == (1, 1, 0)


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", tm.CRAFTED + OLD)
def test_crafted_sets(name, canonical):
    k, mk, m, kmers = _case(name, canonical)
    _check_marks(kmers, k, canonical, mk)
    if name == "dense":  # two removing rounds in the plain form, one in the bidirected one
        mm, st, removing = _check_clip(m, mk, False, 0)
        assert (m.count(), removing, st["kmers_left"], st["fixpoint"]) == ((36292, 1, 36064, 1) if canonical else (39344, 2, 38662, 1))
        if not canonical:
            assert _check_clip(m, mk, False, 1)[1]["kmers_left"] == 38667
        return
    for isolated in (False, True):
        for rounds in (1, 2, 0):
            _check_clip(m, mk, isolated, rounds)


def _first_round(name, canonical):
    k, mk, m, kmers = _case(name, canonical)
    return tm.features(kmers, tm.marks_of_set(kmers, k, canonical, mk), canonical)


def test_the_case_list_holds_every_kind_of_tip():
    feats = {(name, canonical): _first_round(name, canonical) for name in tm.CRAFTED for canonical in FORMS}
    for canonical in FORMS:  # a tip that is dead on the left and one that is dead on the right; an isolated unitig
        assert any(f["left_dead"] for (_, c), f in feats.items() if c == canonical) and any(f["right_dead"] for (_, c), f in feats.items() if c == canonical)
        assert feats[("islands", canonical)]["isolated"] and feats[("deep", canonical)]["isolated"]
    assert any(f["reversed_end"] for (_, c), f in feats.items() if c) and not any(f["reversed_end"] for (_, c), f in feats.items() if not c)
    assert feats[("edge", True)]["reversed_end"]
    for name in ("edge", "edge15", "edge33", "edge59"):  # a tip at the threshold; the branches one k-mer over it stay
        for canonical in FORMS:
            k, mk, m, kmers = _case(name, canonical)
            marks = tm.marks_of_set(kmers, k, canonical, mk)
            ln, kind = marks["table"]["length"], marks["kind"]
            dead = (marks["left"] == 0) != (marks["right"] == 0)
            assert sorted(ln[kind == 1].tolist()) == [mk, mk] and ln[(ln == mk + 1) & dead].tolist() == [mk + 1, mk + 1] and not kind[ln == mk + 1].any()
    for canonical in FORMS:
        # the cascade: rounds = 1, 2 and 0 leave three different indexes, with rounds / fixpoint 1 / 0, 2 / 0 and 3 / 1
        k, mk, m, _ = _case("cascade", canonical)
        res = [_check_clip(m, mk, False, r) for r in (1, 2, 0)]
        assert [(st["rounds"], st["fixpoint"]) for _, st, _ in res] == [(1, 0), (2, 0), (3, 1)]
        blobs = [mm.serialize() for mm, _, _ in res]  # round 3 removes nothing: the third index is the second, the stats tell the calls apart
        assert blobs[0] != blobs[1] and blobs[1] == blobs[2] and m.serialize() not in blobs and [st["tips"] for _, st, _ in res] == [2, 3, 3]
        # the fork empties in one round: the stem is a tip too
        k, mk, m, _ = _case("fork", canonical)
        mm, st, _ = _check_clip(m, mk, False, 1)
        assert st["tips"] == 3 and mm.count() == 0 and mm.buckets == {} and mm.serialize() == tm.PyCBL(k, 24, canonical).serialize()
        # islands: the path of max_kmers k-mers is isolated, the one of max_kmers + 1 is not marked; neither the cycle nor poly-A ever is
        k, mk, m, kmers = _case("islands", canonical)
        marks = tm.marks_of_set(kmers, k, canonical, mk)
        t, kind = marks["table"], marks["kind"]
        assert t["length"][kind == 2].tolist() == [mk] and (mk + 1) in t["length"][kind == 0].tolist()
        poly_a = t["unitig"][kmers.index(0)] if 0 in kmers else t["unitig"][kmers.index(bm.rc(0, k))]
        assert t["length"][poly_a] == 1 and kind[poly_a] == 0 and (marks["left"][poly_a], marks["right"][poly_a]) == (1, 1)
        assert (t["flags"][poly_a] & 1) == (0 if canonical else 1)
        assert ((t["flags"] & 1) & (t["length"] == 7)).any()
    # canonical islands: the hairpin unitig has one dead end and one end linked to itself alone — a tip, not an isolated unitig
    k, mk, m, kmers = _case("islands", True)
    marks = tm.marks_of_set(kmers, k, True, mk)
    t = marks["table"]
    pairs = gm.slot_pairs(gm.definition_model(kmers, k, True, t))
    hp = [a >> 1 for a, b in pairs if b == a ^ 1]
    assert len(hp) == 1 and marks["kind"][hp[0]] == 1 and sorted((int(marks["left"][hp[0]]), int(marks["right"][hp[0]]))) == [0, 1]
    assert t["length"][hp[0]] == (k + 1) // 2
    # deep: buckets of many words, one of them emptied by the isolated path
    for canonical in FORMS:
        k, mk, m, _ = _case("deep", canonical)
        assert max(len(b[1]) for b in m.buckets.values()) >= 100
        assert len(_check_clip(m, mk, True, 1)[0].buckets) < len(m.buckets)
