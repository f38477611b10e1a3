"""Bubble popping on the CPU: the marks of tests/bubbles_model.py against their own definition (every popped arm has a kept sibling, one kept arm per group,
both views of a bidirected group agree), pop_model's rounds and the carry of the counts on the crafted read sets of the GPU tests and on random sets, in
both forms; CBL.bubble_kinds against the model; and what the case list must hold."""
import random

import numpy as np
import pytest

import cbl_amd
from oracle import Oracle

import abundance_model as am
import biunitigs_model as bm
import bubbles_model as bb
import components_model as cm
import gfa_model as gm
import neighbors_model as nm
import removal_model as rm
import tips_model as tm

FORMS = (True, False)  # canonical (bidirected unitigs), non-canonical (plain unitigs)


def _check_marks(kmers, k, canonical, max_kmers, counts=None):
    """The kinds against the definition, read off the arms once more; CBL.bubble_kinds restates the rule. Returns the marks."""
    marks = bb.marks_of_set(kmers, k, canonical, max_kmers, counts)
    t, lt, kind, arms, kc = marks["table"], marks["links"], marks["kind"], marks["arms"], marks["kc"]
    length = t["length"]
    pairs = set(gm.slot_pairs(lt))
    for a, x, tt in arms:  # an arm is what the definition says, and in the bidirected form its other image is an arm of the mirror view
        assert (a, x) in pairs and (x, tt) in pairs and int(length[x >> 1]) <= max_kmers and x >> 1 not in (a >> 1, tt >> 1)
        assert sum(1 for p in pairs if p[1] == x) == 1 and sum(1 for p in pairs if p[0] == x) == 1
        assert not canonical or (tt ^ 1, x ^ 1, a ^ 1) in arms
    of_unitig = {}
    for a, x, tt in arms:
        of_unitig.setdefault(x >> 1, set()).add(frozenset({(a, tt), (tt ^ 1, a ^ 1)}) if canonical else frozenset({(a, tt)}))
    assert all(len(g) == 1 for g in of_unitig.values())  # an arm is in exactly one group
    live = [mem for mem in marks["groups"].values() if len(mem) >= 2]
    assert all(len(mem) <= 4 for mem in marks["groups"].values())
    assert int((kind == 2).sum()) == len(live) == marks["counts"][0]  # kept = groups
    for mem in live:
        kept = [u for u in mem if kind[u] == 2]
        assert len(kept) == 1 and all(kind[u] == 1 for u in mem if u != kept[0])  # every popped arm has a kept sibling with the same source and target
        assert all(bb.above(kept[0], u, length, kc) for u in mem if u != kept[0])
    assert set(np.flatnonzero(kind).tolist()) == {u for mem in live for u in mem}
    assert marks["counts"] == (int((kind == 2).sum()), int((kind == 1).sum()), int(length[kind == 1].sum()))
    if canonical:  # the kinds from one view alone: the arms seen from the smaller source slot, and from the larger, give the same kinds
        for pick in (min, max):
            half = [(a, x, tt) for a, x, tt in arms if a == pick(a, tt ^ 1)]
            again, _ = bb.kinds_model(bb.groups_model(half, True), length, kc)
            assert np.array_equal(again, kind)
    left = None if canonical else np.bincount(lt["link_to"].astype(np.int64), minlength=len(length)).astype(np.uint8)
    got = cbl_amd.CBL.bubble_kinds(lt["link_start"], lt["link_to"], lt["link_rev"], length, left, kc, max_kmers)
    assert got.dtype == np.uint8 and np.array_equal(got, kind)
    return marks


def _components(m):
    kmers = [tm.kmer_of_word(w, m.P) for w in tm.iteration_words(m)]
    return cm.definition_model(kmers, m.P["K"], m.canonical)["components"] if kmers else 0


def _check_pop(m, max_kmers, counts, rounds, seqs=None):
    """pop_model on a copy of m: every round removes exactly the popped k-mers and keeps the component count, the stats add up, a fixpoint holds no popped
    arm, the carried counts are those of the surviving words (and, given the reads, a fresh tally on the popped index). Returns (index, stats, counts)."""
    k, canonical = m.P["K"], m.canonical
    mm, trace = rm.copy_cbl(m), []
    before = dict(zip(tm.iteration_words(m), [] if counts is None else np.asarray(counts).tolist()))
    comps = _components(m)
    st, after = bb.pop_model(mm, max_kmers, counts, rounds, trace)
    assert st["rounds"] == len(trace) and (rounds == 0 or st["rounds"] <= rounds) and st["kmers_left"] == mm.count()
    for r, (kmers, sel, marks, now) in enumerate(trace):
        nxt = trace[r + 1][0] if r + 1 < len(trace) else [tm.kmer_of_word(w, mm.P) for w in tm.iteration_words(mm)]
        assert len(set(nxt)) == len(nxt) and set(nxt) == {x for x, f in zip(kmers, sel.tolist()) if not f}
        assert int(sel.sum()) == marks["counts"][2] and (sel.any() or r + 1 == len(trace))
        if now is not None:  # the counts of a round are those its words had on entry
            assert [before[tm.word_of_kmer(x, mm.P)] for x in kmers] == now.tolist()
    removing = sum(1 for _, sel, _, _ in trace if sel.any())
    assert st["popped_kmers"] == m.count() - mm.count() and st["fixpoint"] == (removing < len(trace))
    assert _components(mm) == comps  # source and target stay connected through the kept arm
    if st["fixpoint"]:
        last = after[: mm.count()] if after is not None else None
        assert not (_check_marks([tm.kmer_of_word(w, mm.P) for w in tm.iteration_words(mm)], k, canonical, max_kmers, last)["kind"] == 1).any()
    if counts is not None:
        assert len(after) == len(counts) and not after[mm.count():].any()
        assert after[: mm.count()].tolist() == [before[w] for w in tm.iteration_words(mm)]
        if removing == 0:
            assert np.array_equal(after, np.asarray(counts, dtype=np.uint32))
        if seqs is not None:
            assert np.array_equal(after[: mm.count()], am.tally_model(mm, seqs)[0])
    return mm, st, after


_done = {}


def _case(name, canonical):
    """(k, max_kmers, the model index, its k-mers in iteration order, counts, the reads of the tally or None) of a crafted case, built through the oracle."""
    key = (name, canonical)
    if key not in _done:
        k, pb, flushes, mk, tally = bb.crafted(name)
        o = Oracle(k, pb, canonical)
        for batch in flushes:
            o.insert_seqs(*nm.Graph.arrays(batch))
        words = o.iter_words()
        m = tm.model_of_words(k, pb, canonical, words)
        assert m.serialize() == o.serialize() and tm.iteration_words(m) == words
        kmers = [tm.kmer_of_word(w, m.P) for w in words]
        counts = bb.counts_of_case(m, kmers, gm.walk_model(kmers, k, canonical), tally)
        _done[key] = (k, mk, m, kmers, counts, None if callable(tally) else tally)
    return _done[key]


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("k", [3, 5, 7])
def test_random_sets(k, canonical):
    rng = random.Random(300 * k + canonical)
    space = 1 << (2 * k)
    pool = [x for x in range(space) if bm.is_fwd(x)] if canonical else list(range(space))
    P = tm.PyCBL(k, 4, canonical).P
    marked = 0
    for trial in range(40):
        if trial % 4 == 3:  # a uniform sample: hardly ever a bubble
            held = rng.sample(pool, rng.randrange(1, min(len(pool), 200) + 1))
        else:  # the k-mers of a few random strings and of their copies with one letter changed
            held = set()
            for _ in range(rng.randrange(1, 4)):
                s = nm._rand(rng, rng.randrange(2 * k + 1, 4 * k + 4))
                for _ in range(rng.randrange(1, 4)):
                    p = rng.randrange(len(s))
                    v = s[:p] + rng.choice(nm.NUCS) + s[p + 1:]
                    held |= {nm.pack(w[i: i + k]) for w in (s, v) for i in range(len(w) - k + 1)}
            held = sorted({bm.canon(x, k)[0] for x in held} if canonical else held)
        m = tm.model_of_words(k, 4, canonical, sorted(tm.word_of_kmer(x, P) for x in held))
        kmers = [tm.kmer_of_word(w, P) for w in tm.iteration_words(m)]
        mk = rng.randrange(1, 6) if trial & 1 else k + 1
        counts = None if trial % 3 == 0 else np.array([rng.choice([0, 1, 1, 2, 3, 7, bb.MAX]) for _ in kmers], dtype=np.uint32)
        marked += int(_check_marks(kmers, k, canonical, mk, counts)["kind"].astype(bool).sum())
        _check_pop(m, mk, counts, (1, 2, 0)[trial % 3])
    assert marked > 0 or k == 3  # (at K = 3 the 64 k-mers repeat so often that hardly an arm has one way in and one way out: the sets check the refusals)
    assert _check_marks([], k, canonical, 3)["counts"] == (0, 0, 0)
    st, after = bb.pop_model(tm.PyCBL(k, 4, canonical), 3, np.zeros(0, dtype=np.uint32), 0)
    assert (st["rounds"], st["fixpoint"], st["kmers_left"]) == (1, 1, 0) and len(after) == 0


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("name", bb.CRAFTED)
def test_crafted_sets(name, canonical):
    k, mk, m, kmers, counts, seqs = _case(name, canonical)
    _check_marks(kmers, k, canonical, mk)
    _check_marks(kmers, k, canonical, mk, counts)
    for rounds in (1, 2, 0):
        _check_pop(m, mk, None, rounds)
        _check_pop(m, mk, counts, rounds, seqs)


def _first_round(name, canonical, counted=False):
    k, mk, m, kmers, counts, _ = _case(name, canonical)
    return bb.features(bb.marks_of_set(kmers, k, canonical, mk, counts if counted else None), canonical)


def test_the_case_list_holds_every_kind_of_bubble():
    for canonical in FORMS:
        for name in ("snp15", "snp31", "snp33", "snp59"):  # arms of exactly K k-mers, popped at max_kmers = K
            k = int(name[3:])
            f = _first_round(name, canonical)
            assert (f["groups"], f["popped_lengths"], f["kept_lengths"]) == ([2], [k], [k])
        f = _first_round("snp31-short", canonical)  # the same arms at max_kmers = K - 1
        assert f["groups"] == [] and f["popped_lengths"] == []
        f = _first_round("indel", canonical)
        assert (f["popped_lengths"], f["kept_lengths"]) == ([30], [31])
        assert _first_round("triple", canonical)["groups"] == [3] and _first_round("quad", canonical)["groups"] == [4]
        assert len(_first_round("quad", canonical)["popped_lengths"]) == 3
        f = _first_round("split", canonical)  # two qualified arms, two groups of one
        assert f["groups"] == [] and f["singles"] == 2
        f = _first_round("shared", canonical)  # no arm qualifies
        assert f["groups"] == [] and f["singles"] == 0
        k, mk, m, kmers, _, _ = _case("edge", canonical)  # arms of max_kmers are popped, arms of max_kmers + 1 are not arms
        t = gm.walk_model(kmers, k, canonical)
        f = _first_round("edge", canonical)
        assert f["popped_lengths"] == [mk] and sorted(t["length"].tolist()).count(mk + 1) == 2
        # ties: every arm of a bubble has the same mean; the longer arm wins the indel, the lower number the SNP
        k, mk, m, kmers, counts, _ = _case("ties", canonical)
        marks = bb.marks_of_set(kmers, k, canonical, mk, counts)
        ln, kc, kind = marks["table"]["length"], marks["kc"], marks["kind"]
        for mem in (g for g in marks["groups"].values() if len(g) >= 2):
            u, v = sorted(mem)
            assert kc[u] * int(ln[v]) == kc[v] * int(ln[u])
            assert kind[u if (ln[u], -u) > (ln[v], -v) else v] == 2
        assert sorted(_first_round("ties", canonical, True)["popped_lengths"]) == [30, 31]
        # cross: 7 over 3 k-mers beats 9 over 4 (28 > 27), while the length rule keeps the arm of 4
        assert _first_round("cross", canonical)["popped_lengths"] == [3] and _first_round("cross", canonical, True)["popped_lengths"] == [4]
        k, mk, m, kmers, counts, _ = _case("long-pair", canonical)  # every count 2^32 - 1: kc = length (2^32 - 1), equal means, the longer arm stays
        marks = bb.marks_of_set(kmers, k, canonical, mk, counts)
        assert sorted(marks["kc"][u] for u in np.flatnonzero(marks["kind"]).tolist()) == [299 * bb.MAX, 300 * bb.MAX]
        assert _first_round("long-pair", canonical, True)["popped_lengths"] == [299]
        # nested: rounds = 1, 2 and 0 give rounds / fixpoint 1 / 0, 2 / 0 and 3 / 1
        k, mk, m, kmers, counts, seqs = _case("nested", canonical)
        for cnt in (None, counts):
            res = [_check_pop(m, mk, cnt, r, seqs if cnt is not None else None) for r in (1, 2, 0)]
            assert [(st["rounds"], st["fixpoint"]) for _, st, _ in res] == [(1, 0), (2, 0), (3, 1)]
            blobs = [mm.serialize() for mm, _, _ in res]
            assert blobs[0] != blobs[1] and blobs[1] == blobs[2] and [st["popped"] for _, st, _ in res] == [1, 2, 2]
        assert _first_round("chain", canonical)["groups"] == [2, 2]  # two independent bubbles in one round
        assert _first_round("loop", canonical)["loop"]  # the source's unitig is the target's
        f = _first_round("tipped", canonical)  # no bubble until the tip is clipped
        assert f["groups"] == []
        k, mk, m, kmers, _, _ = _case("tipped", canonical)
        mm = rm.copy_cbl(m)
        assert tm.clip_model(mm, 4, False, 1)["tips"] == 1  # (the ends of the reads are longer dead ends)
        assert bb.pop_model(mm, mk, None, 1)[0]["popped"] == 1
        for n in bb.SIZES:  # unitig counts at the wave and workgroup edges of the per-unitig and per-slot grids
            f = _first_round(f"sized{n}", canonical)
            assert f["unitigs"] == n and f["groups"] == [2] * 8
        # deep: buckets of many words; Vecs that lose a word that is not their last one, so ordinals move under the carry
        k, mk, m, kmers, counts, seqs = _case("deep", canonical)
        assert max(len(b[1]) for b in m.buckets.values()) >= 100
        words = tm.iteration_words(m)
        sel = bb.selected(bb.marks_of_set(kmers, k, canonical, mk, counts))
        gone = {w for w, f in zip(words, sel.tolist()) if f}
        sb = m.P["SB"]
        lost = {p: [((p << sb) | s) in gone for s in items] for p, (kd, items) in m.buckets.items() if kd == "vec"}
        assert any(True in f and False in f[f.index(True):] for f in lost.values())
        mm, st, after = _check_pop(m, mk, counts, 1, seqs)
        moved = [w for j, w in enumerate(tm.iteration_words(mm)) if [x for x in words if x not in gone][j] != w]
        assert moved  # the survivors are not in their old relative order: a carry by compaction alone would be wrong
    # a bucket that empties, in both forms
    for canonical in FORMS:
        k, mk, m, _, _, _ = _case("snp31", canonical)
        assert len(_check_pop(m, mk, None, 1)[0].buckets) < len(m.buckets)
    k, mk, m, _, _, _ = _case("deep", True)
    assert len(_check_pop(m, mk, None, 1)[0].buckets) < len(m.buckets)
    # the bidirected views: an arm entered at the head of its mirror image, a writing view with an odd source slot, the self-mirror group
    feats = {name: _first_round(name, True) for name in bb.CRAFTED}
    assert feats["strands"]["entered_reversed"] and any(f["source_odd"] for f in feats.values())
    assert feats["mirror2"]["self_mirror"] and feats["mirror2"]["groups"] == [2]
    f1 = feats["mirror1"]  # one unitig, both images in the group: never compared with itself
    assert f1["groups"] == [] and f1["singles"] == 1
    k, mk, m, kmers, _, _ = _case("mirror1", True)
    arms = bb.marks_of_set(kmers, k, True, mk)["arms"]
    assert len(arms) == 2 and arms[0][0] == arms[0][2] ^ 1 and arms[0][1] == arms[1][1] ^ 1
    assert not any(_first_round(name, False)["entered_reversed"] for name in bb.CRAFTED)
