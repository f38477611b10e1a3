"""The abundance model (tests/abundance_model.py) against its own definitions, on the CPU: the sums, the tagged text and its way back, both filter rules
as one remove_batch. Random sets at K = 3, 5, 7 in both forms and the crafted cases."""
import random

import numpy as np
import pytest

from oracle import Oracle
from oracle.pyref import PyCBL

import abundance_model as am
import biunitigs_model as bm
import gfa_model as gm
import neighbors_model as nm
import removal_model as rm
import setops_model as sm
import tips_model as tm

FORMS = (True, False)


def _random_case(k, canonical, seed):
    """A PyCBL of random reads at a small K (many repeats, branches and cycles), and reads to tally: some of its own, some foreign, some short."""
    rng = random.Random(seed * 100 + k + canonical)
    pb = 2
    m = PyCBL(k, pb, canonical)
    own = [nm._rand(rng, rng.randrange(k, 4 * k)).encode() for _ in range(3 if k == 3 else 8)]
    for r in own:
        m.insert_seq(r)
    batch = own[::2] + [nm._rand(rng, 3 * k).encode() for _ in range(4)] + [b"AC", own[0], own[0][::-1]]
    return m, batch


def _crafted_case(name, canonical):
    k, pb, flushes = bm.crafted(name)
    o = Oracle(k, pb, canonical)
    for batch in flushes:
        o.insert_seqs(*nm.Graph.arrays(batch))
    m = tm.model_of_words(k, pb, canonical, o.iter_words())
    assert m.serialize() == o.serialize()
    reads = [r for batch in flushes for r in batch]
    return m, reads[: 40] + reads[: 3]


CASES = [("random", k, s) for k in (3, 5, 7) for s in (1, 2)] + [("crafted", name, 0) for name in ("cycles", "hairpin", "at", "homopolymers", "branch", "graph15")]


def _case(kind, what, seed, canonical):
    return _random_case(what, canonical, seed) if kind == "random" else _crafted_case(what, canonical)


@pytest.mark.parametrize("canonical", FORMS)
@pytest.mark.parametrize("kind,what,seed", CASES)
def test_sums_text_and_filters(kind, what, seed, canonical):
    m, batch = _case(kind, what, seed, canonical)
    k = m.P["K"]
    words = tm.iteration_words(m)
    n = len(words)
    counts, total, found = am.tally_model(m, batch)
    assert total == sum(len(am.enumerate_words(m, s)) for s in batch) and 0 < found <= total and int(counts.sum()) == found
    again, t2, f2 = am.tally_model(m, batch, counts)  # the call accumulates
    assert (t2, f2) == (total, found) and np.array_equal(again, 2 * counts)
    hist = am.spectrum(counts)
    assert int(hist.sum()) == n and int((hist * np.arange(256)).sum()) == found  # (no count reaches 255 here)
    table = am.table_of(m)
    kmers = [tm.kmer_of_word(w, m.P) for w in words]
    kc = am.kc_model(table, counts)
    assert sum(kc) == int(counts.sum()) and len(kc) == len(table["head"])  # sum of kc = sum of counts
    # the tagged text parses back to the untagged text plus the tags
    text = gm.gfa_model(kmers, k, canonical, table, gm.definition_model(kmers, k, canonical, table))
    for with_kc in (True, False):
        tagged = am.tagged_text(text, table, k, kc if with_kc else None)
        back, tags = am.untag(tagged)
        assert back == text
        assert tags == [(u, int(table["length"][u]) + k - 1, kc[u] if with_kc else None) for u in range(len(kc))]
    # the filter removes exactly the selected k-mers
    for unitigs in (False, True):
        for mc in (1, 2, int(counts.max()) + 1):
            sel, gone = am.select_model(counts, mc, table if unitigs else None)
            c = rm.copy_cbl(m)
            st = am.filter_model(c, counts, mc, unitigs)
            want = {w for w, f in zip(words, sel.tolist()) if not f}
            assert sm.words(c) == want and st["kmers_left"] == len(want) == c.count()
            assert st == {"kmers": n, "removed_kmers": n - len(want), "unitigs": len(kc) if unitigs else 0, "removed_unitigs": len(gone), "kmers_left": len(want),
                          "min_count": mc}
            if unitigs and mc == 1:  # min_count = 1 keeps exactly the unitigs of mean coverage >= 1: none without support goes free, and a unitig
                # whose every k-mer has support stays. (A unitig with some support but kc < length goes: the rule is the mean, in integers.)
                ln = table["length"].tolist()
                assert gone == [u for u, v in enumerate(kc) if v < ln[u]] and set(gone) >= {u for u, v in enumerate(kc) if v == 0}
                covered = {u for u in range(len(kc)) if all(counts[i] for i in am.members(table)[u])}
                assert not covered & set(gone)
            if mc == int(counts.max()) + 1 and not unitigs:  # a threshold above every count empties the index
                assert c.count() == 0 and not c.buckets
        c = rm.copy_cbl(m)
        am.filter_model(c, counts, (max(kc) if unitigs else int(counts.max())) + 1, unitigs)
        assert c.count() == 0 and c.serialize() == PyCBL(k, m.P["PB"], canonical).serialize()


@pytest.mark.parametrize("canonical", FORMS)
def test_enumerations_agree_and_both_strands_count(canonical):
    """The oracle's enumeration and the Python restatement give the same occurrences (dirty bytes, short sequences); a read and its reverse complement
    count for the same stored k-mers of a canonical index."""
    k, pb = 15, 6
    reads = tm.deep_reads(k)
    o, m = Oracle(k, pb, canonical), PyCBL(k, pb, canonical)
    for r in reads:
        o.insert_seq(r)
        m.insert_seq(r)
    assert o.serialize() == m.serialize() and o.iter_words() == tm.iteration_words(m)
    batches = am.tally_reads(k, reads)
    for name, batch in batches.items():
        assert am.occurrences(o, batch) == am.occurrences(m, batch), name
        a, b = am.tally_model(o, batch), am.tally_model(m, batch)
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:], name
    c, total, found = am.tally_model(o, batches["both-strands"])
    one, t1, f1 = am.tally_model(o, batches["both-strands"][:1])
    assert total == 2 * t1
    if canonical:
        assert found == 2 * f1 and np.array_equal(c, 2 * one)
    assert am.tally_model(o, batches["none"])[1:] == (0, 0) and am.tally_model(o, batches["only-short"])[1:] == (0, 0)
    assert am.tally_model(o, batches["miss"])[2] == 0 and am.tally_model(o, batches["miss"])[1] > 0
    pa = am.tally_model(o, batches["poly-a"])
    assert pa[1] == 300 - k + 1 and pa[2] == 0  # the index of deep_reads holds no poly-A


def test_saturation_spectrum_and_digit_counts():
    before = np.array([am.MAX - 2, am.MAX, 7, 0], dtype=np.uint32)
    assert am.accumulate(before, [5, 5, 5, 0]).tolist() == [am.MAX, am.MAX, 12, 0]
    h = am.spectrum(np.array([0, 1, 254, 255, 256, am.MAX, 1], dtype=np.uint32))
    assert (int(h[0]), int(h[1]), int(h[254]), int(h[255]), int(h.sum())) == (1, 2, 1, 3, 7)
    k = 31
    reads = am.long_unitig_reads(k)
    o = Oracle(k, 24, False)
    o.insert_seqs(*nm.Graph.arrays(reads))
    kmers = nm.oracle_kmers(o)
    table = gm.walk_model(kmers, k, False)
    counts, kc = am.digit_counts(table)
    assert set(am.DIGIT_TARGETS) <= set(kc) and 300 * am.MAX in kc and len(str(300 * am.MAX)) == 13
    assert sum(kc) == int(counts.astype(np.uint64).sum()) and 1 in table["length"].tolist()
    mc = 5
    ec = am.unitig_edge_counts(table, mc)
    ekc = am.kc_model(table, ec)
    ln = table["length"].tolist()
    assert {ekc[u] - mc * ln[u] for u in range(len(ln)) if u % 3 != 2} == {-1, 0}
    a, _ = am.select_model(ec, mc, None)
    b, _ = am.select_model(ec, mc, table)
    assert not np.array_equal(a, b)  # the two rules differ on these counts
    rng = random.Random(9)
    for _ in range(300):
        hist = [rng.randrange(4) for _ in range(rng.randrange(1, 12))]
        import cbl_amd

        assert cbl_amd.CBL.solid_threshold(hist) == am.solid_threshold(hist), hist
