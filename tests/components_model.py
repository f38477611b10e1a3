"""Connected components of the compacted de Bruijn graph on the CPU, in both forms, and the crafted read sets of the CPU and the GPU
tests. (i) The definition: a union-find straight on the stored k-mers over gfa_model.edges — the weakly connected components of the graph —, which must
never split a unitig. (ii) The route the device takes, restated with numpy: the link table of gfa_model.definition_model, then rounds of hook and compress;
it returns `rounds`. (iii) The filter as one removal_model.remove_batch on an oracle.pyref.PyCBL. Pure CPU; no expectation comes from the GPU path. A helper,
not a test file.

    component       a class of the smallest equivalence on the unitigs in which u ~ link_to[l] for every link l that leaves slot 2 u or 2 u + 1
    numbering       0 .. C - 1 by ascending smallest unitig, first[c]
    table           component (uint32 per unitig), kmer_component (uint32 per k-mer), first, unitigs (uint32 per component), kmers (uint64 per component)
    counts          kmers, unitigs, links, components, largest_kmers, rounds
    a round         hook: nxt = par; for every link (u, v) with a = par[u] != b = par[v]: nxt[max(a, b)] = min(nxt[max(a, b)], min(a, b)); a round whose hook
                    changes nothing ends the loop and counts. Compress: nxt = nxt[nxt] until nothing moves; the result is par. No round on an empty set."""
from __future__ import annotations

import random

import numpy as np

from oracle.pyref import PyCBL

import biunitigs_model as bm
import gfa_model as gm
import removal_model as rm
import tips_model as tm
from neighbors_model import _primitive, _rand

COUNTS = ("kmers", "unitigs", "links", "components", "largest_kmers", "rounds")
STATS = ("components", "removed_components", "removed_kmers", "kmers_left", "largest_kmers", "rounds")
ARRAYS = ("component", "kmer_component", "first", "unitigs", "kmers")
MAX_ROUNDS = 128


# ---- the table of a labelling ------------------------------------------------------------------------------------------------------------------------
def _table(t, label, n_links: int, rounds):
    """`label`: per unitig, any value that is equal exactly inside a component. Numbered by ascending smallest unitig."""
    nu, n = len(t["head"]), len(t["unitig"])
    number, first = {}, []
    component = np.zeros(nu, dtype=np.uint32)
    for u in range(nu):
        key = int(label[u])
        if key not in number:
            number[key] = len(first)
            first.append(u)
        component[u] = number[key]
    nc = len(first)
    unitigs = np.bincount(component, minlength=nc).astype(np.uint32) if nu else np.zeros(0, dtype=np.uint32)
    kmers = np.bincount(component, weights=t["length"].astype(np.float64), minlength=nc).astype(np.uint64) if nu else np.zeros(0, dtype=np.uint64)
    out = {"component": component, "kmer_component": component[t["unitig"].astype(np.int64)] if n else np.zeros(0, dtype=np.uint32),
           "first": np.array(first, dtype=np.uint32), "unitigs": unitigs, "kmers": kmers, "kmers_n": n, "unitigs_n": nu, "links": n_links, "components": nc,
           "largest_kmers": int(kmers.max()) if nc else 0, "rounds": rounds}
    return out


def counts_of(table):
    return (table["kmers_n"], table["unitigs_n"], table["links"], table["components"], table["largest_kmers"], table["rounds"])


def largest_of(table) -> int:
    """The number of the largest component: most k-mers, a tie goes to the lower number."""
    return int(np.argmax(table["kmers"])) if table["components"] else -1


def same_table(a, b, rounds: bool = True):
    return all(np.array_equal(a[key], b[key]) and a[key].dtype == b[key].dtype for key in ARRAYS) and counts_of(a)[: 6 if rounds else 5] == counts_of(b)[: 6 if rounds else 5]


# ---- (i) the definition ------------------------------------------------------------------------------------------------------------------------------
def _find(p, x):
    while p[x] != x:
        p[x] = p[p[x]]
        x = p[x]
    return x


def definition_model(kmers, k: int, canonical: bool, t=None, lt=None):
    """Union-find on the stored k-mers over every edge of the graph (an oriented k-mer 2 i + s is k-mer i). `rounds` is None: the definition has no rounds."""
    t = gm.walk_model(kmers, k, canonical) if t is None else t
    lt = gm.definition_model(kmers, k, canonical, t) if lt is None else lt
    p = list(range(len(kmers)))
    for v, _, w in gm.edges(kmers, k, canonical):
        a, b = _find(p, v >> 1), _find(p, w >> 1)
        if a != b:
            p[max(a, b)] = min(a, b)
    cls = [_find(p, i) for i in range(len(kmers))]
    label = np.full(len(t["head"]), -1, dtype=np.int64)
    for i, u in enumerate(t["unitig"].tolist()):
        assert label[u] in (-1, cls[i])  # a unitig lies inside one class: the components of the unitigs ARE those of the k-mers
        label[u] = cls[i]
    return _table(t, label, lt["n_links"], None)


# ---- (ii) the device's route ---------------------------------------------------------------------------------------------------------------------------
def link_pairs(lt):
    """(from unitig, to unitig) arrays of a link table: sides and link_rev dropped."""
    start = lt["link_start"].astype(np.int64)
    frm = np.repeat(np.arange(len(start) - 1, dtype=np.int64) >> 1, np.diff(start))
    return frm, lt["link_to"].astype(np.int64)


def label_model(nu: int, frm, to):
    """(par, rounds) of the hook / compress rule on the links (frm[l], to[l]) over nu unitigs."""
    par = np.arange(nu, dtype=np.int64)
    rounds = 0
    if nu == 0:
        return par, rounds
    while True:
        assert rounds < MAX_ROUNDS
        a, b = par[frm], par[to]
        differ = a != b
        nxt = par.copy()
        np.minimum.at(nxt, np.maximum(a, b)[differ], np.minimum(a, b)[differ])
        rounds += 1
        if not differ.any():
            assert np.array_equal(nxt, par)
            return par, rounds
        while True:
            g = nxt[nxt]
            if np.array_equal(g, nxt):
                break
            nxt = g
        par = nxt


def route_model(kmers, k: int, canonical: bool, t=None, lt=None):
    t = gm.walk_model(kmers, k, canonical) if t is None else t
    lt = gm.definition_model(kmers, k, canonical, t) if lt is None else lt
    frm, to = link_pairs(lt)
    par, rounds = label_model(len(t["head"]), frm, to)
    assert (par <= np.arange(len(par))).all() and np.array_equal(par[par], par)  # the smallest unitig of the component
    return _table(t, par, lt["n_links"], rounds)


def check_identities(table, lt):
    """What every table satisfies."""
    n, nu, nc = table["kmers_n"], table["unitigs_n"], table["components"]
    first = table["first"].astype(np.int64)
    assert (np.diff(first) > 0).all() and int(table["kmers"].sum()) == n and int(table["unitigs"].sum()) == nu and len(first) == nc
    assert nu == 0 or (first[0] == 0 and np.array_equal(table["component"][first], np.arange(nc)))
    frm, to = link_pairs(lt)
    assert np.array_equal(table["component"][frm], table["component"][to])  # every link joins equal labels
    assert (nc == 0) == (n == 0) and table["largest_kmers"] == (int(table["kmers"].max()) if nc else 0)


# ---- (iii) the filter --------------------------------------------------------------------------------------------------------------------------------
def dropped(table, min_kmers=None, largest: bool = False):
    """Per component: whether the filter removes it. Exactly one rule."""
    assert (min_kmers is None) == bool(largest) and (largest or min_kmers >= 1)
    if largest:
        drop = np.ones(table["components"], dtype=bool)
        if table["components"]:
            drop[largest_of(table)] = False
        return drop
    return table["kmers"] < np.uint64(min_kmers)


def filter_model(m: PyCBL, min_kmers=None, largest: bool = False, trace=None, table=None):
    """cblx_components_filter on m, in place; returns the stats. trace (a list) takes (k-mers in iteration order, the table, the selection per k-mer). `table`:
    route_model's of m's k-mers in iteration order, where the caller has it already."""
    k, canonical = m.P["K"], m.canonical
    words = tm.iteration_words(m)
    kmers = [tm.kmer_of_word(w, m.P) for w in words]
    table = route_model(kmers, k, canonical) if table is None else table
    drop = dropped(table, min_kmers, largest)
    sel = drop[table["kmer_component"].astype(np.int64)] if len(kmers) else np.zeros(0, dtype=bool)
    if trace is not None:
        trace.append((kmers, table, sel))
    st = {"components": table["components"], "removed_components": int(drop.sum()), "removed_kmers": int(table["kmers"][drop].sum()) if len(drop) else 0,
          "kmers_left": 0, "largest_kmers": table["largest_kmers"], "rounds": table["rounds"]}
    assert st["removed_kmers"] == int(sel.sum())
    if sel.any():
        rm.remove_batch(m, [w for w, f in zip(words, sel.tolist()) if f])  # the words of the selected k-mers are the stored words themselves
    st["kmers_left"] = m.count()
    return st


def wave_views(table, wave: int = 64):
    """The number of distinct components among every `wave` consecutive unitigs: what a wave of k_cc_sizes sees."""
    c = table["component"]
    return [len(set(c[a: a + wave].tolist())) for a in range(0, len(c), wave)]


# ---- crafted read sets: lists of reads (bytes), usable in both forms -----------------------------------------------------------------------------------
def comb_reads(k: int = 31, branches: int = 2000, every: int = 6, seed: int = 61):
    """A random trunk with a dead-end branch of 2 k-mers leaving it every `every` k-mers: one component whose unitigs form a chain `branches` long."""
    rng = random.Random(seed + k)
    trunk = _rand(rng, every * (branches + 1) + k)
    return [trunk.encode()] + [tm._leaving(rng, trunk, every * (j + 1), k, 2).encode() for j in range(branches)]


def _path(rng, k: int, m: int) -> str:
    return _rand(rng, k - 1 + m)


def _cycle(rng, k: int, m: int) -> str:
    s = _rand(rng, m)
    while not _primitive(s):
        s = _rand(rng, m)
    return (s * (k // m + 2))[: m + k - 1]


def archipelago_reads(k: int, mk: int, islands: int = 300, seed: int = 67, extras: bool = True):
    """`islands` separate paths and pure cycles of mk - 1, mk and mk + 1 k-mers by turns. With `extras` every fifth one is a cycle, and there are also: two paths of 12 mk
    k-mers (the two equal largest components), a trunk with two branches (a component of several unitigs), and a path of mk - 1 k-mers over C and G alone,
    whose words have a prefix of their own, so that the filter empties a bucket. The islands are shuffled, so their unitig numbers interleave."""
    rng = random.Random(seed + k)
    reads = []
    for j in range(islands):
        m = mk - 1 + j % 3
        reads.append(_cycle(rng, k, m) if extras and j % 5 == 4 else _path(rng, k, m))
    if extras:
        reads += [_path(rng, k, 12 * mk), _path(rng, k, 12 * mk)]
        trunk = _rand(rng, 4 * k)
        reads += [trunk, tm._leaving(rng, trunk, k, k, 3), tm._entering(rng, trunk, 2 * k, k, 2)]
        reads.append("".join(rng.choice("CG") for _ in range(k - 1 + mk - 1)))
    rng.shuffle(reads)
    return [r.encode() for r in reads]


def one_kmer_reads(k: int):
    return [_rand(random.Random(71 + k), k).encode()]


MIN_KMERS = {"arch15": 6, "arch31": 9}  # the mk of the archipelagos
CRAFTED = ["comb", "arch15", "arch31", "arch64", "arch256", "arch257", "strands", "one", "empty"]
OLD = ["islands", "dense", "cycles", "hairpin", "at", "homopolymers", "branch"]  # of tips_model / biunitigs_model


def crafted(name):
    """(k, pb, flushes) of a case: the CPU and the GPU tests insert the same flushes, into an index of either form."""
    if name == "comb":
        return 31, 24, [comb_reads()]
    if name == "arch15":
        return 15, 6, [archipelago_reads(15, MIN_KMERS[name])]
    if name == "arch31":
        return 31, 24, [archipelago_reads(31, MIN_KMERS[name])]
    if name in ("arch64", "arch256", "arch257"):  # exactly that many unitigs, every one a component
        return 31, 24, [archipelago_reads(31, 4, islands=int(name[4:]), extras=False)]
    if name == "strands":
        first, second = bm.strand_reads(31)
        return 31, 24, [first, second]
    if name == "one":
        return 31, 24, [one_kmer_reads(31)]
    if name == "empty":
        return 31, 24, []
    if name == "islands":
        return 31, 24, [tm.island_reads(31, 30)]
    k, pb, flushes = bm.crafted(name)
    return k, pb, flushes


def build_case(k: int, pb: int, canonical: bool, flushes):
    """(the oracle's bytes, the model index, the k-mers in iteration order) of an index that took the flushes, one insert each."""
    from oracle import Oracle

    import neighbors_model as nm

    o = Oracle(k, pb, canonical)
    for batch in flushes:
        o.insert_seqs(*nm.Graph.arrays(batch))
    blob = o.serialize()
    m = tm.model_of_words(k, pb, canonical, o.iter_words())
    assert m.serialize() == blob
    return blob, m, nm.oracle_kmers(o)


def features(table, lt):
    """What a case exercises."""
    start = lt["link_start"].astype(np.int64)
    frm, to = link_pairs(lt)
    slot = np.repeat(np.arange(len(start) - 1, dtype=np.int64), np.diff(start))
    single = table["unitigs"][table["component"]] == 1 if table["unitigs_n"] else np.zeros(0, dtype=bool)
    self_link = frm == to
    return {"single_with_self_link": bool((self_link & single[frm]).any()) if len(frm) else False,
            "slot_of_4": bool((np.diff(start) == 4).any()), "one_component": table["components"] == 1 and table["unitigs_n"] > 1,
            "all_singletons": table["components"] == table["unitigs_n"] and table["unitigs_n"] > 1,
            "rev_links": bool((lt["link_rev"] == 1).any()) if len(frm) else False, "odd_slots": bool((slot & 1).any()) if len(slot) else False,
            "views": sorted(set(wave_views(table)))}
