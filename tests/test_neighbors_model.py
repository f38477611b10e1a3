"""De Bruijn neighbourhoods on the CPU: CBL.neighbor_kmers and the models of tests/neighbors_model.py against a string-level definition (a successor of
ACTG string s is s[1:] + c, a predecessor c + s[:-1]), CBL.degree_summary and graph_report on hand-written tables, and the new names where the header,
the bindings, the built library and the Rust crates carry them."""
import os
import random
import re

import numpy as np
import pytest

import cbl_amd
from oracle import Oracle

import neighbors_model as nm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_neighbors_kmers": 5, "cblx_neighbors_kmers_device": 5, "cblx_neighbors_range": 5, "cblx_neighbors_range_device": 5, "cblx_degree_table": 2}
KERNELS = ("k_neighbor_words", "k_fold_neighbor_flags", "k_degree_tally")


def _edge_strings(k, rng):
    """Random k-mers, and k-mers whose first and last bases are each of the four codes."""
    out = ["".join(rng.choice(nm.NUCS) for _ in range(k)) for _ in range(20)]
    for a in nm.NUCS:
        for b in nm.NUCS:
            out.append(a + "".join(rng.choice(nm.NUCS) for _ in range(k - 2)) + b)
    return out + [c * k for c in nm.NUCS]


@pytest.mark.parametrize("k", [15, 31, 33, 59])
def test_neighbor_kmers_against_strings(k):
    rng = random.Random(k)
    for s in _edge_strings(k, rng):
        x = nm.pack(s)
        assert nm.unpack(x, k) == s
        want = [nm.pack(y) for y in nm.neighbors_str(s)]
        assert cbl_amd.CBL.neighbor_kmers(x, k) == want, s
        assert nm.neighbors(x, k) == want, s
        assert all(0 <= y < 1 << (2 * k) for y in want)
    with pytest.raises(ValueError):
        cbl_amd.CBL.neighbor_kmers(1 << (2 * k), k)


@pytest.mark.parametrize("k,pb,canonical", [(15, 6, False), (15, 6, True), (33, 16, False), (33, 16, True)])
def test_mask_model_against_a_set_of_strings(k, pb, canonical):
    g = nm.Graph(k)
    o = Oracle(k, pb, canonical)
    o.insert_seqs(*nm.Graph.arrays(g.batch1))
    held = set()
    for r in g.batch1:
        r = r.decode()
        for i in range(len(r) - k + 1):
            held.add(nm.canonical_str(r[i: i + k]) if canonical else r[i: i + k])
    assert {nm.unpack(x, k) for x in nm.oracle_kmers(o)} == held and o.count() == len(held)
    qs = nm.queries(g, o, canonical)
    masks = nm.masks_model(o, qs, k)
    assert masks.tolist() == [nm.mask_str(held, nm.unpack(x, k), canonical) for x in qs]
    by = {x: int(m) for x, m in zip(qs, masks)}
    if not canonical:  # (a canonical index may hold more: the reverse complements count as well)
        assert by[nm.pack(g.fork)] & 15 == 15 and by[nm.pack(g.join)] >> 4 == 15
        for c, ch in enumerate(nm.NUCS):
            m = by[nm.pack(ch * k)]
            assert (m >> c) & 1 and (m >> (4 + c)) & 1  # a self-loop sets its bit in both nibbles
        ring = g.ring
        assert (by[nm.pack(ring)] >> nm.CODE[ring[0]]) & 1 and (by[nm.pack(ring)] >> (4 + nm.CODE[ring[-1]])) & 1  # the next and the previous rotation
        assert (by[nm.pack(g.dinuc)] >> nm.CODE["C"]) & 1 and (by[nm.pack(g.dinuc_partner)] >> nm.CODE["A"]) & 1  # the 2-cycle
        t = nm.table_model(nm.masks_model(o, nm.oracle_kmers(o), k))
        s = cbl_amd.CBL.degree_summary(t)
        assert s["nodes"] == o.count() and s["out_edges"] == s["in_edges"]  # every edge is seen once from each end
    # an index that holds s alone does not show the rotations of s: they share its necklace, at other positions
    alone = Oracle(k, pb, canonical)
    assert alone.insert_kmer(nm.pack(g.ring))
    assert nm.mask_model(alone, nm.pack(g.ring), k) == nm.mask_str({nm.canonical_str(g.ring) if canonical else g.ring}, g.ring, canonical)
    if not canonical:
        assert nm.mask_model(alone, nm.pack(g.ring), k) == 0


def test_degree_summary_and_graph_report():
    from cbl_amd.__main__ import graph_report

    t = np.zeros((5, 5), dtype=np.uint64)
    t[0, 0], t[1, 0], t[0, 1], t[1, 1], t[2, 1], t[1, 4], t[3, 0], t[0, 2], t[4, 4] = 3, 5, 7, 100, 11, 13, 2, 1, 17
    s = cbl_amd.CBL.degree_summary(t)
    assert list(s) == ["nodes", "out_edges", "in_edges", "isolated", "sources", "sinks", "simple", "branching"]
    assert s["nodes"] == int(t.sum()) == 159
    assert s["out_edges"] == 5 + 100 + 22 + 13 + 6 + 68 and s["in_edges"] == 7 + 100 + 11 + 52 + 2 + 68
    assert (s["isolated"], s["sources"], s["sinks"], s["simple"], s["branching"]) == (3, 5 + 2, 7 + 1, 100, 11 + 13 + 2 + 1 + 17)
    # every node is in a class; only a source or a sink of degree 2 or more is in two (it is branching as well)
    twice = int(t[2:, 0].sum() + t[0, 2:].sum())
    assert s["isolated"] + s["sources"] + s["sinks"] + s["simple"] + s["branching"] - twice == s["nodes"]
    assert cbl_amd.CBL.degree_summary(t.reshape(25)) == s and cbl_amd.CBL.degree_summary(t.tolist()) == s
    assert all(type(v) is int for v in s.values())
    big = np.zeros((5, 5), dtype=np.uint64)
    big[4, 4] = (1 << 63) + 5  # Python ints: no 64-bit wrap in the edge sums
    assert cbl_amd.CBL.degree_summary(big)["out_edges"] == 4 * ((1 << 63) + 5)
    lines, summary, human = graph_report(t)
    assert lines == ["3\t7\t1\t0\t0", "5\t100\t0\t0\t13", "0\t11\t0\t0\t0", "2\t0\t0\t0\t0", "0\t0\t0\t0\t17"]
    assert summary == [f"{key}\t{value}" for key, value in s.items()] and summary[0] == "nodes\t159"
    assert len(human) == 2 and "159 nodes" in human[0]
    zero = np.zeros((5, 5), dtype=np.uint64)
    lines, summary, _ = graph_report(zero)
    assert lines == ["0\t0\t0\t0\t0"] * 5 and all(ln.endswith("\t0") for ln in summary)
    with pytest.raises(ValueError):
        graph_report(np.zeros((4, 5)))


def test_table_model():
    masks = [0x00, 0x01, 0x10, 0x11, 0xFF, 0xF0, 0x0F, 0x35, 0x11]
    t = nm.table_model(masks)
    assert t[0, 0] == 1 and t[1, 0] == 1 and t[0, 1] == 1 and t[1, 1] == 2 and t[4, 4] == 1 and t[0, 4] == 1 and t[4, 0] == 1 and t[2, 2] == 1
    assert int(t.sum()) == len(masks)


def test_bindings_header_and_kernels_carry_the_new_names():
    with open(os.path.join(ROOT, "include", "cblx.h")) as f:
        header = f.read()
    note = header[: header.index("#define CBLX_ABI_VERSION 3")]
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    with open(os.path.join(ROOT, "rust", "cblx-sys", "src", "lib.rs")) as f:
        sys_rs = f.read()
    for name, nargs in NEW.items():
        assert name in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES[name][1]) == nargs, name
        assert hasattr(cbl_amd.lib(), name), name
        assert re.search(r"\b%s\b(?!_)" % name, note), f"{name} is not named in the 'Added under 3' note in front of CBLX_ABI_VERSION"
        assert re.search(r"\bint %s\s*\(" % name, body), f"{name} is not declared"
        assert re.search(r"pub fn %s\s*\(" % name, sys_rs), f"{name} is not declared in the Rust sys crate"
    with open(os.path.join(ROOT, "cbl_amd", "csrc", "kernels_graph.hpp")) as f:
        kg = f.read()
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kg), kernel
    for meth in ("neighbors_np", "neighbors_device", "neighbors_range_np", "neighbors_range_device", "degree_table", "successors", "predecessors", "neighbor_kmers",
                 "degree_summary"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    with open(os.path.join(ROOT, "rust", "cbl-gpu", "src", "lib.rs")) as f:
        facade = f.read()
    assert re.search(r"pub fn neighbors\b", facade) and re.search(r"pub fn degree_table\b", facade)
