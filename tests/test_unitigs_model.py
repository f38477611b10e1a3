"""Unitigs on the CPU: the sequential walk of tests/unitigs_model.py (the definition) against the restatement of the device's route (jump rounds with the
stall rule, cycle cut, numbering) on random k-mer sets and on every crafted input of the GPU tests; the identities of the definition; the text and its
way back to the set; CBL.unitig_summary; and the new names where the header, the bindings, the built library, the command line and the Rust crates
carry them."""
import os
import random
import re

import numpy as np
import pytest

import cbl_amd
from oracle import Oracle

import neighbors_model as nm
import unitigs_model as um

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_rank_kmers": 5, "cblx_rank_kmers_device": 5, "cblx_unitig_table": 11, "cblx_unitig_table_device": 11, "cblx_unitigs_text_device": 5,
       "cblx_unitigs_to_fd": 5, "cblx_unitigs_to_file": 5}
KERNELS = ("k_rank", "k_unitig_links", "k_unitig_jump", "k_cycle_min", "k_cycle_cut", "k_unitig_number", "k_unitig_text")


def _both(kmers, k):
    masks = um.masks_of_set(kmers, k)
    walk, route = um.walk_model(kmers, k, masks), um.route_model(kmers, k, masks)
    assert um.same_table(walk, route), "the route's restatement differs from the walk"
    assert walk["n_simple"] == route["n_simple"]
    um.check_identities(walk, len(kmers))
    um.check_identities(route, len(kmers))
    text = um.text_model(kmers, walk, k)
    assert sorted(um.kmers_of_text(text, k)) == sorted(kmers)  # the lines re-cut into k-mers give the set, each k-mer once
    return walk, route, text


@pytest.mark.parametrize("k", [3, 5, 7])
def test_walk_equals_route_on_random_sets(k):
    """Dense random sets: at K = 3 every density from a few k-mers to all 64, cycles of every kind included (the order of the list is the ordinal)."""
    rng = random.Random(k)
    circular = 0
    for trial in range(100):
        space = 1 << (2 * k)
        n = rng.randrange(1, min(space, 400) + 1)
        kmers = rng.sample(range(space), n)
        walk, _, _ = _both(kmers, k)
        circular += walk["n_circular"]
    assert circular > 0  # the cycle cut was exercised
    # sets made of cycles: the rotations of random strings, in shuffled order, plus loose k-mers
    for trial in range(100):
        held = set()
        for _ in range(rng.randrange(1, 5)):
            s = nm._rand(rng, rng.randrange(1, 30))
            r = s * (k // len(s) + 2)
            held |= {nm.pack(r[i: i + k]) for i in range(len(s))}
        held |= {rng.getrandbits(2 * k) for _ in range(rng.randrange(0, 4))}
        kmers = list(held)
        rng.shuffle(kmers)
        _both(kmers, k)


def test_set_masks_equal_the_oracle_masks():
    k, pb = 15, 6
    g = nm.Graph(k)
    o = Oracle(k, pb, False)
    for batch in (g.batch1, g.batch2):
        o.insert_seqs(*nm.Graph.arrays(batch))
    kmers = nm.oracle_kmers(o)
    assert np.array_equal(um.masks_of_set(kmers, k), nm.masks_model(o, kmers, k))


@pytest.mark.parametrize("k,pb", [(15, 6), (31, 24), (33, 16)])
def test_the_neighbour_graph_has_six_circular_unitigs(k, pb):
    g = nm.Graph(k)
    o = Oracle(k, pb, False)
    for batch in (g.batch1, g.batch2):
        o.insert_seqs(*nm.Graph.arrays(batch))
    kmers = nm.oracle_kmers(o)
    walk, route, _ = _both(kmers, k)
    circ = sorted(walk["length"][walk["flags"] == 1].tolist())
    assert circ == sorted([1, 1, 1, 1, 2, k]), circ  # the four homopolymers, the dinucleotide pair, the rotation ring
    by = {x: i for i, x in enumerate(kmers)}
    ring = [by[nm.pack(g.ring[i:] + g.ring[:i])] for i in range(k)]
    u = int(walk["unitig"][ring[0]])
    assert {int(walk["unitig"][i]) for i in ring} == {u} and int(walk["head"][u]) == min(ring) and int(walk["length"][u]) == k
    assert 3000 < len(kmers) < 4000 and 15 <= len(walk["head"]) <= 40
    assert route["rounds"] >= 12  # ceil(log2 of the longest path) rounds, then the stall, then the cut cycles again


@pytest.mark.parametrize("k", [31, 33])
def test_path_length_edges(k):
    reads = um.path_edge_reads(k)
    o = Oracle(k, 24 if k == 31 else 16, False)
    o.insert_seqs(*nm.Graph.arrays(reads))
    kmers = nm.oracle_kmers(o)
    assert len(kmers) == sum(um.PATH_LENGTHS) + sum(um.CYCLE_LENGTHS) + 200 + 40
    walk, route, _ = _both(kmers, k)
    lengths = walk["length"].tolist()
    for ln in um.PATH_LENGTHS:
        assert ln in lengths
    assert sorted(walk["length"][walk["flags"] == 1].tolist()) == sorted(um.CYCLE_LENGTHS)  # the cycle of 200 has a read running into it: linear
    assert walk["n_circular"] == 3 and 200 in lengths and 40 in lengths
    assert len(lengths) == len(um.PATH_LENGTHS) + 3 + 2


def test_long_path_and_dense_graph():
    k = 31
    o = Oracle(k, 24, False)
    o.insert_seqs(*nm.Graph.arrays(um.long_path_reads(k)))
    kmers = nm.oracle_kmers(o)
    walk, route, text = _both(kmers, k)
    assert len(kmers) == 70000 and len(walk["head"]) == 1 and walk["n_circular"] == 0
    assert route["rounds"] == 18  # 17 rounds finish a path of 70 000 (2^16 < 69 999 <= 2^17); the count reaches 0 one round later
    assert len(text) == 70000 + 31
    k = 9
    o = Oracle(k, 4, False)
    o.insert_seqs(*nm.Graph.arrays(um.dense_reads()))
    kmers = nm.oracle_kmers(o)
    walk, _, _ = _both(kmers, k)
    assert len(kmers) > 30000 and len(walk["head"]) > 10000 and int(walk["length"].max()) < 100  # a branching graph of short unitigs


@pytest.mark.parametrize("k", [15, 31, 33])
def test_edge_cases_and_the_branch(k):
    pb = {15: 6, 31: 24, 33: 16}[k]
    for kmers, nu, ncirc in (([], 0, 0), ([nm.pack(nm._rand(random.Random(k), k))], 1, 0), ([0], 1, 1)):  # empty; one k-mer; poly-A alone
        walk, _, text = _both(kmers, k)
        assert len(walk["head"]) == nu and walk["n_circular"] == ncirc and len(text) == len(kmers) + nu * k
    assert um.text_model([0], um.walk_model([0], k), k) == b"A" * k + b"\n"
    first, second = um.branch_reads(k)
    o = Oracle(k, pb, False)
    o.insert_seqs(*nm.Graph.arrays(first))
    assert len(um.walk_model(nm.oracle_kmers(o), k)["head"]) == 1
    o.insert_seqs(*nm.Graph.arrays(second))
    walk, _, _ = _both(nm.oracle_kmers(o), k)
    assert sorted(walk["length"].tolist()) == [21, 149, 151]  # up to the branching k-mer, after it, and the branch


def test_unitig_summary():
    S = cbl_amd.CBL.unitig_summary
    s = S([3, 1, 10, 2], [0, 1, 0, 0], 5)
    assert list(s) == ["unitigs", "circular", "kmers", "bases", "longest", "n50"]
    assert s == {"unitigs": 4, "circular": 1, "kmers": 16, "bases": 32, "longest": 10, "n50": 7}  # bases 14, 7, 6, 5: 14 alone is less than half of 32, 14 + 7 = 21 is more
    assert S([10, 3], [0, 0], 5)["n50"] == 14  # 14 of 21
    # the tie: exactly half of the bases sit in the largest unitig — it is the N50 (at least half)
    assert S([8, 2, 2], [0, 0, 0], 5) == {"unitigs": 3, "circular": 0, "kmers": 12, "bases": 24, "longest": 8, "n50": 12}
    assert S([6, 2, 2], [0, 0, 0], 5)["n50"] == 6  # 10 of 22 is short of half
    assert S([6, 6], [0, 0], 5)["n50"] == 10 and S([1, 1], [1, 1], 31) == {"unitigs": 2, "circular": 2, "kmers": 2, "bases": 62, "longest": 1, "n50": 31}
    assert S([], [], 31) == {"unitigs": 0, "circular": 0, "kmers": 0, "bases": 0, "longest": 0, "n50": 0}
    assert S(np.array([4, 4], dtype=np.uint32), np.array([0, 0], dtype=np.uint8), 3) == um.summary_model([4, 4], [0, 0], 3)
    assert all(type(v) is int for v in S(np.array([7], dtype=np.uint32), np.array([1], dtype=np.uint8), 9).values())
    rng = random.Random(1)
    for _ in range(50):
        ls = [rng.randrange(1, 50) for _ in range(rng.randrange(1, 20))]
        fs = [rng.randrange(2) for _ in ls]
        assert S(ls, fs, 7) == um.summary_model(ls, fs, 7)
    with pytest.raises(ValueError):
        S([1, 2], [0], 5)
    with pytest.raises(ValueError):
        S([0], [0], 5)


def test_unitigs_report():
    from cbl_amd.__main__ import unitigs_report

    s = cbl_amd.CBL.unitig_summary([3, 1, 10, 2], [0, 1, 0, 0], 5)
    lines, human = unitigs_report(s)
    assert lines == ["unitigs\t4", "circular\t1", "kmers\t16", "bases\t32", "longest\t10", "n50\t7"]
    assert len(human) == 1 and "4 unitigs (1 circular)" in human[0]


def test_the_unitigs_subcommand_parses(capsys):
    from cbl_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["unitigs", "--help"])
    assert e.value.code == 0
    out = capsys.readouterr().out
    assert "--stats" in out and "--output" in out and "index" in out
    with pytest.raises(SystemExit) as e:
        main(["unitigs"])  # the index is required
    assert e.value.code == 2
    with pytest.raises(SystemExit) as e:
        main(["graph", "--help"])
    assert e.value.code == 0 and "--stats" not in capsys.readouterr().out  # `graph` is as it was


def test_bindings_header_and_kernels_carry_the_new_names():
    with open(os.path.join(ROOT, "include", "cblx.h")) as f:
        header = f.read()
    assert "#define CBLX_ABI_VERSION 3" in header
    note = header[: header.index("#define CBLX_ABI_VERSION 3")]
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    with open(os.path.join(ROOT, "rust", "cblx-sys", "src", "lib.rs")) as f:
        sys_rs = f.read()
    for name, nargs in NEW.items():
        assert name in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES[name][1]) == nargs, name
        assert hasattr(cbl_amd.lib(), name), f"the library built here does not export {name}"
        assert re.search(r"\b%s\b(?!_)" % name, note), f"{name} is not named in the 'Added under 3' note in front of CBLX_ABI_VERSION"
        decl = re.search(r"\bint %s\s*\(([^)]*)\)" % name, body)
        assert decl and len(decl.group(1).split(",")) == nargs, f"{name} is not declared with {nargs} parameters"
        rs = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, sys_rs)
        assert rs and len(rs.group(1).split(",")) == nargs, f"{name} is not declared in the Rust sys crate with {nargs} parameters"
    with open(os.path.join(ROOT, "cbl_amd", "csrc", "kernels_unitig.hpp")) as f:
        ku = f.read()
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, ku), kernel
    assert "asm" not in ku  # plain C++ HIP
    for meth in ("rank_np", "rank_device", "unitig_table_np", "unitig_table_device", "unitigs_text_np", "unitigs", "unitigs_to_file", "unitigs_to_fd",
                 "unitig_summary"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    with open(os.path.join(ROOT, "rust", "cbl-gpu", "src", "lib.rs")) as f:
        facade = f.read()
    assert re.search(r"pub fn rank\b", facade) and re.search(r"pub fn unitig_counts\b", facade) and re.search(r"pub fn unitigs_to_file\b", facade)
