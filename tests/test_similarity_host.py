"""CPU-side checks of the set-similarity feature (cblx_intersection_count): the arithmetic of CBL.similarity on hand-worked triples, the lines of
`cbl compare`, the presence of the two entry points in the header and in cbl_amd.SIGNATURES, and the route rule of cbl_amd/csrc/common_route.hpp against
a table written out by hand (tests/host/common_route_unit.cpp under AddressSanitizer + UBSan; tests/similarity_shapes.py holds the same rows)."""
import re
import subprocess
from pathlib import Path

import pytest

import cbl_amd
from cbl_amd import CBL
from cbl_amd.__main__ import compare_report

import similarity_shapes as ss  # tests/

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("na,nb,common,exp", [
    (0, 0, 0, dict(common=0, union=0, only_a=0, only_b=0, sym_diff=0, jaccard=1.0, containment_a_in_b=1.0, containment_b_in_a=1.0)),  # both empty
    (0, 7, 0, dict(common=0, union=7, only_a=0, only_b=7, sym_diff=7, jaccard=0.0, containment_a_in_b=1.0, containment_b_in_a=0.0)),  # a empty
    (7, 0, 0, dict(common=0, union=7, only_a=7, only_b=0, sym_diff=7, jaccard=0.0, containment_a_in_b=0.0, containment_b_in_a=1.0)),  # b empty
    (12, 12, 12, dict(common=12, union=12, only_a=0, only_b=0, sym_diff=0, jaccard=1.0, containment_a_in_b=1.0, containment_b_in_a=1.0)),  # identical
    (5, 9, 0, dict(common=0, union=14, only_a=5, only_b=9, sym_diff=14, jaccard=0.0, containment_a_in_b=0.0, containment_b_in_a=0.0)),  # disjoint
    (10, 20, 5, dict(common=5, union=25, only_a=5, only_b=15, sym_diff=20, jaccard=0.2, containment_a_in_b=0.5, containment_b_in_a=0.25)),
    (4, 16, 4, dict(common=4, union=16, only_a=0, only_b=12, sym_diff=12, jaccard=0.25, containment_a_in_b=1.0, containment_b_in_a=0.25)),  # a inside b
    (3 << 40, 1 << 40, 1 << 39, dict(common=1 << 39, union=7 << 39, only_a=5 << 39, only_b=1 << 39, sym_diff=6 << 39, jaccard=1 / 7,
                                     containment_a_in_b=1 / 6, containment_b_in_a=0.5)),  # sizes past 2^32 stay exact integers
])
def test_similarity_hand_worked(na, nb, common, exp):
    got = CBL.similarity(na, nb, common)
    assert set(got) == set(exp)
    for key, v in exp.items():
        if isinstance(v, int):
            assert got[key] == v and isinstance(got[key], int), key
        else:
            assert got[key] == pytest.approx(v, rel=1e-15), key


def test_similarity_refuses_an_impossible_intersection():
    for na, nb, common in ((3, 5, 4), (5, 3, 4), (1, 1, -1)):
        with pytest.raises(ValueError):
            CBL.similarity(na, nb, common)


def test_compare_report_lines():
    counts = [[10, 5, 0], [5, 20, 20], [0, 20, 40]]
    lines, human = compare_report(counts)
    assert lines == [
        "0\t1\t10\t20\t5\t25\t0.200000\t0.500000\t0.250000",
        "0\t2\t10\t40\t0\t50\t0.000000\t0.000000\t0.000000",
        "1\t2\t20\t40\t20\t40\t0.500000\t1.000000\t0.500000",
    ]
    assert len(human) == 3 and all("\t" not in h and "\n" not in h for h in human)
    assert "0 and 1" in human[0] and " 5 " in human[0]
    # an empty index: Jaccard of two empty sets and the containment of an empty set are 1
    lines, _ = compare_report([[0, 0], [0, 0]])
    assert lines == ["0\t1\t0\t0\t0\t0\t1.000000\t1.000000\t1.000000"]
    lines, _ = compare_report([[0, 0], [0, 3]])
    assert lines == ["0\t1\t0\t3\t0\t3\t0.000000\t1.000000\t0.000000"]
    assert compare_report([[4]]) == ([], [])
    import numpy as np

    assert compare_report(np.array(counts, dtype=np.uint64))[0][0] == "0\t1\t10\t20\t5\t25\t0.200000\t0.500000\t0.250000"


def test_entry_points_declared():
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "cblx.h").read_text(), flags=re.S)
    assert re.search(r"int cblx_intersection_count\(cblx_ctx\* a, cblx_ctx\* b, uint64_t\* common, uint64_t\* stats\);", header)
    assert re.search(r"int cblx_intersection_counts\(cblx_ctx\* const\* srcs, uint32_t n, uint64_t\* out\);", header)
    assert re.search(r"#define CBLX_COMMON_STATS 5\b", header)
    for name in ("cblx_intersection_count", "cblx_intersection_counts"):
        assert name in cbl_amd.SIGNATURES
        assert hasattr(cbl_amd.lib(), name)
    assert len(CBL.COMMON_ROUTES) + 1 == 5 and CBL.COMMON_ROUTES == ss.ROUTES
    for meth in ("intersection_count", "set_op_count", "similarity", "jaccard", "containment", "intersection_matrix"):
        assert callable(getattr(CBL, meth))


def test_route_table_and_its_python_mirror():
    text = (ROOT / "cbl_amd" / "csrc" / "common_route.hpp").read_text()
    assert int(re.search(r"COMMON_SMALL = (\d+);", text).group(1)) == ss.COMMON_SMALL
    assert int(re.search(r"COMMON_LDS = (\d+);", text).group(1)) == ss.COMMON_LDS
    assert len(ss.ROUTE_ROWS) >= 80
    for ca, cb, ka, kb, r, stage_a in ss.ROUTE_ROWS:
        assert ss.route(ca, cb, ka, kb) == r, (ca, cb, ka, kb)
        assert stage_a == (1 if ca <= cb else 0)
    # the C++ unit holds the same rows
    unit = (ROOT / "tests" / "host" / "common_route_unit.cpp").read_text()
    names = ("COMMON_WAVE", "COMMON_WG", "COMMON_MERGE", "COMMON_SLICED")
    cpp_rows = [(int(a), int(b), int(c), int(d), names.index(e), int(f)) for a, b, c, d, e, f in
                re.findall(r"\{(\d+)u, (\d+)u, (\d), (\d), (COMMON_[A-Z]+), (\d)\}", unit)]
    assert cpp_rows == [tuple(row) for row in ss.ROUTE_ROWS]


def test_common_route_host_unit(tmp_path):
    """common_route / common_stage_a as the device code compiles them, on every edge of the rule, under AddressSanitizer + UBSan."""
    exe = tmp_path / "common_route_unit"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "host" / "common_route_unit.cpp")], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
