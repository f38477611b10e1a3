"""The bubble entry points where the header, the built library, the Python bindings, the Rust crates, the kernel file and the command line carry them."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cbl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_bubbles_mark": 8, "cblx_bubbles_mark_device": 8, "cblx_pop_bubbles": 7}
KERNELS = ("k_bubble_left", "k_bubble_mark", "k_bubble_select", "k_bubble_gather", "k_counts_scatter")
STATS = ("rounds", "bubbles", "popped", "popped_kmers", "kmers_left", "fixpoint")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_library_and_bindings_carry_the_symbols():
    header = _read("include", "cblx.h")
    assert "#define CBLX_ABI_VERSION 3" in header and cbl_amd.lib().cblx_abi_version() == 3  # a new symbol is compatible: the version stays
    note = header[: header.index("#define CBLX_ABI_VERSION 3")]
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    sys_rs = _read("rust", "cblx-sys", "src", "lib.rs")
    for name, nargs in NEW.items():
        assert re.search(r"\b%s\b(?!_)" % name, note), f"{name} is not named in the 'Added under 3' note in front of CBLX_ABI_VERSION"
        decl = re.search(r"\bint %s\s*\(([^)]*)\)" % name, body)
        assert decl and len(decl.group(1).split(",")) == nargs, f"{name} is not declared with {nargs} parameters"
        assert hasattr(cbl_amd.lib(), name), f"the library built here does not export {name}"
        assert name in cbl_amd.SIGNATURES and len(cbl_amd.SIGNATURES[name][1]) == nargs, name
        rs = re.search(r"pub fn %s\s*\(([^)]*)\)" % name, sys_rs)
        assert rs and len(rs.group(1).split(",")) == nargs, f"{name} is not declared in the Rust sys crate with {nargs} parameters"
    # the struct: six uint64 in the same order in the header, the Python binding and the Rust crate
    assert "cblx_bubble_stats" in note
    st = re.search(r"typedef struct cblx_bubble_stats \{\s*uint64_t ([^;]*);\s*\} cblx_bubble_stats;", body)
    assert st and tuple(x.strip() for x in st.group(1).split(",")) == STATS
    assert tuple(n for n, _ in cbl_amd.BubbleStats._fields_) == STATS and C.sizeof(cbl_amd.BubbleStats) == 48
    assert cbl_amd.BUBBLE_COUNTS == ("bubbles", "popped", "popped_kmers")
    rs = re.search(r"pub struct cblx_bubble_stats \{(.*?)\}", sys_rs, flags=re.S)
    assert rs and tuple(re.findall(r"pub (\w+): u64,", rs.group(1))) == STATS
    facade = _read("rust", "cbl-gpu", "src", "lib.rs")
    assert re.search(r"pub unsafe fn pop_bubbles\b", facade) and "sys::cblx_pop_bubbles(" in facade


def test_python_surface_and_kernel_file():
    for meth in ("bubbles_np", "bubbles_mark_device", "bubble_counts", "pop_bubbles", "bubble_kinds"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    kb = _read("cbl_amd", "csrc", "kernels_bubbles.hpp")
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kb), kernel
    assert "asm" not in kb and "atomicCAS" not in kb and len(re.findall(r"\batomicAdd\(", kb)) == 1  # plain C++ HIP; the one atomic is the counters'
    # every launch site of the new kernels is in bubbles.hpp, and there is one of each; the older files launch none of them
    host = _read("cbl_amd", "csrc", "bubbles.hpp")
    graph, abundance = _read("cbl_amd", "csrc", "graph.hpp"), _read("cbl_amd", "csrc", "abundance.hpp")
    for kernel in KERNELS:
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, host)) == 1, kernel
        assert not re.search(r"\b%s\b" % kernel, graph) and not re.search(r"\b%s\b" % kernel, abundance), kernel
    # the kernels it borrows keep their launch sites where they were: bubbles.hpp calls the functions around them
    for old in ("k_tip_select", "k_tip_gather", "k_tip_ends", "k_tip_mark", "k_gfa_link_counts", "k_gfa_link_fill", "k_rank", "k_unitig_kc", "k_abundance_gather"):
        assert not re.search(r"hipLaunchKernelGGL\(\(?%s\b" % old, host), old
    for called in ("gfa_count(", "gfa_fill(", "kc_of_table(", "export_passes(", "rank_kmers_device<", "exclusive_scan<u32>("):
        assert called in host, called
    assert len(re.findall(r"\bremove_words<C>\(", host)) == 1  # a round's one remove_batch
    cpp = _read("cbl_amd", "csrc", "cblx.cpp")
    assert cpp.index('#include "abundance.hpp"') < cpp.index('#include "bubbles.hpp"')


def test_bubble_kinds_on_literals():
    f = cbl_amd.CBL.bubble_kinds
    # plain form, 4 unitigs: 0 -> {1, 2} -> 3. Slots 2 u; the odd slots hold nothing
    start = np.array([0, 2, 2, 3, 3, 4, 4, 4, 4], dtype=np.uint64)
    to, rev = np.array([1, 2, 3, 3], dtype=np.uint32), np.zeros(4, dtype=np.uint8)
    left = np.array([0, 1, 1, 2], dtype=np.uint8)
    assert f(start, to, rev, [9, 5, 6, 9], left, None, 6).tolist() == [0, 1, 2, 0]  # the longer arm is kept
    assert f(start, to, rev, [9, 5, 5, 9], left, None, 6).tolist() == [0, 2, 1, 0]  # equal lengths: the lower number
    assert f(start, to, rev, [9, 5, 6, 9], left, None, 5).tolist() == [0, 0, 0, 0]  # one arm over max_kmers: a group of one
    assert f(start, to, rev, [9, 5, 6, 9], left, [0, 11, 13, 0], 6).tolist() == [0, 2, 1, 0]  # 11 / 5 > 13 / 6
    assert f(start, to, rev, [9, 5, 6, 9], left, [0, 10, 12, 0], 6).tolist() == [0, 1, 2, 0]  # equal means: the longer
    big = (1 << 32) - 1
    assert f(start, to, rev, [9, 299, 300, 9], left, [0, 299 * big, 300 * big - 1, 0], 300).tolist() == [0, 2, 1, 0]  # exact in integers
    assert f(start, to, rev, [9, 5, 6, 9], np.array([0, 2, 1, 2], dtype=np.uint8), None, 6).tolist() == [0, 0, 0, 0]  # a second way into an arm
    # bidirected form, the same graph with its mirror links: 3- -> {1-, 2-} -> 0-
    start = np.array([0, 2, 2, 3, 4, 5, 6, 6, 8], dtype=np.uint64)
    to = np.array([1, 2, 3, 0, 3, 0, 1, 2], dtype=np.uint32)
    rev = np.array([0, 0, 0, 1, 0, 1, 1, 1], dtype=np.uint8)
    assert f(start, to, rev, [9, 5, 6, 9], None, None, 6).tolist() == [0, 1, 2, 0]
    assert f(start, to, rev, [9, 5, 6, 9], None, [0, 11, 13, 0], 6).tolist() == [0, 2, 1, 0]
    with pytest.raises(ValueError):
        f(start, to, rev, [9, 5, 6, 9], None, None, 0)


def test_the_pop_command(capsys):
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "pop", "-h"], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    out = " ".join(r.stdout.decode().split())
    assert "--max-kmers" in out and "--rounds" in out and "--output" in out and "[reads ...]" in out and "2 K" in out
    from cbl_amd.__main__ import main

    for bad in (["pop", "index.cbl"], ["pop", "index.cbl", "-o", "out.cbl", "--max-kmers", "0"], ["pop", "index.cbl", "reads.fa", "-o", "out.cbl", "--rounds", "-1"],
                ["pop", "-o", "out.cbl"], ["pop", "index.cbl", "-o", "out.cbl", "--isolated"]):
        with pytest.raises(SystemExit) as e:
            main(["-k", "31"] + bad)  # refused by the parser, before anything is loaded
        assert e.value.code == 2
        capsys.readouterr()
    assert "`pop`" in _read("README.md") and "cblx_pop_bubbles" in _read("INTEGRATION.md") and "6q" in _read("DESIGN.md")
