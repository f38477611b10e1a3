"""The abundance entry points where the header, the built library, the Python bindings, the Rust crates, the kernel file and the command line carry them."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import cbl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_abundance_seqs": 8, "cblx_abundance_seqs_device": 8, "cblx_abundance_histogram": 4, "cblx_unitig_coverage": 6, "cblx_unitig_coverage_device": 6,
       "cblx_gfa_tagged_text_device": 8, "cblx_gfa_tagged_to_fd": 8, "cblx_gfa_tagged_to_file": 8, "cblx_abundance_filter": 6}
KERNELS = ("k_rank_tally", "k_abundance_compact", "k_abundance_hist", "k_unitig_kc", "k_abundance_select", "k_abundance_unitig_stats", "k_abundance_gather", "k_gfa_s_bytes_tagged",
           "k_gfa_s_tags")
STATS = ("kmers", "removed_kmers", "unitigs", "removed_unitigs", "kmers_left", "min_count")


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
    st = re.search(r"typedef struct cblx_abundance_stats \{\s*uint64_t ([^;]*);\s*\} cblx_abundance_stats;", body)
    assert st and tuple(x.strip() for x in st.group(1).split(",")) == STATS
    assert tuple(n for n, _ in cbl_amd.AbundanceStats._fields_) == STATS and C.sizeof(cbl_amd.AbundanceStats) == 48
    rs = re.search(r"pub struct cblx_abundance_stats \{(.*?)\}", sys_rs, flags=re.S)
    assert rs and tuple(re.findall(r"pub (\w+): u64,", rs.group(1))) == STATS
    assert re.search(r"#define CBLX_ABUNDANCE_UNITIGS 1u\b", body) and "pub const CBLX_ABUNDANCE_UNITIGS: u32 = 1;" in sys_rs and cbl_amd.ABUNDANCE_UNITIGS == 1
    facade = _read("rust", "cbl-gpu", "src", "lib.rs")
    assert re.search(r"pub unsafe fn abundance_filter\b", facade) and "sys::cblx_abundance_filter(" in facade


def test_python_surface_and_kernel_file():
    for meth in ("abundance_seqs", "abundance_seqs_device", "abundance_histogram", "unitig_coverage_np", "unitig_coverage_device", "gfa_tagged_text_np",
                 "gfa_tagged_text_device", "gfa_tagged_to_file", "gfa_tagged_to_fd", "abundance_filter", "solid_threshold"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    ka = _read("cbl_amd", "csrc", "kernels_abundance.hpp")
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, ka), kernel
    assert "asm" not in ka and len(re.findall(r"\batomicCAS\(", ka)) == 1  # plain C++ HIP; the one compare-and-swap is the saturating add's
    # every launch site of the new kernels is in abundance.hpp, and there is one of each; the kernels it borrows keep their single launch site in graph.hpp
    host, graph = _read("cbl_amd", "csrc", "abundance.hpp"), _read("cbl_amd", "csrc", "graph.hpp")
    for kernel in KERNELS:
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, host)) == 1 and not re.search(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, graph), kernel
    for old in ("k_tip_gather", "k_cc_gather", "k_gfa_s_bytes", "k_gfa_s_prefix", "k_gfa_l_bytes", "k_gfa_l_text", "k_unitig_text", "k_biunitig_text", "k_rank"):
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % old, graph)) == 1 and not re.search(r"hipLaunchKernelGGL\(\(?%s\b" % old, host), old
    assert len(re.findall(r"\bremove_words<C>\(", host)) == 1  # the filter's one remove_batch
    assert '#include "abundance.hpp"' in _read("cbl_amd", "csrc", "cblx.cpp")


def test_solid_threshold_on_literals():
    f = cbl_amd.CBL.solid_threshold
    assert f([0, 100, 20, 5, 8, 30, 12]) == 3  # the valley between the error peak and the coverage peak
    assert f([7, 100, 20, 5, 5, 5, 8]) == 3  # a plateau: its first bin
    assert f([0, 5, 9, 4]) == 1  # rising from bin 1: nothing to cut
    assert f([99, 3, 3, 4]) == 1  # bin 0 is not looked at
    assert f([0, 9, 5, 3, 3]) is None and f([0, 4, 4, 4]) is None and f([5]) is None and f([]) is None and f([0] * 256) is None  # never rises again
    import numpy as np

    h = np.zeros(256, dtype=np.uint64)
    h[1:6] = [1000, 300, 40, 90, 400]
    assert f(h) == 3 and isinstance(f(h), int)


def test_the_abundance_command(capsys):
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "abundance", "-h"], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    out = " ".join(r.stdout.decode().split())
    assert "--hist" in out and "--min-count" in out and "--unitigs" in out and "--output" in out and "--gfa" in out and "reads [reads ...]" in out
    from cbl_amd.__main__ import abundance_report, main

    for bad in (["abundance", "index.cbl", "reads.fa", "-o", "out.cbl", "--min-count", "0"], ["abundance", "index.cbl", "reads.fa", "--unitigs"],
                ["abundance", "index.cbl", "reads.fa", "--min-count", "3"], ["abundance", "index.cbl", "reads.fa", "-o", "out.cbl"],
                ["abundance", "index.cbl", "reads.fa", "-o", "out.cbl", "--unitigs"], ["abundance", "index.cbl"]):
        with pytest.raises(SystemExit) as e:
            main(["-k", "31"] + bad)  # refused by the parser, before anything is loaded
        assert e.value.code == 2
        capsys.readouterr()
    hist = [0] * 256
    hist[0], hist[1], hist[2], hist[3], hist[255] = 4, 10, 2, 6, 1
    lines, human = abundance_report(50, 40, hist)
    assert lines == ["total\t50", "found\t40", "kmers\t23", "unseen\t4", "once\t10", "saturated_bin\t1", "solid_threshold\t2"] and len(human) == 3
    assert abundance_report(0, 0, [0] * 256)[0][-1] == "solid_threshold\tnone"
    assert "abundance" in _read("README.md") and "cblx_abundance_filter" in _read("INTEGRATION.md") and "6p" in _read("DESIGN.md")
