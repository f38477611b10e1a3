"""The connected-component entry points where the header, the built library, the Python bindings, the Rust crates, the kernel file and the command line carry
them."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

import cbl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_components": 10, "cblx_components_device": 10, "cblx_components_filter": 4}
KERNELS = ("k_cc_init", "k_cc_hook", "k_cc_jump", "k_cc_roots", "k_cc_number", "k_cc_sizes", "k_cc_kmer", "k_cc_keep", "k_cc_select", "k_cc_gather")
STATS = ("components", "removed_components", "removed_kmers", "kmers_left", "largest_kmers", "rounds")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_library_and_bindings_carry_the_three_symbols():
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
    st = re.search(r"typedef struct cblx_component_stats \{\s*uint64_t ([^;]*);\s*\} cblx_component_stats;", body)
    assert st and tuple(x.strip() for x in st.group(1).split(",")) == STATS
    assert tuple(n for n, _ in cbl_amd.ComponentStats._fields_) == STATS and C.sizeof(cbl_amd.ComponentStats) == 48
    rs = re.search(r"pub struct cblx_component_stats \{(.*?)\}", sys_rs, flags=re.S)
    assert rs and tuple(re.findall(r"pub (\w+): u64,", rs.group(1))) == STATS
    assert re.search(r"#define CBLX_COMPONENTS_LARGEST 1u\b", body) and "pub const CBLX_COMPONENTS_LARGEST: u32 = 1;" in sys_rs and cbl_amd.COMPONENTS_LARGEST == 1
    facade = _read("rust", "cbl-gpu", "src", "lib.rs")
    assert re.search(r"pub fn component_counts\b", facade) and "sys::cblx_components(" in facade
    assert re.search(r"pub fn components_filter\b", facade) and "sys::cblx_components_filter(" in facade


def test_python_surface_and_kernel_file():
    for meth in ("component_counts", "components_np", "components_device", "components_filter", "component_summary"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    # host only: a largest component of 6 of 12 k-mers, two components of one unitig
    sm = cbl_amd.CBL.component_summary([3, 6, 1, 2], [1, 4, 1, 2])
    assert sm == {"components": 4, "largest": 6, "singletons": 2, "largest_fraction": 0.5}
    assert cbl_amd.CBL.component_summary([], []) == {"components": 0, "largest": 0, "singletons": 0, "largest_fraction": 0.0}
    for bad in (([3], [1, 1]), ([0], [1]), ([2], [3])):  # lengths differ; an empty component; fewer k-mers than unitigs
        with pytest.raises(ValueError):
            cbl_amd.CBL.component_summary(*bad)
    kc = _read("cbl_amd", "csrc", "kernels_components.hpp")
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kc), kernel
    assert "asm" not in kc and len(re.findall(r"\batomicMin\(", kc)) == 1  # plain C++ HIP; the one min is the hook's
    # the link table, the export sweep and the removal are the existing ones; every launch site of the new kernels is in graph.hpp, and there is one of each
    host = _read("cbl_amd", "csrc", "graph.hpp")
    for kernel in KERNELS:
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, host)) == 1, kernel
    for old in ("k_tip_gather", "k_tip_select", "k_gfa_l_bytes", "k_gfa_link_fill", "k_gfa_link_counts"):
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % old, host)) == 1, old  # the existing kernels keep their single launch site
    assert "gfa_count(c, g);" in host and "gfa_fill(c, g, link_to.get(), nullptr)" in host
    assert len(re.findall(r"remove_words<C>\(c, [^;]*, ns, gstart, false, nullptr\);", host)) == 2  # a round of clip_tips, and the filter


def test_the_components_command(capsys):
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "components", "-h"], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    out = " ".join(r.stdout.decode().split())
    assert "--sizes" in out and "--min-kmers" in out and "--largest" in out and "--output" in out
    from cbl_amd.__main__ import main

    for bad in (["components", "index.cbl", "-o", "out.cbl", "--min-kmers", "0"], ["components", "index.cbl", "-o", "out.cbl", "--min-kmers", "5", "--largest"],
                ["components", "index.cbl", "--min-kmers", "5"], ["components", "index.cbl", "--largest"], ["components", "index.cbl", "-o", "out.cbl"]):
        with pytest.raises(SystemExit) as e:
            main(["-k", "31"] + bad)  # refused by the parser, before anything is loaded
        assert e.value.code == 2
        capsys.readouterr()
    assert "components" in _read("README.md") and "cblx_components_filter" in _read("INTEGRATION.md") and "6o" in _read("DESIGN.md")
