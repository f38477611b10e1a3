"""The tip-clipping entry points where the header, the built library, the Python bindings, the Rust crates, the kernel file and the command line carry them."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import cbl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_unitig_ends": 5, "cblx_unitig_ends_device": 5, "cblx_tips_mark": 6, "cblx_tips_mark_device": 6, "cblx_clip_tips": 5}
KERNELS = ("k_tip_ends", "k_tip_mark", "k_tip_select", "k_tip_gather")
STATS = ("rounds", "tips", "tip_kmers", "isolated", "isolated_kmers", "kmers_left", "fixpoint")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_library_and_bindings_carry_the_five_symbols():
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
    # the struct: seven uint64 in the same order in the header, the Python binding and the Rust crate
    st = re.search(r"typedef struct cblx_clip_stats \{\s*uint64_t ([^;]*);\s*\} cblx_clip_stats;", body)
    assert st and tuple(x.strip() for x in st.group(1).split(",")) == STATS
    assert tuple(n for n, _ in cbl_amd.ClipStats._fields_) == STATS and C.sizeof(cbl_amd.ClipStats) == 56
    rs = re.search(r"pub struct cblx_clip_stats \{(.*?)\}", sys_rs, flags=re.S)
    assert rs and tuple(re.findall(r"pub (\w+): u64,", rs.group(1))) == STATS
    assert re.search(r"#define CBLX_CLIP_ISOLATED 1u\b", body) and "pub const CBLX_CLIP_ISOLATED: u32 = 1;" in sys_rs and cbl_amd.CLIP_ISOLATED == 1
    facade = _read("rust", "cbl-gpu", "src", "lib.rs")
    assert re.search(r"pub fn clip_tips\b", facade) and "sys::cblx_clip_tips(" in facade


def test_python_surface_and_kernel_file():
    for meth in ("unitig_ends_np", "unitig_ends_device", "tips_np", "tip_counts", "tips_mark_device", "clip_tips", "tip_kinds"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    # host only: a tip at the threshold, one over it, an isolated unitig, a unitig linked on both sides
    kinds = cbl_amd.CBL.tip_kinds([3, 4, 3, 1, 3], [0, 0, 0, 0, 0], [0, 0, 0, 2, 1], [1, 1, 0, 1, 0], 3)
    assert kinds.dtype == np.uint8 and kinds.tolist() == [1, 0, 2, 0, 1]
    with pytest.raises(ValueError):
        cbl_amd.CBL.tip_kinds([3], [0], [0], [1], 0)
    with pytest.raises(ValueError):
        cbl_amd.CBL.tip_kinds([3], [1], [0], [1], 3)  # a circular unitig has a link on either side
    kt = _read("cbl_amd", "csrc", "kernels_tips.hpp")
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kt), kernel
    assert "asm" not in kt and len(re.findall(r"\batomicAdd\(", kt)) == 1  # plain C++ HIP; the one atomic is k_tip_mark's, once per workgroup and counter
    # the compaction, the export sweep and the removal are the existing ones; every launch site of the new kernels is new, and there is one of each
    host = _read("cbl_amd", "csrc", "graph.hpp")
    for kernel in KERNELS:
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, host)) == 1, kernel
    assert "unitig_compute(c, u, t.form, true)" in host and re.search(r"remove_words<C>\(c, [^;]*, ns, gstart, false, nullptr\);", host)
    assert len(re.findall(r"\bneighbor_masks_range\(c, 0, n, masks\.get\(\)", host)) == 1


def test_the_clip_command(capsys):
    r = subprocess.run([sys.executable, "-m", "cbl_amd", "clip", "-h"], capture_output=True, cwd=ROOT, timeout=120)
    assert r.returncode == 0, r.stderr
    out = " ".join(r.stdout.decode().split())
    assert "--max-kmers" in out and "--isolated" in out and "--rounds" in out and "--output" in out
    from cbl_amd.__main__ import main

    for bad in (["clip", "index.cbl"], ["clip", "index.cbl", "-o", "out.cbl", "--max-kmers", "0"], ["clip", "index.cbl", "-o", "out.cbl", "--rounds", "-1"]):
        with pytest.raises(SystemExit) as e:
            main(["-k", "31"] + bad)  # refused by the parser, before anything is loaded
        assert e.value.code == 2
        capsys.readouterr()
    assert "clip" in _read("README.md") and "cblx_clip_tips" in _read("INTEGRATION.md")
