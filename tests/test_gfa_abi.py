"""The link and GFA entry points where the header, the built library, the Python bindings, the Rust crates, the kernel file and the command line carry them."""
import os
import re

import pytest

import cbl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_gfa_links": 8, "cblx_gfa_links_device": 8, "cblx_gfa_text_device": 6, "cblx_gfa_to_fd": 6, "cblx_gfa_to_file": 6}
KERNELS = ("k_gfa_link_counts", "k_gfa_link_fill", "k_gfa_s_bytes", "k_gfa_l_bytes", "k_gfa_s_prefix", "k_gfa_l_text")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_header_library_and_bindings_carry_the_five_symbols():
    header = _read("include", "cblx.h")
    assert "#define CBLX_ABI_VERSION 3" in header  # a new symbol is compatible: the version stays
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
    links = re.search(r"\bint cblx_gfa_links\s*\(([^)]*)\)", body).group(1)
    assert re.search(r"uint64_t\s*\*\s*link_start", links) and re.search(r"uint32_t\s*\*\s*link_to", links) and re.search(r"uint8_t\s*\*\s*link_rev", links)
    facade = _read("rust", "cbl-gpu", "src", "lib.rs")
    assert re.search(r"pub fn gfa_counts\b", facade) and re.search(r"pub fn gfa_to_file\b", facade)


def test_python_surface_and_kernel_file():
    for meth in ("gfa_counts", "gfa_links_np", "gfa_links_device", "gfa_text_device", "gfa_text_np", "gfa_to_file", "gfa_to_fd", "gfa_link_tuples"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    assert list(cbl_amd.CBL.gfa_link_tuples([0, 1, 1, 3], [1, 0, 1], [1, 0, 0])) == [(0, "+", 1, "-"), (1, "+", 0, "+"), (1, "+", 1, "+")]  # host only
    kg = _read("cbl_amd", "csrc", "kernels_gfa.hpp")
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kg), kernel
    assert "asm" not in kg and "atomic" not in kg  # plain C++ HIP, plain stores: every output element has one writer
    # the links keep the masks of the one compaction (no second mask computation), and the S lines' letters come from the unitig text's own launch site
    host = _read("cbl_amd", "csrc", "graph.hpp")
    assert len(re.findall(r"\bneighbor_masks_range\(c, 0, n, masks\.get\(\)", host)) == 1
    assert re.search(r"void unitig_compute\([^)]*bool keep_masks = false\)", host)
    for kernel in ("k_unitig_text", "k_biunitig_text") + KERNELS:
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, host)) == 1, kernel


def test_the_unitigs_command_names_gfa(capsys):
    from cbl_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["unitigs", "--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "--gfa" in out and "--stats" in out
    with pytest.raises(SystemExit) as e:
        main(["-k", "31", "--prefix-bits", "24", "unitigs", "index.cbl", "--gfa", "--stats"])  # refused by the parser, before anything is loaded
    assert e.value.code == 2 and "not allowed with" in capsys.readouterr().err
