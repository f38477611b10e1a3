"""The bidirected-unitig entry points where the header, the built library, the Python bindings, the Rust crates and the kernel file carry them."""
import os
import re

import cbl_amd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = {"cblx_biunitig_table": 12, "cblx_biunitig_table_device": 12, "cblx_biunitigs_text_device": 5, "cblx_biunitigs_to_fd": 5, "cblx_biunitigs_to_file": 5}
KERNELS = ("k_biunitig_links", "k_biunitig_tails", "k_biunitig_keep", "k_biunitig_number", "k_biunitig_text")


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
    table = re.search(r"\bint cblx_biunitig_table\s*\(([^)]*)\)", body).group(1)
    assert re.search(r"uint8_t\s*\*\s*reversed", table)  # reversed is uint8_t[cap_kmers]
    facade = _read("rust", "cbl-gpu", "src", "lib.rs")
    assert re.search(r"pub fn biunitig_counts\b", facade) and re.search(r"pub fn biunitigs_to_file\b", facade)


def test_python_surface_and_kernel_file():
    for meth in ("biunitig_counts", "biunitig_table_np", "biunitig_table_device", "biunitigs_text_device", "biunitigs_text_np", "biunitigs", "biunitigs_to_file",
                 "biunitigs_to_fd", "unitig_summary"):
        assert callable(getattr(cbl_amd.CBL, meth, None)), meth
    kb = _read("cbl_amd", "csrc", "kernels_biunitig.hpp")
    for kernel in KERNELS:
        assert re.search(r"__global__[^;{]*\b%s\(" % kernel, kb), kernel
    assert "asm" not in kb and "atomic" not in kb  # plain C++ HIP, plain stores: every output element has one writer
    # the ranking is section 6k's kernels, unchanged, behind one function; both forms go through one compaction that launches each form's kernels once
    host = "".join(_read("cbl_amd", "csrc", name) for name in ("cblx.cpp", "list.hpp", "graph.hpp"))
    assert len(re.findall(r"^void unitig_rank\(", host, flags=re.M)) == 1 and len(re.findall(r"\bunitig_rank\(c, u, ", host)) == 1
    for kernel in ("k_unitig_jump", "k_unitig_links", "k_biunitig_links", "k_unitig_number", "k_biunitig_number", "k_unitig_text", "k_biunitig_text"):
        assert len(re.findall(r"hipLaunchKernelGGL\(\(?%s\b" % kernel, host)) == 1, kernel


def test_the_unitigs_command_serves_both_forms(capsys):
    import pytest

    from cbl_amd.__main__ import main

    with pytest.raises(SystemExit) as e:
        main(["--help"])
    assert e.value.code == 0
    out = " ".join(capsys.readouterr().out.split())
    assert "of a canonical index the bidirected unitigs" in out
