"""The fused bit operations of cbl_amd/csrc/necklace.hpp on the host: the same source the HIP kernels compile (there the helpers
and_or / mask_or / bit_select become three-input instructions, here the plain expressions) against the definition, under
AddressSanitizer + UBSan. Exhaustive on rings of 6..20 bits; 62-, 66-, 90- and 118-bit rings on random, sparse, periodic and
degenerate words and on zero runs of exactly 10, 11, 12 and BITS - 1 bits at every position, wrapping ones included."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_necklace_fused_host_unit(tmp_path):
    exe = tmp_path / "necklace_fused_unit"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "host" / "necklace_fused_unit.cpp")], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout, r.stdout
