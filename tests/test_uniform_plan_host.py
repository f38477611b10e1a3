"""The arithmetic chunk plan of cbl_amd/csrc/uniform_plan.hpp on the host: the formulas KRN-1 computes for reads of one length
(chunk_start, kmer_off, tile_first) against a restatement of the table kernels' definition, under AddressSanitizer + UBSan.
K = 5, 21, 31, 59; offsets[0] at every residue mod 16; L = K, K + 1, 64, 150, K + 2047 (2048 k-mers: the largest single chunk) and
K + 2048 (two chunks: not arithmetic); 1, 2, 27, 28, 29 and 1000 sequences; a last tile that holds no chunk start; 3000 random shapes."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_uniform_plan_host_unit(tmp_path):
    exe = tmp_path / "uniform_plan_unit"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "host" / "uniform_plan_unit.cpp")], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout, r.stdout
