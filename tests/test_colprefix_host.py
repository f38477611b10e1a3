"""The two-level column prefixes of cbl_amd/csrc/colprefix.hpp on the host: the same source the partition kernels compile (the
super-tile scan of the producers, the accessor of the scatter / k_seg_adjust / k_dir_gather) against a flat exclusive column prefix
and the column totals, under AddressSanitizer + UBSan. 0, 1, 15, 16, 17, 31, 32, 33 and 1000 tiles; random and skewed counts with a
ragged last tile; every record of 16 full tiles in one column (local prefix 61 440); all-zero rows."""
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_colprefix_host_unit(tmp_path):
    exe = tmp_path / "colprefix_unit"
    subprocess.run(["g++", "-O2", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "host" / "colprefix_unit.cpp")], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "bad=0" in r.stdout, r.stdout
