#!/usr/bin/env python3
"""Times reading an index out on one MI355X: K = 31, PREFIX_BITS = 24, 1 M reads of 150 bases (about 120 M k-mers, 3.8 GB of text), files in /dev/shm.
Recorded, not asserted; the results are in profiles/list_rate.md.

    python tools/dev_list_rate.py [--reads 1000000] [--steps 3] [--dir /dev/shm] [--baseline-main FILE] [--timeout 600]

Rows (wall time around calls that return after the device is done; the range calls include one scan of the bucket lengths, tens of microseconds):
  (a) `python -m cbl_amd list -o` as a child process — and, with --baseline-main, the same command line given to another __main__.py (an earlier
      revision's, to compare; both outputs must be equal byte for byte);
  (b) k_export_range alone into a device buffer, text and packed: cblx_list_range_device / cblx_export_kmers_range_device over the whole index, ms and
      TB/s of its algorithmic bytes (8 B of suffix read + LINE or 8 B written per k-mer) against the 8 TB/s peak; next to it the whole-index
      cblx_export_kmers (k_export_kmers + the download of 8 B per k-mer) and the ranged host export of the same elements (k_export_range + that download);
  (c) list_to_file: the whole call, and its parts measured apart — emit (row b), emit + download (cblx_list_range into host memory), and write() of the
      same bytes from host memory to a file in the same directory;
  (d) cblx_bucket_nodes (kernels + the download of 8 B per bucket).
Every step that touches the GPU runs in a child process under a time limit; nothing is started after one that fails."""
import argparse
import filecmp
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

K, PB, LENGTH = 31, 24, 150


def child(a):
    import numpy as np
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    g = cbl_amd.CBL(K, PB, device=0)
    b, o = synth.reads_torch(42, a.reads, LENGTH, device=dev)
    g.insert_seqs_device(b, o, a.reads)
    del b, o
    n, nb, line = g.count(), g.num_buckets(), K + 1
    out = {"kmers": n, "buckets": nb, "text_bytes": n * line}
    g.save_to_file(a.index)

    def timed(fn, steps=a.steps):
        ms = []
        for _ in range(steps + 1):  # the first call warms up (workspace allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ms[1:]

    d_text = torch.empty(n * line, dtype=torch.uint8, device=dev)
    d_lo = torch.empty(n, dtype=torch.int64, device=dev)
    out["emit_text_ms"] = timed(lambda: g.list_range_device(0, n, d_text, n * line))
    out["emit_packed_ms"] = timed(lambda: g.export_kmers_range_device(0, n, d_lo, None))
    del d_lo
    lo = np.empty(n, dtype=np.uint64)
    out["export_kmers_host_ms"] = timed(lambda: g.kmers_np())
    out["export_range_host_ms"] = timed(lambda: g.export_kmers_range(0, n, lo, None))
    del lo
    host = np.empty(n * line, dtype=np.uint8)
    out["list_range_host_ms"] = timed(lambda: g.list_range(0, n, host))
    assert bytes(host[:line]) == bytes(d_text[:line].cpu().numpy())
    del d_text
    path = os.path.join(a.dir, "dev_list_rate.txt")

    def plain_write():
        with open(path, "wb", buffering=0) as f:
            mv, off = memoryview(host), 0
            while off < len(mv):
                off += f.write(mv[off : off + (64 << 20)])

    out["write_host_to_file_ms"] = timed(plain_write)
    out["list_to_file_ms"] = timed(lambda: g.list_to_file(path))
    assert os.path.getsize(path) == n * line
    with open(path, "rb") as f:
        assert f.read(1 << 20) == host[: 1 << 20].tobytes()
    os.unlink(path)
    del host
    out["bucket_nodes_ms"] = timed(lambda: g.bucket_nodes_np())
    print(json.dumps(out), flush=True)


def run(cmd, timeout):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, timeout=timeout, capture_output=True, text=True, cwd=str(ROOT), env=dict(os.environ, PYTHONPATH=str(ROOT)))
    return r, round(time.perf_counter() - t0, 3)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--baseline-main", help="another revision's cbl_amd/__main__.py, run as a script with the same arguments")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds one child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--index", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    index, txt, txt0 = (os.path.join(a.dir, "dev_list_rate" + s) for s in (".cbl", ".list.txt", ".list0.txt"))
    try:
        r, _ = run([sys.executable, str(Path(__file__).resolve()), "--child", "--index", index, "--reads", str(a.reads), "--steps", str(a.steps), "--dir", a.dir], a.timeout)
        if r.returncode != 0:
            print(json.dumps({"error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
            return 1  # nothing more is started on the GPU after a failure
        out = json.loads(r.stdout.strip().splitlines()[-1])
        args = ["-k", str(K), "--prefix-bits", str(PB), "list", index, "-o"]
        out["cli_list_s"] = []
        for _ in range(a.steps):
            r, s = run([sys.executable, "-m", "cbl_amd"] + args + [txt], a.timeout)
            if r.returncode != 0:
                print(json.dumps({"error": "list: exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
                return 1
            out["cli_list_s"].append(s)
        if a.baseline_main:
            out["cli_list_baseline_s"] = []
            for _ in range(a.steps):
                r, s = run([sys.executable, a.baseline_main] + args + [txt0], a.timeout)
                if r.returncode != 0:
                    print(json.dumps({"error": "baseline list: exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
                    return 1
                out["cli_list_baseline_s"].append(s)
            out["baseline_output_equal"] = filecmp.cmp(txt, txt0, shallow=False)
        n, line = out["kmers"], K + 1
        best = lambda key: min(out[key])  # noqa: E731
        out["emit_text_TBps"] = round(n * (8 + line) / (best("emit_text_ms") * 1e-3) / 1e12, 3)
        out["emit_packed_TBps"] = round(n * 16 / (best("emit_packed_ms") * 1e-3) / 1e12, 3)
        out["list_to_file_GBps"] = round(n * line / (best("list_to_file_ms") * 1e-3) / 1e9, 2)
        out["write_host_to_file_GBps"] = round(n * line / (best("write_host_to_file_ms") * 1e-3) / 1e9, 2)
        print(json.dumps(out), flush=True)
        return 0
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "time limit of %.0f s" % a.timeout}), flush=True)
        return 1
    finally:
        for p in (index, txt, txt0):
            if os.path.exists(p):
                os.unlink(p)


if __name__ == "__main__":
    sys.exit(main())
