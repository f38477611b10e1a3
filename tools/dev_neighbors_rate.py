#!/usr/bin/env python3
"""Times the de Bruijn neighbourhood calls on one MI355X: K = 31, PREFIX_BITS = 24, the index of 1 M reads of 150 bases from cbl_amd.synth (120 M k-mers).
Recorded, not asserted; the results are in profiles/neighbors_rate.md.

    python tools/dev_neighbors_rate.py [--reads 1000000] [--steps 5] [--baseline-kmers 16777216] [--timeout 900]
    python tools/dev_neighbors_rate.py --child --only-degree --steps 3      # nothing but degree_table calls: the run to put under a kernel trace

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process:
  (a) the way to the masks on the parent commit: kmers_np of a range, the eight neighbours by numpy shifts on the host, cblx_contains_kmers of the 8 n neighbours
      (raw ABI on numpy arrays), the flags folded into bytes by numpy. Over the first `--baseline-kmers` k-mers of the iteration order only (the whole index
      is 960 M look-ups fed from the host); reported per k-mer as well, which is what compares with (b);
  (b) neighbors_range_device over the whole index into a device tensor;
  (c) degree_table().
Checked in the same process: (a)'s masks equal the head of (b)'s, and the table of (c) is the histogram of (b)'s masks. The child runs under a time limit;
nothing is started after one that fails."""
import argparse
import json
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
    n = a.reads
    g = cbl_amd.CBL(K, PB, device=0)
    b, o = synth.reads_torch(42, n, LENGTH, device=dev)
    g.insert_seqs_device(b, o, n)
    del b, o
    count = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "reads": n, "index_kmers": count}

    def timed(fn, steps):
        ms = []
        for _ in range(steps + 1):  # the first call warms up (workspace allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ms[1:]

    if a.only_degree:
        out["degree_table_ms"] = timed(g.degree_table, a.steps)
        print(json.dumps(out), flush=True)
        return 0

    m = min(a.baseline_kmers, count)
    mask = (1 << (2 * K)) - 1
    base_masks = np.zeros(m, dtype=np.uint8)

    def baseline():
        lo, _ = g.kmers_np(0, m)
        nb = np.empty((m, 8), dtype=np.uint64)
        for c in range(4):
            nb[:, c] = ((lo << np.uint64(2)) | np.uint64(c)) & np.uint64(mask)
            nb[:, 4 + c] = (lo >> np.uint64(2)) | np.uint64(c << (2 * (K - 1)))
        flags = np.zeros(8 * m, dtype=np.uint8)
        g._chk(g._L.cblx_contains_kmers(g._h, nb.ctypes.data, None, 8 * m, flags.ctypes.data))
        base_masks[:] = np.packbits(flags.reshape(m, 8), axis=1, bitorder="little")[:, 0]

    out["baseline_kmers"] = m
    out["baseline_ms"] = timed(baseline, a.baseline_steps)
    d_masks = torch.empty(count, dtype=torch.uint8, device=dev)
    out["range_device_ms"] = timed(lambda: g.neighbors_range_device(0, count, d_masks), a.steps)
    out["degree_table_ms"] = timed(g.degree_table, a.steps)
    table = g.degree_table()
    masks = d_masks.cpu().numpy()
    assert np.array_equal(masks[:m], base_masks), "the host baseline and the device masks disagree"
    pop = np.array([bin(v).count("1") for v in range(16)], dtype=np.int64)
    want = np.bincount(5 * pop[masks & 15] + pop[masks >> 4], minlength=25).reshape(5, 5)
    assert np.array_equal(table.astype(np.int64), want), "the degree table is not the histogram of the masks"
    out["table"] = table.tolist()
    out["summary"] = cbl_amd.CBL.degree_summary(table)
    out["baseline_ns_per_kmer"] = round(min(out["baseline_ms"]) * 1e6 / m, 3)
    out["range_device_ns_per_kmer"] = round(min(out["range_device_ms"]) * 1e6 / count, 3)
    out["degree_table_ns_per_kmer"] = round(min(out["degree_table_ms"]) * 1e6 / count, 3)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--baseline-kmers", type=int, default=1 << 24, help="k-mers row (a) takes, from the head of the iteration order")
    ap.add_argument("--baseline-steps", type=int, default=2, help="timed steps of row (a): a step is seconds of host work")
    ap.add_argument("--only-degree", action="store_true", help="only degree_table calls (for a kernel trace)")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps), "--baseline-kmers", str(a.baseline_kmers),
           "--baseline-steps", str(a.baseline_steps)] + (["--only-degree"] if a.only_degree else [])
    try:
        r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, cwd=str(ROOT))
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "time limit of %.0f s" % a.timeout}), flush=True)
        return 1
    if r.returncode != 0:
        print(json.dumps({"error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
        return 1
    run = json.loads(r.stdout.strip().splitlines()[-1])
    print(json.dumps(run), flush=True)
    if not a.only_degree:
        f = lambda v: "%.3f – %.3f, best %.3f" % (min(v), max(v), min(v))  # noqa: E731
        print("| row | k-mers | ms | ns per k-mer |\n|---|---|---|---|")
        print("| (a) host baseline | %d | %s | %.3f |" % (run["baseline_kmers"], f(run["baseline_ms"]), run["baseline_ns_per_kmer"]))
        print("| (b) neighbors_range_device | %d | %s | %.3f |" % (run["index_kmers"], f(run["range_device_ms"]), run["range_device_ns_per_kmer"]))
        print("| (c) degree_table | %d | %s | %.3f |" % (run["index_kmers"], f(run["degree_table_ms"]), run["degree_table_ns_per_kmer"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
