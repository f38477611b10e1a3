#!/usr/bin/env python3
"""Times the batch query on one MI355X in its three forms: K = 31, PREFIX_BITS = 24, 1 M reads of 150 bases from cbl_amd.synth (120 M queries) against the
index of those reads, with every second read replaced by a random one so that both outcomes occur. Recorded, not asserted; the results are in
profiles/query_counts_rate.md.

    python tools/dev_query_counts_rate.py [--reads 1000000] [--steps 5] [--rounds 2] [--parent-lib FILE] [--timeout 600]

Rows (wall time around calls that return after the device is done; reads, offsets and outputs are device tensors), all of one library in one process:
  (a) tallies only: cblx_contains_seqs_device without a flag tensor (the join without ordinals);
  (b) flags: cblx_contains_seqs_device into a device flag tensor (the join with ordinals);
  (c) per-sequence counts: cblx_contains_seqs_counts_device (the flags of (b) into device scratch + k_chunk_tally + k_seq_tally);
  (d) counts and flags: cblx_contains_seqs_flags_counts_device into the flag tensor of (b): (d) - (b) is the tally pass, (c) - (d) the scratch.
--parent-lib: a libcblx.so built from the parent commit, loaded through CBLX_LIB_PATH in a process of its own for rows (a) and (b); the two libraries take
turns, `--rounds` times, so that a drift of the box shows. Every process that touches the GPU runs under a time limit; nothing is started after one that fails."""
import argparse
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
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    n = a.reads
    g = cbl_amd.CBL(K, PB, device=0)
    b, o = synth.reads_torch(42, n, LENGTH, device=dev)
    g.insert_seqs_device(b, o, n)
    b2, _ = synth.reads_torch(4242, n, LENGTH, device=dev)
    b[: n * LENGTH].view(n, LENGTH)[1::2] = b2[: n * LENGTH].view(n, LENGTH)[1::2]  # every second read: random, (nearly) nothing of it is found
    del b2
    nk = n * (LENGTH - K + 1)
    out = {"lib": str(cbl_amd.LIB_PATH), "reads": n, "queries": nk, "index_kmers": g.count()}

    def timed(fn):
        ms = []
        for _ in range(a.steps + 1):  # the first call warms up (workspace allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ms[1:]

    d_f = torch.empty(nk, dtype=torch.uint8, device=dev)
    tallies = g.contains_seqs_device(b, o, n)
    assert tallies[0] == nk and 0 < tallies[1] < nk
    out["positive"] = tallies[1]
    out["tallies_ms"] = timed(lambda: g.contains_seqs_device(b, o, n))
    out["flags_ms"] = timed(lambda: g.contains_seqs_device(b, o, n, d_f, nk))
    assert int(d_f.sum(dtype=torch.int64)) == tallies[1]
    if hasattr(g._L, "cblx_contains_seqs_counts_device"):
        d_t = torch.empty(n, dtype=torch.int32, device=dev)
        d_p = torch.empty(n, dtype=torch.int32, device=dev)
        out["counts_ms"] = timed(lambda: g.contains_seqs_counts_device(b, o, n, d_t, d_p))
        assert (int(d_t.sum(dtype=torch.int64)), int(d_p.sum(dtype=torch.int64))) == tallies
        assert bool((d_p[::2] == LENGTH - K + 1).all())  # the reads of the index are found whole
        out["counts_and_flags_ms"] = timed(lambda: g.contains_seqs_counts_device(b, o, n, d_t, d_p, d_flags=d_f))
        assert (int(d_p.sum(dtype=torch.int64)), int(d_f.sum(dtype=torch.int64))) == (tallies[1], tallies[1])
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--parent-lib", help="libcblx.so of the parent commit (rows a and b)")
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds one child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps)]
    runs = []
    try:
        for _ in range(a.rounds):
            for lib in ([a.parent_lib] if a.parent_lib else []) + [None]:
                env = dict(os.environ, PYTHONPATH=str(ROOT))
                env.pop("CBLX_LIB_PATH", None)
                if lib:
                    env["CBLX_LIB_PATH"] = str(Path(lib).resolve())
                r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, cwd=str(ROOT), env=env)
                if r.returncode != 0:
                    print(json.dumps({"error": "exit %d" % r.returncode, "lib": lib or "this tree", "stderr": r.stderr[-2000:], "runs": runs}), flush=True)
                    return 1  # nothing more is started on the GPU after a failure
                run = json.loads(r.stdout.strip().splitlines()[-1])
                run["which"] = "parent" if lib else "this tree"
                runs.append(run)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "time limit of %.0f s" % a.timeout, "runs": runs}), flush=True)
        return 1
    best = {}
    for run in runs:
        for key in ("tallies_ms", "flags_ms", "counts_ms", "counts_and_flags_ms"):
            if key in run:
                k2 = run["which"] + " " + key
                best[k2] = min(best.get(k2, float("inf")), min(run[key]))
    print(json.dumps({"runs": runs, "best_ms": best}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
