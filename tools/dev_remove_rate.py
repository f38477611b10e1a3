#!/usr/bin/env python3
"""Times cblx_remove_seqs_device next to its two yardsticks on one MI355X, on cfg 2's index (K = 31, PREFIX_BITS = 24, 10 M reads of 150 bases). Recorded,
not asserted; the results are in profiles/remove_rate.md.

    python tools/dev_remove_rate.py [--steps 3] [--warmup 1] [--reads 10000000] [--timeout 400]

Two workloads, each in a child process of its own under a time limit (a hung step ends that child and nothing after it is started):
  `half`   the second half of the index's reads is removed;
  `copies` as many reads, all copies of 64 distinct ones of that half (the repetitive case: 64 x 120 effective removals among 600 M removal words).
A child builds the index once, then per step clones it (`|=` into an empty index, outside the timed region) and times the removal: wall ms and the stage
timers (`directory`: visit, group scan, slot offsets, tail; `bucket_remove`: hash table, probe, replay; `merge_gather`: the compacted arena). In the same
process: (a) the build of the removed reads into an empty index, (b) `a -= b` (cblx_set_op_assign, SUB) on a fresh clone with b built from those reads."""
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

WORKLOADS = ("half", "copies")


def child(a):
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    k, pb, length = 31, 24, 150
    half = a.reads // 2
    A = cbl_amd.CBL(k, pb, device=0)
    ab, ao = synth.reads_torch(42, a.reads, length, first_read=0, device=dev)
    A.insert_seqs_device(ab, ao, a.reads)
    del ab, ao
    rb, ro = synth.reads_torch(42, half, length, first_read=a.reads - half, device=dev)
    if a.child == "copies":
        idx = torch.arange(half, device=dev) % 64
        rb = torch.cat([rb[: 64 * length].view(64, length)[idx].reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    out = {"workload": a.child, "words_index": A.count(), "reads_removed": half, "remove_ms": [], "build_ms": [], "sub_ms": []}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 3)

    def add_stages(ctx, into):
        for name, (t, n) in ctx.stage_times().items():
            if n:
                into.setdefault(name, []).append(round(t, 3))

    def clone():
        c = cbl_amd.CBL(k, pb, device=0, profile=True)
        c |= A
        c.stage_times_reset()
        return c

    stages = {}
    for i in range(a.warmup + a.steps):
        c = clone()
        ms = timed(lambda: c.remove_seqs_device(rb, ro, half))
        if i >= a.warmup:
            out["remove_ms"].append(ms)
            add_stages(c, stages)
        out["words_left"] = c.count()
        c.close()
    out["remove_stage_ms"] = stages
    stages = {}
    B = None
    for i in range(a.warmup + a.steps):  # (a) the build of the same reads
        if B is not None:
            B.close()
        B = cbl_amd.CBL(k, pb, device=0, profile=True)
        ms = timed(lambda: B.insert_seqs_device(rb, ro, half))
        if i >= a.warmup:
            out["build_ms"].append(ms)
            add_stages(B, stages)
    out["build_stage_ms"] = stages
    out["words_b"] = B.count()
    stages = {}
    for i in range(a.warmup + a.steps):  # (b) a -= b
        c = clone()
        ms = timed(lambda: c.set_op_assign(B, "sub"))
        if i >= a.warmup:
            out["sub_ms"].append(ms)
            add_stages(c, stages)
        out["sub_words_left"] = c.count()
        c.close()
    out["sub_stage_ms"] = stages
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds one child may take")
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--child", choices=WORKLOADS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for w in a.workloads.split(","):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", w, "--steps", str(a.steps), "--warmup", str(a.warmup), "--reads", str(a.reads)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=dict(os.environ))
        except subprocess.TimeoutExpired:
            print(json.dumps({"workload": w, "error": "time limit of %.0f s" % a.timeout}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"workload": w, "error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
            return 1  # nothing more is started on the GPU after a failure
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
