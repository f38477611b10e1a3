#!/usr/bin/env python3
"""Times the set operations of cblx_set_op on the two operands of `bench.py --config merge` (cfg 5's per-GPU share: K = 31, PREFIX_BITS = 24,
6.25 M reads of 150 bases each from seeds 42 and 43), next to the yardstick: cblx_merge_from on the same operands. Recorded, not asserted.

    python tools/dev_setops_rate.py [--steps 3] [--warmup 1] [--reads 6250000] [--timeout 120]

Every operation runs in a child process of its own under a time limit (a hung step ends that child and nothing after it is started); a child
builds the operands, runs the warm-up steps and prints one JSON line with the time of every step in ms (device work and the call's host part:
cblx_set_op returns synchronised). To time the yardstick on another build of the library, run with CBLX_LIB_PATH=<that libcblx.so> --ops merge_from.
"""
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

OPS = ("merge_from", "or", "and", "sub", "xor")


def child(a):
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    k, pb, length = 31, 24, 150
    ab, ao = synth.reads_torch(42, a.reads, length, first_read=0, device=dev)
    bb, bo = synth.reads_torch(43, a.reads, length, first_read=0, device=dev)
    A, B, work = cbl_amd.CBL(k, pb, device=0), cbl_amd.CBL(k, pb, device=0), cbl_amd.CBL(k, pb, device=0)
    A.insert_seqs_device(ab, ao, a.reads)
    B.insert_seqs_device(bb, bo, a.reads)
    out = {"op": a.child, "words_a": A.count(), "words_b": B.count(), "ms": []}

    def step():
        if a.child == "merge_from":
            work.merge_from(A, B)
        else:
            cbl_amd.CBL.set_op(A, B, a.child, out=work)

    for i in range(a.warmup + a.steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        if i >= a.warmup:
            out["ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
    out["words_out"] = work.count()
    out["buckets_out"] = work.num_buckets()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=6_250_000)
    ap.add_argument("--timeout", type=float, default=120.0, help="seconds one operation's child may take")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--child", choices=OPS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for op in a.ops.split(","):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", op, "--steps", str(a.steps), "--warmup", str(a.warmup), "--reads", str(a.reads)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=dict(os.environ))
        except subprocess.TimeoutExpired:
            print(json.dumps({"op": op, "error": "time limit of %.0f s" % a.timeout}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"op": op, "error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
            return 1  # nothing more is started on the GPU after a failure
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
