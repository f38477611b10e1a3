#!/usr/bin/env python3
"""Times the assigning set operations of cblx_set_op_assign (`a &= b`, `a -= b`, `a ^= b`) next to their yardstick, cblx_set_op with the same op on the
same operands (the same sorts, then the merge rounds in place of the lookups and the swap_remove layout), on the operands of `bench.py --config merge` (cfg 5's per-GPU
share: K = 31, PREFIX_BITS = 24, 6.25 M reads of 150 bases each). Recorded, not asserted.

    python tools/dev_setops_assign_rate.py [--steps 3] [--warmup 1] [--reads 6250000] [--timeout 240]

Two pairs of operands: `disjoint` (reads of seeds 42 and 43: no shared k-mer, so `&=` deletes everything) and `half` (b holds the second half of a's
reads and as many of its own). Every (pair, op) runs in a child process of its own under a time limit (a hung step ends that child and nothing after it
is started). A child builds the operands, then times cblx_set_op into a third index and cblx_set_op_assign on a fresh clone of a per step — the clone
(`|=` into an empty index) is made outside the timed region — and prints one JSON line: ms per step, and the stage timers of both forms
(`bucket_medium` + `bucket_huge`: the in-arena sorts of both forms; `bucket_big`: k_bucket_setop, the merge rounds; `bucket_small`: k_bucket_setop_assign, whose
lookups, pushed words and layout share one kernel and so one timer — the layout's own share is what `bucket_small` costs beyond `bucket_big` of the yardstick)."""
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

OPS = ("and", "sub", "xor")
PAIRS = ("disjoint", "half")


def child(a):
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    k, pb, length = 31, 24, 150
    A, B, work = cbl_amd.CBL(k, pb, device=0), cbl_amd.CBL(k, pb, device=0), cbl_amd.CBL(k, pb, device=0, profile=True)
    ab, ao = synth.reads_torch(42, a.reads, length, first_read=0, device=dev)
    A.insert_seqs_device(ab, ao, a.reads)
    if a.pair == "disjoint":
        bb, bo = synth.reads_torch(43, a.reads, length, first_read=0, device=dev)
        B.insert_seqs_device(bb, bo, a.reads)
    else:  # the second half of a's reads, then as many of b's own
        half = a.reads // 2
        sb_, so = synth.reads_torch(42, half, length, first_read=a.reads - half, device=dev)
        B.insert_seqs_device(sb_, so, half)
        bb, bo = synth.reads_torch(43, a.reads - half, length, first_read=0, device=dev)
        B.insert_seqs_device(bb, bo, a.reads - half)
    out = {"pair": a.pair, "op": a.child, "words_a": A.count(), "words_b": B.count(), "set_op_ms": [], "assign_ms": []}

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

    stages = {}
    for i in range(a.warmup + a.steps):
        work.stage_times_reset()
        ms = timed(lambda: cbl_amd.CBL.set_op(A, B, a.child, out=work))
        if i >= a.warmup:
            out["set_op_ms"].append(ms)
            add_stages(work, stages)
    out["set_op_stage_ms"] = stages
    out["words_out"] = work.count()
    work.clear()
    stages = {}
    for i in range(a.warmup + a.steps):
        c = cbl_amd.CBL(k, pb, device=0, profile=True)
        c |= A  # every bucket cloned as stored; A's Vecs on shared prefixes were sorted by the steps above, as the yardstick found them from step 2 on
        c.stage_times_reset()
        ms = timed(lambda: c.set_op_assign(B, a.child))
        if i >= a.warmup:
            out["assign_ms"].append(ms)
            add_stages(c, stages)
        out["assign_words_out"] = c.count()
        c.close()
    out["assign_stage_ms"] = stages
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=6_250_000)
    ap.add_argument("--timeout", type=float, default=240.0, help="seconds one child may take")
    ap.add_argument("--ops", default=",".join(OPS))
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--child", choices=OPS, help=argparse.SUPPRESS)
    ap.add_argument("--pair", choices=PAIRS, default="disjoint", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for pair in a.pairs.split(","):
        for op in a.ops.split(","):
            cmd = [sys.executable, str(Path(__file__).resolve()), "--child", op, "--pair", pair, "--steps", str(a.steps), "--warmup", str(a.warmup), "--reads", str(a.reads)]
            try:
                r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=dict(os.environ))
            except subprocess.TimeoutExpired:
                print(json.dumps({"pair": pair, "op": op, "error": "time limit of %.0f s" % a.timeout}), flush=True)
                return 1
            if r.returncode != 0:
                print(json.dumps({"pair": pair, "op": op, "error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
                return 1  # nothing more is started on the GPU after a failure
            print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
