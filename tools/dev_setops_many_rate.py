#!/usr/bin/env python3
"""Times cblx_set_op_many (CBL.merge / CBL.intersect) for n = 4 next to the yardstick, the fold of cblx_set_op over the same operands in the same
process: the two operands of `bench.py --config merge` (cfg 5's per-GPU share: K = 31, PREFIX_BITS = 24, 6.25 M reads of 150 bases each from seeds
42 and 43) plus two built the same way from seeds 44 and 45. Recorded, not asserted.

    python tools/dev_setops_many_rate.py [--steps 3] [--warmup 1] [--reads 6250000] [--timeout 300]

Every operation runs in a child process of its own under a time limit (a hung step ends that child and nothing after it is started). A child builds
the four operands, runs the warm-up steps, times the n-ary call and the fold step by step (wall time: the calls return synchronised) and prints one
JSON line with both, and with the stage timers of both taken in one more step each on a profiling context. After the first step the operands' Vec
buckets are sorted, so later steps sort sorted runs, in both forms alike."""
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

OPS = ("or", "and")
SEEDS = (42, 43, 44, 45)


def child(a):
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    k, pb, length = 31, 24, 150
    xs = []
    for seed in SEEDS:
        bases, offsets = synth.reads_torch(seed, a.reads, length, first_read=0, device=dev)
        x = cbl_amd.CBL(k, pb, device=0)
        x.insert_seqs_device(bases, offsets, a.reads)
        xs.append(x)
        del bases, offsets
    work = cbl_amd.CBL(k, pb, device=0, profile=True)
    t1, t2 = cbl_amd.CBL(k, pb, device=0, profile=True), cbl_amd.CBL(k, pb, device=0, profile=True)
    out = {"op": a.child, "words": [x.count() for x in xs], "many_ms": [], "fold_ms": []}

    def many():
        (cbl_amd.CBL.merge if a.child == "or" else cbl_amd.CBL.intersect)(xs, out=work)

    def fold():
        cbl_amd.CBL.set_op(xs[0], xs[1], a.child, out=t1)
        cbl_amd.CBL.set_op(t1, xs[2], a.child, out=t2)
        cbl_amd.CBL.set_op(t2, xs[3], a.child, out=t1)

    def stages(ctxs):
        s = {}
        for c in ctxs:
            for name, (t, n) in c.stage_times().items():
                if n:
                    s[name] = round(s.get(name, 0.0) + t, 3)
        return s

    for what, step, ctxs in (("many", many, [work]), ("fold", fold, [t1, t2])):
        for i in range(a.warmup + a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            if i >= a.warmup:
                out[what + "_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
        for c in ctxs:
            c.stage_times_reset()
        step()
        out[what + "_stage_ms"] = stages(ctxs)
    out["many_words_out"], out["many_buckets_out"] = work.count(), work.num_buckets()
    out["fold_words_out"], out["fold_buckets_out"] = t1.count(), t1.num_buckets()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=6_250_000)
    ap.add_argument("--timeout", type=float, default=300.0, help="seconds one operation's child may take")
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
