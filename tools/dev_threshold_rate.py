#!/usr/bin/env python3
"""Times CBL.at_least(t = 2) and CBL.occupancy for n = 4 next to the yardsticks, CBL.merge and CBL.intersect of the same operands, in ONE process,
alternating: the two operands of `bench.py --config merge` (cfg 5's per-GPU share: K = 31, PREFIX_BITS = 24, 6.25 M reads of 150 bases each from
seeds 42 and 43) plus two built the same way from seeds 44 and 45. Recorded, not asserted.

    python tools/dev_threshold_rate.py [--steps 3] [--warmup 1] [--reads 6250000] [--timeout 600]

The work runs in a child process under a time limit (a hung step ends the child and nothing after it is started). The child builds the four operands,
then runs warm-up + steps rounds of (merge, intersect, at_least(2), occupancy) — wall time per call: the calls return synchronised — and one more
round with the stage timers read after each call. It also reports, from the operands' bucket tables, how the visited buckets split by route:
words of all holders up to MANY_SMALL (one wave), up to MANY_LDS (one workgroup), longer (the long route). After the first call the operands' Vec
buckets are sorted, so later calls sort sorted runs, in all four alike. Prints one JSON line."""
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

SEEDS = (42, 43, 44, 45)
MANY_SMALL, MANY_LDS = 256, 2048  # cbl_amd/csrc/kernels_setops.hpp
CALLS = ("merge", "intersect", "at_least_2", "occupancy")


def route_split(tables, nprefix, t):
    """{route: (buckets, words of all holders)} of the prefixes t operands or more hold (at least two: a one-holder bucket takes no bucket kernel),
    from the operands' (prefix, length) tables. Host only."""
    import numpy as np

    holders, words = np.zeros(nprefix, dtype=np.uint8), np.zeros(nprefix, dtype=np.uint64)
    for p, l in tables:
        holders[p] += 1
        words[p] += l.astype(np.uint64)
    w = words[holders >= max(t, 2)]
    cls = {"wave": w <= MANY_SMALL, "workgroup": (w > MANY_SMALL) & (w <= MANY_LDS), "long": w > MANY_LDS}
    return {name: (int(sel.sum()), int(w[sel].sum())) for name, sel in cls.items()}


def child(a):
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    k, pb, length = 31, 24, 150
    xs = []
    for i, seed in enumerate(SEEDS):
        bases, offsets = synth.reads_torch(seed, a.reads, length, first_read=0, device=dev)
        x = cbl_amd.CBL(k, pb, device=0, profile=(i == 0))  # occupancy runs on its first operand's stream: that context reads its stage timers
        x.insert_seqs_device(bases, offsets, a.reads)
        xs.append(x)
        del bases, offsets
    work = cbl_amd.CBL(k, pb, device=0, profile=True)
    out = {"words": [x.count() for x in xs], "buckets": [x.num_buckets() for x in xs]}
    tables = [x.bucket_table_np()[:2] for x in xs]
    for t in (1, 2, 4):
        out["routes_t%d" % t] = route_split(tables, 1 << pb, t)
    del tables
    result = {}

    def run(what):
        if what == "merge":
            cbl_amd.CBL.merge(xs, out=work)
        elif what == "intersect":
            cbl_amd.CBL.intersect(xs, out=work)
        elif what == "at_least_2":
            cbl_amd.CBL.at_least(xs, 2, out=work)
        else:
            result["hist"] = [int(v) for v in cbl_amd.CBL.occupancy(xs)]
            return
        result[what] = (work.count(), work.num_buckets())

    for what in CALLS:
        out[what + "_ms"] = []
    for i in range(a.warmup + a.steps):
        for what in CALLS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(what)
            torch.cuda.synchronize()
            if i >= a.warmup:
                out[what + "_ms"].append(round((time.perf_counter() - t0) * 1e3, 3))
    for what in CALLS:
        ctx = xs[0] if what == "occupancy" else work
        ctx.stage_times_reset()
        run(what)
        out[what + "_stage_ms"] = {name: round(t, 3) for name, (t, n) in ctx.stage_times().items() if n}
    for what in CALLS[:3]:
        out[what + "_words_out"], out[what + "_buckets_out"] = result[what]
    out["hist"] = result["hist"]
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reads", type=int, default=6_250_000)
    ap.add_argument("--timeout", type=float, default=600.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--steps", str(a.steps), "--warmup", str(a.warmup), "--reads", str(a.reads)]
    try:
        r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=dict(os.environ))
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": "time limit of %.0f s" % a.timeout}), flush=True)
        return 1
    if r.returncode != 0:
        print(json.dumps({"error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
        return 1
    print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
