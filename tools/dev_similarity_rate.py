#!/usr/bin/env python3
"""Times cblx_intersection_count next to what it replaces and next to a plain stream over the same words, on the two operands of
`bench.py --config merge` (cfg 5's per-GPU share: K = 31, PREFIX_BITS = 24, 6.25 M reads of 150 bases each from seeds 42 and 43 — two sets that share
next to nothing) and on a second pair whose reads overlap by half (seed 42, reads [0, n) against [n / 2, 3 n / 2)). Recorded, not asserted.

    python tools/dev_similarity_rate.py [--steps 3] [--reads 6250000] [--timeout 400] [--pairs disjoint,half]

Every pair runs in a child process of its own under a time limit (a hung step ends that child and nothing after it is started). A child builds the
two operands, warms up with one intersection_count, and then times in ONE process
    step 1  a.intersection_count(b)
    step 2  CBL.set_op(a, b, "and"), count() and close() of the result: what the count cost before
    step 3  cblx_merge_from on the same operands: a stream over the same words, which also writes them
first step 1 alone (`count_before_ms`: no AND has run yet, the operands' Vec buckets are as built), then the three steps alternating. Step 2 and
step 3 sort Vec buckets of the operands where they are stored, so the later step-1 times are on the sorted layout; both layouts must give the same
count. It prints one JSON line per pair: the times in ms (the call's host part included: every call returns synchronised), the route counts, the
bytes the count has to read — 8 per word (16 for a wide suffix) of every bucket both hold, 13 per side and bucket of directory, the two bitvectors
and rank directories — and that figure as a fraction of 8 TB/s at the median step-1 time.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PAIRS = ("disjoint", "half")


def child(a):
    import numpy as np
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    k, pb, length = 31, 24, 150
    ab, ao = synth.reads_torch(42, a.reads, length, first_read=0, device=dev)
    if a.child == "disjoint":
        bb, bo = synth.reads_torch(43, a.reads, length, first_read=0, device=dev)
    else:
        bb, bo = synth.reads_torch(42, a.reads, length, first_read=a.reads // 2, device=dev)
    A, B, work = cbl_amd.CBL(k, pb, device=0), cbl_amd.CBL(k, pb, device=0), cbl_amd.CBL(k, pb, device=0)
    A.insert_seqs_device(ab, ao, a.reads)
    B.insert_seqs_device(bb, bo, a.reads)
    del ab, ao, bb, bo
    torch.cuda.empty_cache()
    out = {"pair": a.child, "words_a": A.count(), "words_b": B.count()}

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = f()
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3, 3), r

    def step2():
        d = cbl_amd.CBL.set_op(A, B, "and")
        n = d.count()
        d.close()
        return n

    common, stats = A.intersection_count(B, stats=True)  # warm-up, and the routes
    out["common"], out["routes"] = common, stats
    before = [timed(lambda: A.intersection_count(B)) for _ in range(a.steps)]
    assert all(n == common for _, n in before)
    out["count_before_ms"] = [t for t, _ in before]
    out["count_ms"], out["and_ms"], out["merge_from_ms"] = [], [], []
    for _ in range(a.steps):
        t, n = timed(lambda: A.intersection_count(B))
        assert n == common, (n, common)
        out["count_ms"].append(t)
        t, n = timed(step2)
        assert n == common, (n, common)
        out["and_ms"].append(t)
        t, _ = timed(lambda: work.merge_from(A, B))
        out["merge_from_ms"].append(t)
    t, n = timed(lambda: A.intersection_count(B))  # once more behind the last AND and the last merge
    assert n == common, (n, common)
    out["count_ms"].append(t)
    assert work.count() == out["words_a"] + out["words_b"] - common
    work.close()
    # the bytes the count has to read
    pa, la, _ = A.bucket_table_np()
    pb_, lb, _ = B.bucket_table_np()
    _, ia, ib = np.intersect1d(pa, pb_, assume_unique=True, return_indices=True)
    words_both = int(la[ia].sum(dtype=np.uint64)) + int(lb[ib].sum(dtype=np.uint64))
    nprefix = 1 << pb
    out["buckets_both"], out["words_in_both_held_buckets"] = int(len(ia)), words_both
    out["bytes_needed"] = words_both * 8 + len(ia) * 2 * 13 + 2 * (nprefix // 8 + nprefix // 64 * 8)
    med = statistics.median(out["count_before_ms"] + out["count_ms"])
    out["fraction_of_8TBps"] = round(out["bytes_needed"] / (med * 1e-3) / 8e12, 4)
    out["count_over_merge_from"] = round(med / statistics.median(out["merge_from_ms"]), 4)
    out["and_spread_ms"] = round(max(out["and_ms"]) - min(out["and_ms"]), 3)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=6_250_000)
    ap.add_argument("--timeout", type=float, default=400.0, help="seconds one pair's child may take")
    ap.add_argument("--pairs", default=",".join(PAIRS))
    ap.add_argument("--child", choices=PAIRS, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    for pair in a.pairs.split(","):
        cmd = [sys.executable, str(Path(__file__).resolve()), "--child", pair, "--steps", str(a.steps), "--reads", str(a.reads)]
        try:
            r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, env=dict(os.environ))
        except subprocess.TimeoutExpired:
            print(json.dumps({"pair": pair, "error": "time limit of %.0f s" % a.timeout}), flush=True)
            return 1
        if r.returncode != 0:
            print(json.dumps({"pair": pair, "error": "exit %d" % r.returncode, "stderr": r.stderr[-2000:]}), flush=True)
            return 1  # nothing more is started on the GPU after a failure
        print(r.stdout.strip().splitlines()[-1], flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
