#!/usr/bin/env python3
"""Times a batch of reads against a PANEL of indexes on one MI355X: K = 31, PREFIX_BITS = 24, 1 M reads of 150 bases from cbl_amd.synth (120 M k-mers per
call), panels of n = 2, 4, 8 and 16 indexes. Recorded, not asserted; the results are in profiles/panel_query_rate.md.

    python tools/dev_panel_query_rate.py [--reads 1000000] [--steps 5] [--panels 2,4,8,16] [--timeout 900]
    python tools/dev_panel_query_rate.py --only-panel 8 --steps 3      # nothing but panel calls at one n: the run to put under a kernel trace

The indexes: the first third of the reads is shared by all of them, the other two thirds are cut into 16 disjoint parts and index j takes part j on top of the
shared third; a panel of n is the first n of the 16. The queries are all the reads, so every read hits the shared third or exactly one index.

Rows (wall time around calls that return after the device is done; reads, offsets and outputs are device tensors), in one process and taking turns step by step:
  (a) n successive cblx_contains_seqs_counts_device calls, one per index: the only way to the table without the panel call;
  (b) one cblx_contains_seqs_counts_many_device call, no mask;
  (c) the same call with a caller's mask tensor.
The child runs under a time limit; nothing is started after one that fails."""
import argparse
import json
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

K, PB, LENGTH, PARTS = 31, 24, 150, 16


def child(a):
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    n = a.reads
    b, o = synth.reads_torch(42, n, LENGTH, device=dev)
    panels = [int(x) for x in a.panels.split(",")] if not a.only_panel else [a.only_panel]
    third = n // 3
    part = (n - third) // PARTS
    per = LENGTH - K + 1
    nk = n * per
    cbls = []
    for j in range(max(panels)):
        g = cbl_amd.CBL(K, PB, device=0)
        g.insert_seqs_device(b, o[: third + 1], third)
        lo = third + j * part
        g.insert_seqs_device(b, o[lo: lo + part + 1], part)
        cbls.append(g)
    out = {"lib": str(cbl_amd.LIB_PATH), "reads": n, "queries": nk, "index_kmers": [g.count() for g in cbls], "panels": {}}
    d_t = torch.empty(n, dtype=torch.int32, device=dev)
    d_m = torch.empty(nk, dtype=torch.int64, device=dev)
    for m in panels:
        panel = cbls[:m]
        d_p = torch.empty((m, n), dtype=torch.int32, device=dev)
        d_q = torch.empty((m, n), dtype=torch.int32, device=dev)

        def one_by_one():
            for j, g in enumerate(panel):
                g.contains_seqs_counts_device(b, o, n, d_t, d_q[j])

        def many():
            cbl_amd.CBL.contains_seqs_counts_many_device(panel, b, o, n, d_t, d_p)

        def many_mask():
            cbl_amd.CBL.contains_seqs_counts_many_device(panel, b, o, n, d_t, d_p, d_m)

        rows = {"many_ms": many} if a.only_panel else {"one_by_one_ms": one_by_one, "many_ms": many, "many_mask_ms": many_mask}
        ms = {key: [] for key in rows}
        for step in range(a.steps + 1):  # the first step warms up (workspace allocation); the rows take turns
            for key, fn in rows.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ms[key].append(round((time.perf_counter() - t0) * 1e3, 3))
        res = {key: v[1:] for key, v in ms.items()}
        if not a.only_panel:
            assert bool((d_p == d_q).all()), "the panel call and the calls one by one disagree"
            hits = d_p.sum(dim=1, dtype=torch.int64).tolist()
            assert all(h == (third + part) * per for h in hits), hits  # an index finds its own reads whole (random reads share no 31-mer)
            bits = torch.zeros(m, dtype=torch.int64, device=dev)
            for j in range(m):
                bits[j] = ((d_m >> j) & 1).sum()
            assert bits.tolist() == hits and not bool((d_m >> m).any())
            res["speedup"] = round(min(res["one_by_one_ms"]) / min(res["many_ms"]), 3)
        out["panels"][str(m)] = res
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--panels", default="2,4,8,16")
    ap.add_argument("--only-panel", type=int, default=0, metavar="N", help="only panel calls without a mask at this n (for a kernel trace)")
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps), "--panels", a.panels, "--only-panel", str(a.only_panel)]
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
    if not a.only_panel:
        print("| n | (a) one by one | (b) panel | (c) panel + mask | a / b |\n|---|---|---|---|---|")
        for m, res in run["panels"].items():
            f = lambda v: "%.3f – %.3f, best %.3f" % (min(v), max(v), min(v))  # noqa: E731
            print("| %s | %s | %s | %s | %.2f |" % (m, f(res["one_by_one_ms"]), f(res["many_ms"]), f(res["many_mask_ms"]), res["speedup"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
