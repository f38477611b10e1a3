#!/usr/bin/env python3
"""Times tip clipping on one MI355X: K = 31, PREFIX_BITS = 24, the index of 1 M reads of 150 bases from cbl_amd.synth plus a second copy of every tenth read
with one substituted base 1 .. K - 1 positions from an end (each copy hangs a dead-end branch of that many k-mers on its twin), non-canonical or, with
--canonical, canonical. Recorded, not asserted; the results are in profiles/tips_rate.md.

    python tools/dev_tips_rate.py [--canonical] [--reads 1000000] [--steps 5] [--baseline-kmers 4194304] [--timeout 1100]
    python tools/dev_tips_rate.py [--canonical] --child --only-clip --steps 1      # nothing but clip_tips(rounds=1) calls: the run to put under a kernel trace
    CBLX_LIB_PATH=<a library without the feature> python tools/dev_tips_rate.py [--canonical] --child --parts

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process; a call that changes the index runs on
a copy of it (`a | empty` into one second index, outside the timed region: that index keeps its pool, as the first one does for the observers):
  (a) the way to the same removal on the parent commit: the table and the link table of the whole index to the host, the first `--baseline-kmers` k-mers
      (kmers_np), the ends from the link table and CBL.tip_kinds in numpy, remove_kmers of the selected k-mers among them;
  (b) tips_mark_device into a device tensor;
  (c) clip_tips(rounds=1);
  (d) clip_tips(rounds=0).
--parts uses nothing this feature added, so that a library built from the parent commit can run it: one table call (unitig_table_device /
biunitig_table_device), one export sweep (export_kmers_range_device over the whole index), and one remove_words_device of the words of the tips, which it
selects with torch from the table, the link table and resident_export. (c) is held against their sum.
Checked in the same process: (c) removes what (b) counted and leaves count - tip_kmers k-mers; (d) ends at a fixpoint; the index --parts leaves has the
checksum of the one (c) leaves. The child runs under a time limit; nothing is started after one that fails."""
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


def build(a, dev):
    """The index, and an empty one of the same parameters to copy it with."""
    import torch

    import cbl_amd
    from cbl_amd import synth

    n = a.reads
    g = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    b, o = synth.reads_torch(42, n, LENGTH, device=dev)
    g.insert_seqs_device(b, o, n)
    m = n // 10
    twin = b[: m * LENGTH].clone().view(m, LENGTH)
    i = torch.arange(m, device=dev)
    d = 1 + i % (K - 1)  # the substituted base is the d-th from an end: d k-mers hold it
    col = torch.where((i // (K - 1)) % 2 == 0, d - 1, LENGTH - d)
    lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=dev)
    old = twin[i, col]
    code = (old[:, None] == lut[None, :]).to(torch.uint8).argmax(dim=1)
    twin[i, col] = lut[(code + 1 + i % 3) % 4]
    flat = torch.cat([twin.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    g.insert_seqs_device(flat, o[: m + 1].clone(), m)
    g.flush()
    torch.cuda.synchronize()
    return g, cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)


def timed(fn, steps, warm=1, before=None):
    import torch

    ms = []
    for _ in range(steps + warm):  # the first call warms up (workspace allocation)
        arg = before() if before else None
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(arg) if before else fn()
        ms.append(round((time.perf_counter() - t0) * 1e3, 3))
    return ms[warm:]


def ends_of_links(np, lt, nu, canonical):
    start = lt["link_start"].astype(np.int64)
    right = start[1::2] - start[0:-1:2]
    left = (start[2::2] - start[1::2]) if canonical else np.bincount(lt["link_to"].astype(np.int64), minlength=nu)
    return left, right


def parts(a):
    """One table call, one export sweep, one remove_words_device: nothing the feature added."""
    import torch

    import cbl_amd

    dev = torch.device("cuda", 0)
    g, empty = build(a, dev)
    n = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "index_kmers": n}
    out["table_ms"] = timed(lambda: (g.biunitig_table_device if a.canonical else g.unitig_table_device)(), a.steps)
    d_lo = torch.empty(n, dtype=torch.int64, device=dev)
    out["export_sweep_ms"] = timed(lambda: g.export_kmers_range_device(0, n, d_lo), a.steps)
    del d_lo
    # the words of the tips, with torch: the ends from the link table, the rule, the words from the resident buckets (ascending prefixes, stored order)
    t = (g.biunitig_table_device if a.canonical else g.unitig_table_device)()
    lt = g.gfa_links_device()
    nu = lt["n_unitigs"]
    start = lt["link_start"]
    right = start[1::2] - start[0:-1:2]
    left = (start[2::2] - start[1::2]) if a.canonical else torch.bincount(lt["link_to"].to(torch.int64), minlength=nu)
    kind = (t["length"].to(torch.int64) <= K - 1) & ((left == 0) != (right == 0))
    sel = kind[t["unitig"].to(torch.int64)]
    del t, lt, start
    c = g.consts()
    assert c["bytes"] == 6 and c["hi_bytes"] == 1 and c["suffix_bits"] == 44
    nb = g.num_buckets()
    prefix, count = torch.empty(nb, dtype=torch.int32, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
    kinds, suffix = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(n * 6, dtype=torch.uint8, device=dev)
    g.resident_export(prefix, count, kinds, suffix)
    p = torch.repeat_interleave(prefix.to(torch.int64), count.to(torch.int64))[sel]
    s = suffix.view(n, 6)[sel].to(torch.int64)
    del suffix
    w_lo = p << 44
    for j in range(6):
        w_lo |= s[:, j] << (8 * j)
    w_hi = (p >> 20).to(torch.uint8)
    ns = int(sel.sum())
    out["selected_kmers"] = ns
    last = {}

    def remove(h):
        h.remove_words_device(w_lo, w_hi, ns)
        last["left"], last["checksum"] = h.count(), h.checksum()

    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    out["remove_words_ms"] = timed(remove, a.steps, before=lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h))
    out["kmers_left"], out["checksum_left"] = last["left"], last["checksum"]
    out["parts_sum_ms"] = round(min(out["table_ms"]) + min(out["export_sweep_ms"]) + min(out["remove_words_ms"]), 3)
    print(json.dumps(out), flush=True)
    return 0


def child(a):
    import numpy as np
    import torch

    import cbl_amd

    dev = torch.device("cuda", 0)
    g, empty = build(a, dev)
    count = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "reads": a.reads, "index_kmers": count}
    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    copy = lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h)  # noqa: E731
    last = {}

    def clip(rounds):
        def run(h):
            last["stats"], last["checksum"] = h.clip_tips(rounds=rounds), None
            if rounds == 1:
                last["checksum"] = h.checksum()
        return run

    if a.only_clip:
        out["clip_tips_1_ms"] = timed(clip(1), a.steps, before=copy)
        out["stats"] = last["stats"]
        print(json.dumps(out), flush=True)
        return 0

    m = min(a.baseline_kmers, count)
    base = {}

    def baseline(h):
        t = h.biunitig_table_np() if a.canonical else h.unitig_table_np()
        lt = h.gfa_links_np()
        lo, _ = h.kmers_np(0, m)
        left, right = ends_of_links(np, lt, lt["n_unitigs"], a.canonical)
        kind = cbl_amd.CBL.tip_kinds(t["length"], t["flags"], left, right, K - 1)
        gone = np.ascontiguousarray(lo[kind[t["unitig"][:m].astype(np.int64)] == 1])
        was = np.zeros(max(len(gone), 1), dtype=np.uint8)
        h._chk(h._L.cblx_remove_kmers(h._h, gone.ctypes.data, None, len(gone), was.ctypes.data))  # (the list form of remove_kmers is for a few k-mers)
        base["removed"] = int(was[: len(gone)].sum())
        base["selected"] = len(gone)

    out["baseline_kmers"] = m
    out["baseline_ms"] = timed(baseline, a.baseline_steps, warm=0, before=copy)
    out["baseline_selected"], out["baseline_removed"] = base["selected"], base["removed"]
    nu = g.tip_counts()["n_unitigs"]
    d_kind = torch.empty(max(nu, 1), dtype=torch.uint8, device=dev)
    marks = {}

    def mark():
        marks.update(g.tips_mark_device(None, d_kind, nu))

    out["tips_mark_device_ms"] = timed(mark, a.steps)
    out["unitigs"], out["marks"] = nu, {key: marks[key] for key in cbl_amd.TIP_COUNTS}
    assert int((d_kind == 1).sum()) == marks["tips"] and int((d_kind == 2).sum()) == marks["isolated"]
    out["clip_tips_1_ms"] = timed(clip(1), a.steps, before=copy)
    st = out["clip_1_stats"] = last["stats"]
    out["clip_1_checksum"] = last["checksum"]
    assert (st["tips"], st["tip_kmers"]) == (marks["tips"], marks["tip_kmers"]) and st["kmers_left"] == count - marks["tip_kmers"], "(c) did not remove what (b) counted"
    out["clip_tips_0_ms"] = timed(clip(0), a.steps, before=copy)
    st = out["clip_0_stats"] = last["stats"]
    assert st["fixpoint"] == 1 and st["kmers_left"] == count - st["tip_kmers"]
    out["baseline_ns_per_kmer"] = round(min(out["baseline_ms"]) * 1e6 / m, 3)
    for key in ("tips_mark_device", "clip_tips_1", "clip_tips_0"):
        out[key + "_ns_per_kmer"] = round(min(out[key + "_ms"]) * 1e6 / count, 3)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--canonical", action="store_true", help="a canonical index: the bidirected form")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--baseline-kmers", type=int, default=1 << 22, help="k-mers row (a) takes, from the head of the iteration order")
    ap.add_argument("--baseline-steps", type=int, default=1, help="timed steps of row (a): a step is seconds of host work")
    ap.add_argument("--only-clip", action="store_true", help="only clip_tips(rounds=1) calls (for a kernel trace)")
    ap.add_argument("--parts", action="store_true", help="the table, the export sweep and remove_words_device alone (runs on a library without the feature)")
    ap.add_argument("--timeout", type=float, default=1100.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return parts(a) if a.parts else child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps), "--baseline-kmers", str(a.baseline_kmers),
           "--baseline-steps", str(a.baseline_steps)] + (["--only-clip"] if a.only_clip else []) + (["--parts"] if a.parts else []) + (["--canonical"] if a.canonical else [])
    try:
        r = subprocess.run(cmd, timeout=a.timeout, capture_output=True, text=True, cwd=str(ROOT), env=dict(os.environ))
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
