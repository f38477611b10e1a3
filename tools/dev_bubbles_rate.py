#!/usr/bin/env python3
"""Times bubble popping on one MI355X: K = 31, PREFIX_BITS = 24, the index of 1 M reads of 150 bases from cbl_amd.synth plus a second copy of every tenth read
with one substituted base at least K positions from both ends (each copy is the second arm, of 31 k-mers, of a SNP bubble on its twin), non-canonical or,
with --canonical, canonical. The counts are a tally of the originals three times and of the copies once. Recorded, not asserted; the results are in
profiles/bubbles_rate.md.

    python tools/dev_bubbles_rate.py [--canonical] [--reads 1000000] [--steps 5] [--timeout 1100]
    python tools/dev_bubbles_rate.py [--canonical] --child --only-pop --steps 1      # nothing but pop_bubbles(counts, rounds=1) calls: for a kernel trace
    CBLX_LIB_PATH=<a library without the feature> python tools/dev_bubbles_rate.py [--canonical] --child --parts --words FILE

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process; a call that changes the index runs on
a copy of it (`a | empty` into one second index, outside the timed region) and on a clone of the counts:
  (b) bubbles_mark_device with counts into a device tensor;
  (c) pop_bubbles(rounds=1) without counts, (c') with counts;
  (d) pop_bubbles(counts, rounds=0).
With --save-words FILE the child also writes the words of the arms (c') pops (uint64 lo, uint8 hi), which --parts reads back. --parts uses nothing this
feature added, so that a library built from the parent commit can run it: one gfa_links_device, one export sweep (export_kmers_range_device over the whole
index), one remove_words_device of those words, one unitig_coverage_device and one rank_device of the survivors. (c) is held against the sum of the
first three, (c') against the sum of all five less the compaction unitig_coverage_device repeats (its k_unitig_kc alone comes from a kernel trace).
Checked in the same process: (c') removes what (b) counted; (d) ends at a fixpoint; the carried counts equal a fresh tally on the popped index; the index
--parts leaves has the checksum of the one (c') leaves. The child runs under a time limit; nothing is started after one that fails."""
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
    """The index, an empty one of the same parameters to copy it with, and the two read batches (originals, copies) on the device."""
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
    col = K + i % (LENGTH - 2 * K)  # at least K bases from both ends: K k-mers hold the substituted base, and one k-mer at least lies on either side
    lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=dev)
    old = twin[i, col]
    code = (old[:, None] == lut[None, :]).to(torch.uint8).argmax(dim=1)
    twin[i, col] = lut[(code + 1 + i % 3) % 4]
    flat = torch.cat([twin.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    o2 = o[: m + 1].clone()
    g.insert_seqs_device(flat, o2, m)
    g.flush()
    torch.cuda.synchronize()
    return g, cbl_amd.CBL(K, PB, canonical=a.canonical, device=0), (b, o, n), (flat, o2, m)


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


def parts(a):
    """One link table, one export sweep, one remove_words_device, one coverage call, one rank of the survivors: nothing the feature added."""
    import numpy as np
    import torch

    import cbl_amd

    dev = torch.device("cuda", 0)
    g, empty, originals, copies = build(a, dev)
    n = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "index_kmers": n}
    out["gfa_links_device_ms"] = timed(lambda: g.gfa_links_device(), a.steps)
    d_lo = torch.empty(n, dtype=torch.int64, device=dev)
    out["export_sweep_ms"] = timed(lambda: g.export_kmers_range_device(0, n, d_lo), a.steps)
    counts = None
    for _ in range(3):
        counts, _, _ = g.abundance_seqs_device(*originals, counts)
    counts, _, _ = g.abundance_seqs_device(*copies, counts)
    out["unitig_coverage_device_ms"] = timed(lambda: g.unitig_coverage_device(counts), a.steps)
    raw = np.fromfile(a.words, dtype=np.uint8)
    ns = len(raw) // 9
    w_lo = torch.from_numpy(raw[: 8 * ns].view(np.int64).copy()).to(dev)
    w_hi = torch.from_numpy(raw[8 * ns:].copy()).to(dev)
    out["selected_kmers"] = ns
    last = {}

    def remove(h):
        h.remove_words_device(w_lo, w_hi, ns)
        last["left"], last["checksum"] = h.count(), h.checksum()

    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    out["remove_words_ms"] = timed(remove, a.steps, before=lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h))
    out["kmers_left"], out["checksum_left"] = last["left"], last["checksum"]
    left = h.count()
    h.export_kmers_range_device(0, left, d_lo)
    d_rank = torch.empty(left, dtype=torch.int64, device=dev)
    out["rank_survivors_ms"] = timed(lambda: h.rank_device(d_lo, None, left, d_rank), a.steps)
    out["parts_sum_ms"] = round(min(out["gfa_links_device_ms"]) + min(out["export_sweep_ms"]) + min(out["remove_words_ms"]), 3)
    out["parts_sum_counts_ms"] = round(out["parts_sum_ms"] + min(out["rank_survivors_ms"]), 3)  # + k_unitig_kc, from a trace
    print(json.dumps(out), flush=True)
    return 0


def child(a):
    import torch

    import cbl_amd

    dev = torch.device("cuda", 0)
    g, empty, originals, copies = build(a, dev)
    count = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "reads": a.reads, "index_kmers": count}
    counts = None
    for _ in range(3):
        counts, _, _ = g.abundance_seqs_device(*originals, counts)
    counts, _, _ = g.abundance_seqs_device(*copies, counts)
    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    state = {}

    def copy():
        cbl_amd.CBL.set_op(g, empty, "or", out=h)
        state["counts"] = counts.clone()
        return h

    last = {}

    def pop(counted, rounds):
        def run(h):
            r = h.pop_bubbles(None, state["counts"] if counted else None, rounds=rounds)
            last["stats"] = r[0] if counted else r
        return run

    if a.only_pop:
        out["pop_counts_1_ms"] = timed(pop(True, 1), a.steps, before=copy)
        out["stats"] = last["stats"]
        print(json.dumps(out), flush=True)
        return 0

    nu = g.bubble_counts()["n_unitigs"]
    d_kind = torch.empty(max(nu, 1), dtype=torch.uint8, device=dev)
    marks = {}

    def mark():
        marks.update(g.bubbles_mark_device(None, counts, d_kind, nu))

    out["bubbles_mark_device_ms"] = timed(mark, a.steps)
    out["unitigs"], out["marks"] = nu, {key: marks[key] for key in cbl_amd.BUBBLE_COUNTS}
    assert int((d_kind == 1).sum()) == marks["popped"] and int((d_kind == 2).sum()) == marks["bubbles"]
    if a.save_words:  # the words of the popped arms, for --parts: the resident words of the index whose k-mer's unitig is popped
        t = (g.biunitig_table_device if a.canonical else g.unitig_table_device)()
        sel = (d_kind == 1)[t["unitig"].to(torch.int64)]
        del t
        c = g.consts()
        assert c["bytes"] == 6 and c["hi_bytes"] == 1 and c["suffix_bits"] == 44
        nb = g.num_buckets()
        prefix, cnt = torch.empty(nb, dtype=torch.int32, device=dev), torch.empty(nb, dtype=torch.int32, device=dev)
        kinds, suffix = torch.empty(nb, dtype=torch.uint8, device=dev), torch.empty(count * 6, dtype=torch.uint8, device=dev)
        g.resident_export(prefix, cnt, kinds, suffix)
        p = torch.repeat_interleave(prefix.to(torch.int64), cnt.to(torch.int64))[sel]
        s = suffix.view(count, 6)[sel].to(torch.int64)
        del suffix
        w_lo = p << 44
        for j in range(6):
            w_lo |= s[:, j] << (8 * j)
        w_hi = (p >> 20).to(torch.uint8)
        with open(a.save_words, "wb") as f:
            f.write(w_lo.cpu().numpy().tobytes())
            f.write(w_hi.cpu().numpy().tobytes())
        out["saved_words"] = int(sel.sum())
        del sel, p, s, w_lo, w_hi
    out["pop_1_ms"] = timed(pop(False, 1), a.steps, before=copy)
    out["pop_1_stats"] = last["stats"]
    out["pop_counts_1_ms"] = timed(pop(True, 1), a.steps, before=copy)
    st = out["pop_counts_1_stats"] = last["stats"]
    out["pop_counts_1_checksum"] = h.checksum()
    assert (st["bubbles"], st["popped"], st["popped_kmers"]) == tuple(marks[key] for key in cbl_amd.BUBBLE_COUNTS), "(c') did not remove what (b) counted"
    assert st["kmers_left"] == count - marks["popped_kmers"]
    fresh = None
    for _ in range(3):
        fresh, _, _ = h.abundance_seqs_device(*originals, fresh)
    fresh, _, _ = h.abundance_seqs_device(*copies, fresh)
    assert torch.equal(fresh, state["counts"][: st["kmers_left"]]) and not bool(state["counts"][st["kmers_left"]:].any()), "the carried counts are not a fresh tally"
    out["carry_equals_fresh_tally"] = True
    out["pop_counts_0_ms"] = timed(pop(True, 0), a.steps, before=copy)
    st = out["pop_counts_0_stats"] = last["stats"]
    assert st["fixpoint"] == 1 and st["kmers_left"] == count - st["popped_kmers"]
    for key in ("bubbles_mark_device", "pop_1", "pop_counts_1", "pop_counts_0"):
        out[key + "_ns_per_kmer"] = round(min(out[key + "_ms"]) * 1e6 / count, 3)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--canonical", action="store_true", help="a canonical index: the bidirected form")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--only-pop", action="store_true", help="only pop_bubbles(counts, rounds=1) calls (for a kernel trace)")
    ap.add_argument("--parts", action="store_true", help="the link table, the export sweep, remove_words_device, the coverage and the rank alone (runs on a library without the feature)")
    ap.add_argument("--save-words", metavar="FILE", help="write the words of the popped arms for --parts")
    ap.add_argument("--words", metavar="FILE", help="the words --save-words wrote")
    ap.add_argument("--timeout", type=float, default=1100.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.parts and not a.words:
        ap.error("--parts needs --words")
    if a.child:
        return parts(a) if a.parts else child(a)
    cmd = ([sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps)] + (["--only-pop"] if a.only_pop else []) +
           (["--parts", "--words", a.words] if a.parts else []) + (["--save-words", a.save_words] if a.save_words else []) + (["--canonical"] if a.canonical else []))
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
