#!/usr/bin/env python3
"""Times the connected components of the compacted graph and their filter on one MI355X: K = 31, PREFIX_BITS = 24, non-canonical or, with --canonical,
canonical. Recorded, not asserted; the results are in profiles/components_rate.md. Two data sets:

  --data tips     the index of tools/dev_tips_rate.py: 1 M reads of 150 bases from cbl_amd.synth plus a second copy of every tenth read with one substituted
                  base: every read with its copy is a component of its own — many small components;
  --data genome   1 M reads of 150 bases cut every 100 bases from one random genome (neighbours overlap by 50 bases), with the same copies: one giant
                  component, the contended case of k_cc_sizes.

    python tools/dev_components_rate.py [--data tips|genome] [--canonical] [--reads 1000000] [--steps 5] [--timeout 1100]
    python tools/dev_components_rate.py [...] --child --only components|filter --steps 1     # nothing but those calls: the run to put under a kernel trace
    CBLX_LIB_PATH=<a library without the feature> python tools/dev_components_rate.py [...] --child --parts

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process; a call that changes the index runs on
a copy of it (`a | empty` into one second index, outside the timed region: that index keeps its pool):
  (a) the host way: gfa_links_np() and the table (unitig_table_np / biunitig_table_np) of the whole index to the host, then
      scipy.sparse.csgraph.connected_components on the links and numpy for the numbering and the sizes — one step;
  (b) gfa_links_device(): what the labelling starts from — the Python method calls the library twice (the counts, then the fill) —, and one
      cblx_gfa_links_device call into tensors allocated once (`links_call`);
  (c) components_device(): the table on the device — two library calls as well, each with the whole labelling —, and one cblx_components_device call into
      tensors allocated once (`components_call`);
  (d) components_filter(min_kmers): every component below the threshold (--min-kmers; default 121, one more than the k-mers of one read: in `tips` a read
      without a copy goes and a read with its copy stays, a removal of most of the index; in `genome` nothing is below it, and the call ends behind the table);
  (e) components_filter(largest=True).
--parts uses nothing this feature added, so that a library built from the parent commit can run it: gfa_links_device and one links call, one export sweep
(export_kmers_range_device over the whole index), and one remove_words_device of the words row (d) removes, which it selects with torch from the table, the
link table (labels by torch min-propagation, untimed) and resident_export. (c) is held against (b) of the same kind, (d) — one library call — against the sum of one links call, the sweep and the removal.
Checked in the same process: (a) and (c) give the same table; (d) leaves count - removed_kmers k-mers; the index --parts leaves has the checksum of the one
(d) leaves. The child runs under a time limit; nothing is started after one that fails."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

K, PB, LENGTH, STEP = 31, 24, 150, 100


def add_copies(g, b, o, n, dev):
    """dev_tips_rate.build's second flush: a copy of every tenth read's worth of reads (the first n / 10) with one substituted base near an end."""
    import torch

    m = n // 10
    twin = b[: m * LENGTH].clone().view(m, LENGTH)
    i = torch.arange(m, device=dev)
    d = 1 + i % (K - 1)
    col = torch.where((i // (K - 1)) % 2 == 0, d - 1, LENGTH - d)
    lut = torch.tensor(list(b"ACTG"), dtype=torch.uint8, device=dev)
    code = (twin[i, col][:, None] == lut[None, :]).to(torch.uint8).argmax(dim=1)
    twin[i, col] = lut[(code + 1 + i % 3) % 4]
    flat = torch.cat([twin.reshape(-1), torch.zeros(16, dtype=torch.uint8, device=dev)])
    g.insert_seqs_device(flat, o[: m + 1].clone(), m)


def build(a, dev):
    """The index, and an empty one of the same parameters to copy it with."""
    import torch

    import cbl_amd
    from cbl_amd import synth

    if a.data == "tips":
        import dev_tips_rate

        return dev_tips_rate.build(a, dev)
    n = a.reads
    g = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    genome, _ = synth.reads_torch(42, 1, STEP * (n - 1) + LENGTH, device=dev)
    o = torch.arange(n + 1, dtype=torch.int64, device=dev) * LENGTH
    b = torch.empty(n * LENGTH + 16, dtype=torch.uint8, device=dev)
    b[-16:] = 0
    part = 1 << 18
    for r0 in range(0, n, part):  # read r = genome[STEP r : STEP r + LENGTH]
        r1 = min(n, r0 + part)
        idx = (torch.arange(r0, r1, device=dev) * STEP)[:, None] + torch.arange(LENGTH, device=dev)[None, :]
        b[r0 * LENGTH: r1 * LENGTH] = genome[idx.reshape(-1)]
    del genome
    g.insert_seqs_device(b, o, n)
    add_copies(g, b, o, n, dev)
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


def links_call(torch, g, dev):
    """One cblx_gfa_links_device call into tensors allocated once: the compaction, the link counts and the fill — what one labelling starts from."""
    u, ln = g.gfa_counts()
    start, to = torch.empty(2 * u + 1, dtype=torch.int64, device=dev), torch.empty(max(ln, 1), dtype=torch.int32, device=dev)
    rev = torch.empty(max(ln, 1), dtype=torch.uint8, device=dev)
    return lambda: g._gfa_links(True, start, 2 * u + 1, to, rev, ln)


def torch_labels(torch, lt, nu):
    """Per unitig the smallest unitig of its component, by min-propagation over the link table with torch alone (untimed: --parts only selects with it)."""
    start = lt["link_start"]
    frm = torch.repeat_interleave(torch.arange(2 * nu, device=start.device) >> 1, start[1:] - start[:-1])
    to = lt["link_to"].to(torch.int64)
    par = torch.arange(nu, device=start.device)
    while True:
        a, b = par[frm], par[to]
        if bool((a == b).all()):
            return par
        nxt = par.clone()
        nxt.scatter_reduce_(0, torch.maximum(a, b), torch.minimum(a, b), reduce="amin")
        while True:
            g = nxt[nxt]
            if bool((g == nxt).all()):
                break
            nxt = g
        par = nxt


def parts(a):
    """gfa_links_device, one export sweep, one remove_words_device: nothing the feature added."""
    import torch

    import cbl_amd

    dev = torch.device("cuda", 0)
    g, empty = build(a, dev)
    n = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "data": a.data, "canonical": a.canonical, "index_kmers": n}
    out["gfa_links_device_ms"] = timed(lambda: g.gfa_links_device(), a.steps)
    out["links_call_ms"] = timed(links_call(torch, g, dev), a.steps)
    d_lo = torch.empty(n, dtype=torch.int64, device=dev)
    out["export_sweep_ms"] = timed(lambda: g.export_kmers_range_device(0, n, d_lo), a.steps)
    del d_lo
    t = (g.biunitig_table_device if a.canonical else g.unitig_table_device)()
    lt = g.gfa_links_device()
    nu = lt["n_unitigs"]
    par = torch_labels(torch, lt, nu)
    size = torch.zeros(nu, dtype=torch.int64, device=dev).index_add_(0, par, t["length"].to(torch.int64))
    sel = (size[par] < a.min_kmers)[t["unitig"].to(torch.int64)]
    out["components"] = int((par == torch.arange(nu, device=dev)).sum())
    del t, lt, par, size
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
        if ns:
            h.remove_words_device(w_lo, w_hi, ns)
        last["left"], last["checksum"] = h.count(), h.checksum()

    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    out["remove_words_ms"] = timed(remove, a.steps, before=lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h))
    out["kmers_left"], out["checksum_left"] = last["left"], last["checksum"]
    out["parts_sum_ms"] = round(min(out["links_call_ms"]) + min(out["export_sweep_ms"]) + min(out["remove_words_ms"]), 3)
    print(json.dumps(out), flush=True)
    return 0


def host_way(np, g, canonical):
    """Row (a): the two tables to the host, scipy's connected components, the numbering by ascending smallest unitig and the sizes in numpy."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components

    t = g.biunitig_table_np() if canonical else g.unitig_table_np()
    lt = g.gfa_links_np()
    nu = lt["n_unitigs"]
    start = lt["link_start"].astype(np.int64)
    frm = np.repeat(np.arange(2 * nu, dtype=np.int64) >> 1, np.diff(start))
    graph = coo_matrix((np.ones(len(frm), dtype=np.uint8), (frm, lt["link_to"].astype(np.int64))), shape=(nu, nu))
    nc, label = connected_components(graph, directed=True, connection="weak")
    first = np.full(nc, nu, dtype=np.int64)
    np.minimum.at(first, label, np.arange(nu, dtype=np.int64))
    rank = np.empty(nc, dtype=np.int64)
    rank[np.argsort(first)] = np.arange(nc)
    component = rank[label].astype(np.uint32)
    kmers = np.bincount(component, weights=t["length"], minlength=nc).astype(np.uint64)
    return component, np.bincount(component, minlength=nc).astype(np.uint32), kmers


def child(a):
    import numpy as np
    import torch

    import cbl_amd

    dev = torch.device("cuda", 0)
    g, empty = build(a, dev)
    count = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "data": a.data, "canonical": a.canonical, "reads": a.reads, "index_kmers": count, "min_kmers": a.min_kmers}
    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    copy = lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h)  # noqa: E731
    last = {}

    def filt(**rule):
        def run(h):
            last["stats"] = h.components_filter(**rule)
            last["checksum"] = h.checksum()
        return run

    if a.only:
        if a.only == "components":
            out["components_device_ms"] = timed(lambda: last.update(t=g.components_device()), a.steps)
            out["counts"] = {key: last["t"][key] for key in ("n_unitigs", "n_links", "n_components", "largest_kmers", "rounds")}
        else:
            out["components_filter_ms"] = timed(filt(min_kmers=a.min_kmers), a.steps, before=copy)
            out["stats"] = last["stats"]
        print(json.dumps(out), flush=True)
        return 0

    out["gfa_links_device_ms"] = timed(lambda: g.gfa_links_device(), a.steps)
    out["links_call_ms"] = timed(links_call(torch, g, dev), a.steps)
    out["components_device_ms"] = timed(lambda: last.update(t=g.components_device()), a.steps)
    t = last.pop("t")
    cap = (t["n_unitigs"], t["n_components"])
    out["components_call_ms"] = timed(lambda: g._components(True, t["component"], cap[0], None, 0, t["first"], t["unitigs"], t["kmers"], cap[1]), a.steps)
    out["counts"] = {key: t[key] for key in ("n_unitigs", "n_links", "n_components", "largest_kmers", "rounds")}
    base = {}
    out["host_way_ms"] = timed(lambda: base.update(r=host_way(np, g, a.canonical)), a.baseline_steps, warm=0)
    component, unitigs, kmers = base.pop("r")
    assert np.array_equal(component, t["component"].cpu().numpy().view(np.uint32)) and np.array_equal(unitigs, t["unitigs"].cpu().numpy().view(np.uint32)) and \
        np.array_equal(kmers, t["kmers"].cpu().numpy().view(np.uint64)), "(a) and (c) differ"
    small = kmers < a.min_kmers
    del t
    out["components_filter_ms"] = timed(filt(min_kmers=a.min_kmers), a.steps, before=copy)
    st = out["filter_stats"] = last["stats"]
    out["filter_checksum"] = last["checksum"]
    assert st["removed_components"] == int(small.sum()) and st["removed_kmers"] == int(kmers[small].sum()) and st["kmers_left"] == count - st["removed_kmers"]
    out["components_largest_ms"] = timed(filt(largest=True), a.steps, before=copy)
    st = out["largest_stats"] = last["stats"]
    assert st["kmers_left"] == int(kmers.max()) and st["removed_components"] == len(kmers) - 1
    for key in ("gfa_links_device", "components_device", "components_filter", "components_largest", "host_way"):
        out[key + "_ns_per_kmer"] = round(min(out[key + "_ms"]) * 1e6 / count, 3)
    out["components_over_links"] = round(min(out["components_device_ms"]) / min(out["gfa_links_device_ms"]), 4)
    out["components_call_over_links_call"] = round(min(out["components_call_ms"]) / min(out["links_call_ms"]), 4)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--data", choices=("tips", "genome"), default="tips")
    ap.add_argument("--canonical", action="store_true", help="a canonical index: the bidirected form")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--min-kmers", type=int, default=LENGTH - K + 2, help="the threshold of row (d): one more than the k-mers of a read")
    ap.add_argument("--baseline-steps", type=int, default=1, help="timed steps of row (a): a step is seconds of host work")
    ap.add_argument("--only", choices=("components", "filter"), help="only those calls (for a kernel trace)")
    ap.add_argument("--parts", action="store_true", help="gfa_links_device, the export sweep and remove_words_device alone (runs on a library without the feature)")
    ap.add_argument("--timeout", type=float, default=1100.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return parts(a) if a.parts else child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--data", a.data, "--reads", str(a.reads), "--steps", str(a.steps), "--min-kmers", str(a.min_kmers),
           "--baseline-steps", str(a.baseline_steps)] + (["--only", a.only] if a.only else []) + (["--parts"] if a.parts else []) + (["--canonical"] if a.canonical else [])
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
