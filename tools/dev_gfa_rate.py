#!/usr/bin/env python3
"""Times the link and GFA calls on one MI355X: K = 31, PREFIX_BITS = 24, the index of 1 M reads of 150 bases from cbl_amd.synth (120 M k-mers), non-canonical
or, with --canonical, canonical. Recorded, not asserted; the results are in profiles/gfa_rate.md.

    python tools/dev_gfa_rate.py [--canonical] [--reads 1000000] [--steps 5] [--baseline-kmers 4194304] [--timeout 1100]
    python tools/dev_gfa_rate.py [--canonical] --child --only-links --steps 1      # nothing but cblx_gfa_links_device calls: the run to put under a kernel trace

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process:
  (a) the way to the links on the parent commit: the table to the host (unitig_table_np / biunitig_table_np, the whole index), then over the first
      `--baseline-kmers` k-mers of the iteration order kmers_np and neighbors_range_np (9 bytes per k-mer over PCIe), the successors of the tails of the images among them
      formed on the host, rank_np of those, and the targets' unitig and side from the table. The two parts are reported apart;
  (b) cblx_gfa_links_device into three device tensors, over the whole index;
  (c) gfa_text_device into a device tensor;
  (d) gfa_to_file.
Checked in the same process: link_start ends in L, L agrees with the degree table through L = E - n + U (2 n, 2 U and both nibbles for a canonical index), the
links of (a) are those of (b) for the slots (a) covers, the text of (c) begins with the header and holds 1 + U + (L lines) newlines, and the file of (d) holds
the bytes of (c). The child runs under a time limit; nothing is started after one that fails."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

K, PB, LENGTH = 31, 24, 150


def rc64(x):
    """Reverse complement of packed K-mers (uint64 array; codes ACTG = 0123, complement = code ^ 2)."""
    import numpy as np

    u = np.uint64
    x = ((x >> u(2)) & u(0x3333333333333333)) | ((x & u(0x3333333333333333)) << u(2))
    x = ((x >> u(4)) & u(0x0F0F0F0F0F0F0F0F)) | ((x & u(0x0F0F0F0F0F0F0F0F)) << u(4))
    x = x.byteswap() >> u(64 - 2 * K)
    return x ^ u(0xAAAAAAAAAAAAAAAA & ((1 << (2 * K)) - 1))


def host_links(g, t, m, canonical):
    """The links that leave the tails of the images among the first m k-mers, the parent commit's way: {slot: [(unitig, rev)] in ascending base}."""
    import numpy as np

    lo, _ = g.kmers_np(0, m)
    masks = g.neighbors_range_np(0, m)
    unitig, offset, length = t["unitig"], t["offset"], t["length"]
    rev = t["reversed"] if canonical else np.zeros(len(unitig), dtype=np.uint8)
    u, off, rv = unitig[:m].astype(np.int64), offset[:m], rev[:m]
    mask = np.uint64((1 << (2 * K)) - 1)
    q_kmer, q_slot, q_flip = [], [], []
    for side in ((0, 1) if canonical else (0,)):
        at = np.flatnonzero(off + 1 == length[u]) if side == 0 else np.flatnonzero(off == 0)
        s = rv[at] ^ side  # the orientation of the stored k-mer on this image
        z = np.where(s == 1, rc64(lo[at]), lo[at])
        mk = masks[at].astype(np.uint32)
        in4 = mk >> 4
        out = np.where(s == 1, ((in4 & 3) << 2) | (in4 >> 2), mk & 15)
        for c in range(4):
            has = np.flatnonzero((out >> c) & 1)
            q_kmer.append(((z[has] << np.uint64(2)) | np.uint64(c)) & mask)
            q_slot.append(2 * u[at[has]] + side)
            q_flip.append(np.full(len(has), c, dtype=np.int64))
    y, slot, base = np.concatenate(q_kmer), np.concatenate(q_slot), np.concatenate(q_flip)
    r = g.rank_np((y, None)).astype(np.int64)
    assert (r >= 0).all() and (r < len(unitig)).all(), "a successor the mask names is not in the index"
    if canonical:
        bits = y ^ (y >> np.uint64(32))  # the stored form has an even number of set bits
        for sh in (16, 8, 4, 2, 1):
            bits = bits ^ (bits >> np.uint64(sh))
        t_flip = (bits & np.uint64(1)).astype(np.uint8)
    else:
        t_flip = np.zeros(len(y), dtype=np.uint8)
    order = np.lexsort((base, slot))
    links = {}
    for a, v, f in zip(slot[order].tolist(), unitig[r[order]].tolist(), (rev[r[order]] != t_flip[order]).tolist()):
        links.setdefault(a, []).append((v, int(f)))
    return links


def child(a):
    import numpy as np
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    n = a.reads
    g = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    b, o = synth.reads_torch(42, n, LENGTH, device=dev)
    g.insert_seqs_device(b, o, n)
    del b, o
    count = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "reads": n, "index_kmers": count}

    def timed(fn, steps, warm=1):
        ms = []
        for _ in range(steps + warm):  # the first call warms up (workspace allocation)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            ms.append(round((time.perf_counter() - t0) * 1e3, 3))
        return ms[warm:]

    L = g._L
    C = cbl_amd.C
    nu, nl = g.gfa_counts()
    out["unitigs"], out["links"] = nu, nl
    start = torch.empty(2 * nu + 1, dtype=torch.int64, device=dev)
    to = torch.empty(max(nl, 1), dtype=torch.int32, device=dev)
    rev = torch.empty(max(nl, 1), dtype=torch.uint8, device=dev)
    counts = [C.c_uint64(0) for _ in range(2)]

    def links():
        g._chk(L.cblx_gfa_links_device(g._h, start.data_ptr(), 2 * nu + 1, to.data_ptr(), rev.data_ptr(), nl, *[C.byref(c) for c in counts]))

    if a.only_links:
        out["gfa_links_device_ms"] = timed(links, a.steps)
        print(json.dumps(out), flush=True)
        return 0

    m = min(a.baseline_kmers, count)
    base = {}

    def baseline_table():
        base["t"] = g.biunitig_table_np() if a.canonical else g.unitig_table_np()

    def baseline_links():
        base["links"] = host_links(g, base["t"], m, a.canonical)

    out["baseline_kmers"] = m
    out["baseline_table_ms"] = timed(baseline_table, a.baseline_steps, warm=0)
    out["baseline_links_ms"] = timed(baseline_links, a.baseline_steps, warm=0)
    out["baseline_slots_with_links"] = len(base["links"])
    out["gfa_links_device_ms"] = timed(links, a.steps)
    assert tuple(c.value for c in counts) == (nu, nl)
    h_start = start.cpu().numpy().view(np.uint64)
    assert int(h_start[-1]) == nl and int(h_start[0]) == 0 and bool((np.diff(h_start.astype(np.int64)) >= 0).all()), "link_start is no CSR ending in L"
    deg = g.degree_table().astype(np.int64)
    e_out, e_in = int((deg.sum(axis=1) * np.arange(5)).sum()), int((deg.sum(axis=0) * np.arange(5)).sum())
    assert nl == (e_out + e_in - 2 * count + 2 * nu if a.canonical else e_out - count + nu), "L does not agree with the degree table"
    h_to, h_rev = to.cpu().numpy().view(np.uint32), rev.cpu().numpy()
    for slot, want in base["links"].items():  # the host route and the device agree where the host route looked
        lo_, hi_ = int(h_start[slot]), int(h_start[slot + 1])
        assert [(int(v), int(f)) for v, f in zip(h_to[lo_:hi_], h_rev[lo_:hi_])] == want, "the links of slot %d differ from the host route's" % slot
    per_slot = np.bincount(np.diff(h_start.astype(np.int64)), minlength=5)
    out["slots_by_links"] = per_slot.tolist()
    del base
    nbytes, nu2, nlines = g.gfa_text_device()
    assert nu2 == nu
    out["text_bytes"], out["l_lines"] = nbytes, nlines
    d_text = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    out["gfa_text_device_ms"] = timed(lambda: g.gfa_text_device(d_text, nbytes), a.steps)
    assert d_text[:11].cpu().numpy().tobytes() == b"H\tVN:Z:1.0\n" and int((d_text == 10).sum()) == 1 + nu + nlines and int(d_text[-1]) == 10, "the text does not hold its lines"
    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        path = os.path.join(tmp, "graph.gfa")
        out["gfa_to_file_ms"] = timed(lambda: g.gfa_to_file(path), a.steps)
        data = np.fromfile(path, dtype=np.uint8)
    assert np.array_equal(data, d_text.cpu().numpy()), "the file differs from the device text"
    out["baseline_links_ns_per_kmer"] = round(min(out["baseline_links_ms"]) * 1e6 / m, 3)
    for key in ("gfa_links_device", "gfa_text_device", "gfa_to_file"):
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
    ap.add_argument("--only-links", action="store_true", help="only cblx_gfa_links_device calls (for a kernel trace)")
    ap.add_argument("--tmp", default=None, help="directory for the file of row (d)")
    ap.add_argument("--timeout", type=float, default=1100.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps), "--baseline-kmers", str(a.baseline_kmers),
           "--baseline-steps", str(a.baseline_steps)] + (["--only-links"] if a.only_links else []) + (["--canonical"] if a.canonical else [])
    if a.tmp:
        cmd += ["--tmp", a.tmp]
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
    if not a.only_links:
        f = lambda v: "%.3f – %.3f, best %.3f" % (min(v), max(v), min(v))  # noqa: E731
        print("| row | k-mers | ms | ns per k-mer |\n|---|---|---|---|")
        print("| (a) host route: the table to the host | %d | %s | |" % (run["index_kmers"], f(run["baseline_table_ms"])))
        print("| (a) host route: the links of a prefix | %d | %s | %.3f |" % (run["baseline_kmers"], f(run["baseline_links_ms"]), run["baseline_links_ns_per_kmer"]))
        for row, key in (("(b) gfa_links_device", "gfa_links_device"), ("(c) gfa_text_device", "gfa_text_device"), ("(d) gfa_to_file", "gfa_to_file")):
            print("| %s | %d | %s | %.3f |" % (row, run["index_kmers"], f(run[key + "_ms"]), run[key + "_ns_per_kmer"]))
    return 1 if "error" in run else 0


if __name__ == "__main__":
    sys.exit(main())
