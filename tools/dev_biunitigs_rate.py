#!/usr/bin/env python3
"""Times the bidirected-unitig calls on one MI355X: K = 31, PREFIX_BITS = 24, the CANONICAL index of 1 M reads of 150 bases from cbl_amd.synth.
Recorded, not asserted; the results are in profiles/biunitigs_rate.md.

    python tools/dev_biunitigs_rate.py [--reads 1000000] [--steps 5] [--baseline-kmers 4194304] [--timeout 1100]
    python tools/dev_biunitigs_rate.py --child --only-table --steps 1      # nothing but biunitig_table_device calls: the run to put under a kernel trace
    python tools/dev_biunitigs_rate.py --child --only-text --steps 1       # ... biunitigs_text_device calls

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process:
  (a) the way to the bidirected unitigs on the parent commit: kmers_np and neighbors_range_np of a range (9 bytes per k-mer over PCIe), then a walk on the
      host — a dict from stored k-mer to ordinal, the simple edges between oriented k-mers, one pass along them and the choice of an image. Over the first
      `--baseline-kmers` k-mers of the iteration order only, an edge that leaves the range counting as none; reported per k-mer;
  (b) biunitig_table_device over the whole index;
  (c) biunitigs_text_device into a device tensor;
  (d) biunitigs_to_file.
Checked in the same process: the lengths of (b) add up to count(), the heads ascend, `reversed` holds 0 / 1, the text of (c) has count() + U K bytes and U
lines, and the file of (d) holds the bytes of (c). The child runs under a time limit; nothing is started after one that fails."""
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


def _rc(x):
    """Reverse complement of packed K-mers (uint64 array; complement = code ^ 2)."""
    import numpy as np

    u = np.uint64
    x = ((x >> u(2)) & u(0x3333333333333333)) | ((x & u(0x3333333333333333)) << u(2))
    x = ((x >> u(4)) & u(0x0F0F0F0F0F0F0F0F)) | ((x & u(0x0F0F0F0F0F0F0F0F)) << u(4))
    x = x.byteswap() ^ u(0xAAAAAAAAAAAAAAAA)
    return x >> u(2 * (32 - K))


def _odd(x):
    """True where the packed k-mer has an odd number of set bits: the form that is not stored."""
    import numpy as np

    for sh in (32, 16, 8, 4, 2, 1):
        x = x ^ (x >> np.uint64(sh))
    return (x & np.uint64(1)).astype(bool)


def host_walk(lo, masks):
    """Bidirected unitigs of the stored k-mers lo[0 .. m) (ordinal = index) from their neighbour masks, on one host core: (unitigs, mirror pairs of simple
    edges). Ids are 2 i + s as on the device."""
    import numpy as np

    m = len(lo)
    mask = np.uint64((1 << (2 * K)) - 1)
    pop = np.array([bin(v).count("1") for v in range(16)], dtype=np.uint8)
    code_of = np.array([0, 0, 1, 0, 2, 0, 0, 0, 3], dtype=np.uint64)
    ordinal = {x: i for i, x in enumerate(lo.tolist())}
    in4 = masks >> 4
    nibble = (masks & 15, ((in4 & 3) << 2) | (in4 >> 2))  # the out-nibble of (i, 0) and of (i, 1)
    indeg = (pop[in4].tolist(), pop[masks & 15].tolist())  # in(r, 0), in(r, 1)
    nxt = [-1] * (2 * m)
    has_prev = [False] * (2 * m)
    edges = 0
    for s in (0, 1):
        one_out = np.flatnonzero(pop[nibble[s]] == 1)
        z = _rc(lo[one_out]) if s else lo[one_out]
        y = ((z << np.uint64(2)) | code_of[nibble[s][one_out]]) & mask
        t = _odd(y)
        stored = np.where(t, _rc(y), y)
        for i, w, tt in zip(one_out.tolist(), stored.tolist(), t.tolist()):
            r = ordinal.get(w, -1)
            if r >= 0 and r != i and indeg[tt][r] == 1:
                nxt[2 * i + s] = 2 * r + tt
                has_prev[2 * r + tt] = True
                edges += 1
    seen = [False] * (2 * m)
    unitigs = 0
    for h in range(2 * m):  # the paths: of each mirror pair the image whose head has the smaller ordinal
        if has_prev[h]:
            continue
        v = last = h
        while v >= 0:
            seen[v] = True
            last = v
            v = nxt[v]
        if (h >> 1) < (last >> 1) or ((h >> 1) == (last >> 1) and not h & 1):
            unitigs += 1
    for h in range(2 * m):  # what is left: cycles, from their smallest id; the image whose head is not reversed
        if seen[h]:
            continue
        v = h
        while not seen[v]:
            seen[v] = True
            v = nxt[v]
        unitigs += not h & 1
    return unitigs, edges // 2


def child(a):
    import numpy as np
    import torch

    import cbl_amd
    from cbl_amd import synth

    dev = torch.device("cuda", 0)
    n = a.reads
    g = cbl_amd.CBL(K, PB, canonical=True, device=0)
    b, o = synth.reads_torch(42, n, LENGTH, device=dev)
    g.insert_seqs_device(b, o, n)
    del b, o
    count = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "reads": n, "index_kmers": count}

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
    unitig, offset, head, length = (torch.empty(count, dtype=torch.int32, device=dev) for _ in range(4))
    rev, flags = torch.empty(count, dtype=torch.uint8, device=dev), torch.empty(count, dtype=torch.uint8, device=dev)
    counts = [C.c_uint64(0) for _ in range(3)]

    def table():
        g._chk(L.cblx_biunitig_table_device(g._h, unitig.data_ptr(), offset.data_ptr(), rev.data_ptr(), count, head.data_ptr(), length.data_ptr(), flags.data_ptr(),
                                            count, *[C.byref(c) for c in counts]))

    if a.only_table:
        out["biunitig_table_device_ms"] = timed(table, a.steps)
        print(json.dumps(out), flush=True)
        return 0
    nbytes, nu = g.biunitigs_text_device()
    d_text = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    if a.only_text:
        out["biunitigs_text_device_ms"] = timed(lambda: g.biunitigs_text_device(d_text, nbytes), a.steps)
        print(json.dumps(out), flush=True)
        return 0

    m = min(a.baseline_kmers, count)
    base = {}

    def baseline():
        lo, _ = g.kmers_np(0, m)
        masks = g.neighbors_range_np(0, m)
        base["unitigs"], base["edges"] = host_walk(lo, masks)

    out["baseline_kmers"] = m
    out["baseline_ms"] = timed(baseline, a.baseline_steps, warm=0)
    out["baseline_unitigs"], out["baseline_simple_edges"] = base["unitigs"], base["edges"]
    out["biunitig_table_device_ms"] = timed(table, a.steps)
    n_k, n_u, n_c = (c.value for c in counts)
    out["unitigs"], out["circular"] = n_u, n_c
    ln = length[:n_u].to(torch.int64)
    assert n_k == count and int(ln.sum()) == count, "the lengths do not add up to count()"
    hd = head[:n_u].to(torch.int64) & 0xFFFFFFFF
    assert bool((hd[1:] > hd[:-1]).all()), "the heads do not ascend"
    assert int(rev.max()) <= 1, "reversed holds something else than 0 / 1"
    out["reversed_kmers"] = int(rev.to(torch.int64).sum())
    out["longest"] = int(ln.max())
    out["summary"] = cbl_amd.CBL.unitig_summary(ln.cpu().numpy(), flags[:n_u].cpu().numpy(), K)
    assert (nbytes, nu) == (count + n_u * K, n_u)
    out["text_bytes"] = nbytes
    out["biunitigs_text_device_ms"] = timed(lambda: g.biunitigs_text_device(d_text, nbytes), a.steps)
    assert int((d_text == 10).sum()) == n_u and int(d_text[-1]) == 10, "the text does not hold U lines"
    with tempfile.TemporaryDirectory(dir=a.tmp) as tmp:
        path = os.path.join(tmp, "unitigs.txt")
        out["biunitigs_to_file_ms"] = timed(lambda: g.biunitigs_to_file(path), a.steps)
        data = np.fromfile(path, dtype=np.uint8)
    assert np.array_equal(data, d_text.cpu().numpy()), "the file differs from the device text"
    out["baseline_ns_per_kmer"] = round(min(out["baseline_ms"]) * 1e6 / m, 3)
    for key in ("biunitig_table_device", "biunitigs_text_device", "biunitigs_to_file"):
        out[key + "_ns_per_kmer"] = round(min(out[key + "_ms"]) * 1e6 / count, 3)
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--baseline-kmers", type=int, default=1 << 22, help="k-mers row (a) takes, from the head of the iteration order")
    ap.add_argument("--baseline-steps", type=int, default=1, help="timed steps of row (a): a step is tens of seconds of host work")
    ap.add_argument("--only-table", action="store_true", help="only biunitig_table_device calls (for a kernel trace)")
    ap.add_argument("--only-text", action="store_true", help="only biunitigs_text_device calls (for a kernel trace)")
    ap.add_argument("--tmp", default=None, help="directory for the file of row (d)")
    ap.add_argument("--timeout", type=float, default=1100.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps), "--baseline-kmers", str(a.baseline_kmers),
           "--baseline-steps", str(a.baseline_steps)] + (["--only-table"] if a.only_table else []) + (["--only-text"] if a.only_text else [])
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
    if not (a.only_table or a.only_text):
        f = lambda v: "%.3f – %.3f, best %.3f" % (min(v), max(v), min(v))  # noqa: E731
        print("| row | k-mers | ms | ns per k-mer |\n|---|---|---|---|")
        print("| (a) host baseline | %d | %s | %.3f |" % (run["baseline_kmers"], f(run["baseline_ms"]), run["baseline_ns_per_kmer"]))
        for row, key in (("(b) biunitig_table_device", "biunitig_table_device"), ("(c) biunitigs_text_device", "biunitigs_text_device"),
                         ("(d) biunitigs_to_file", "biunitigs_to_file")):
            print("| %s | %d | %s | %.3f |" % (row, run["index_kmers"], f(run[key + "_ms"]), run[key + "_ns_per_kmer"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
