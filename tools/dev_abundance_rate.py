#!/usr/bin/env python3
"""Times the k-mer abundance calls on one MI355X: K = 31, PREFIX_BITS = 24, non-canonical or, with --canonical, canonical. Recorded, not asserted; the
results are in profiles/abundance_rate.md. The index is tools/dev_tips_rate.py's (1 M reads of 150 bases from cbl_amd.synth plus a second copy of every tenth
read with one substituted base: 121.5 M k-mers); the batch is those 1 M reads (120 M occurrences, all held).

    python tools/dev_abundance_rate.py [--canonical] [--reads 1000000] [--steps 5] [--timeout 1100]
    python tools/dev_abundance_rate.py [...] --child --only tally|coverage|filter --steps 1      # nothing but those calls: the run to put under a kernel trace
    CBLX_LIB_PATH=<a library without the feature> python tools/dev_abundance_rate.py [...] --child --parts

Rows (wall time around calls that return after the device is done), best of `--steps` after one warm-up, in one process; a call that changes the index runs on
a copy of it (`a | empty` into one second index, outside the timed region):
  (a) abundance_seqs_device of the batch into a zeroed array;
  (b) unitig_coverage_device(counts), and gfa_tagged_to_file(path on tmpfs, counts);
  (c) abundance_filter(counts, min_count) under the k-mer rule and under the unitig rule, min_count = what CBL.solid_threshold picks on the spectrum of a
      tally of the batch plus a second tally of its first half (so that the spectrum has two peaks); --min-count overrides;
  (d) the contended tally: a batch of poly-A reads (every occurrence is one k-mer, which the index is made to hold) through abundance_seqs_device; and, with
      --dup (a run of its own, in both modes), bench.py's `--config dup` reads — 8 M windows of 150 bases at uniform random positions of one random genome of
      40 Mbp, every k-mer about 24 times — against their own index: abundance_seqs_device here, rank_device + torch.bincount under --parts.
--parts uses nothing this feature added, so that a library built from the parent commit can run it: (a') rank_device on the same occurrences handed over as
packed k-mers (made with torch beforehand, not timed) plus torch.bincount of the ranks; (b') one tips_mark_device call and gfa_to_file; (c') one export sweep
and one remove_words_device of the words the k-mer rule removes (selected with torch from the same counts, which (a') makes). Checked in the same process: the
counts of (a) add up to `found`; the spectrum adds up to the index; sum(kc) = sum(counts); (c) leaves kmers - removed_kmers k-mers; the checksum the k-mer
rule leaves is printed by both modes. The child runs under a time limit; nothing is started after one that fails."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (str(ROOT), str(ROOT / "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

K, PB, LENGTH = 31, 24, 150


def batch(torch, a, dev):
    from cbl_amd import synth

    return synth.reads_torch(42, a.reads, LENGTH, device=dev)


def packed_kmers(torch, b, n):
    """The k-mers of n clean reads of LENGTH bases as packed int64 (2 bits per base, b"ACTG"[code], first base most significant), read after read."""
    lut = torch.zeros(256, dtype=torch.int64, device=b.device)
    for code, ch in enumerate(b"ACTG"):
        lut[ch] = code
    codes = lut[b[: n * LENGTH].to(torch.int64)].view(n, LENGTH)
    nk = LENGTH - K + 1
    out = torch.zeros((n, nk), dtype=torch.int64, device=b.device)
    for i in range(K):
        out = (out << 2) | codes[:, i: i + nk]
    return out.reshape(-1)


def two_peak_counts(torch, g, b, o, n):
    """A tally of the batch plus one of its first half: most k-mers at 1 or 2, the copies' own k-mers at 0."""
    counts, _, _ = g.abundance_seqs_device(b, o, n)
    g.abundance_seqs_device(b, o[: n // 2 + 1].clone(), n // 2, counts)
    return counts


def dup_reads(torch, a, dev):
    """bench.py's --config dup reads (rank 0): windows of one random genome (splitmix64 seed 4242) at uniform random positions (torch generator seed 7)."""
    from cbl_amd import synth

    n, genome = a.dup_reads, a.dup_genome
    gen, _ = synth.reads_torch(4242, 1, genome, device=dev)
    gtor = torch.Generator(device=dev)
    gtor.manual_seed(7)
    pos = torch.randint(0, genome - LENGTH, (n,), device=dev, dtype=torch.int64, generator=gtor)
    ar = torch.arange(LENGTH, device=dev)
    b = torch.cat([gen[(pos[i:i + 1_000_000, None] + ar[None, :]).reshape(-1)] for i in range(0, n, 1_000_000)] + [torch.zeros(16, dtype=torch.uint8, device=dev)])
    return b, torch.arange(0, (n + 1) * LENGTH, LENGTH, device=dev, dtype=torch.int64)


def dup(a):
    """Row (d)'s duplicate-heavy batch, in either mode."""
    import torch

    import cbl_amd
    from dev_tips_rate import timed

    dev = torch.device("cuda", 0)
    n = a.dup_reads
    b, o = dup_reads(torch, a, dev)
    g = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    g.insert_seqs_device(b, o, n)
    g.flush()
    nk = g.count()
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "dup_reads": n, "dup_genome": a.dup_genome, "index_kmers": nk, "occurrences": n * (LENGTH - K + 1)}
    last = {}
    if a.parts:
        kmers = torch.cat([packed_kmers(torch, b[i * LENGTH:], min(1_000_000, n - i)) for i in range(0, n, 1_000_000)])
        rank = torch.empty(kmers.numel(), dtype=torch.int64, device=dev)

        def rank_bincount():
            g.rank_device(kmers, None, kmers.numel(), rank)
            last["counts"] = torch.bincount(rank, minlength=nk)  # (every occurrence is held)

        out["dup_rank_bincount_ms"] = timed(rank_bincount, a.steps)
        out["dup_rank_device_ms"] = timed(lambda: g.rank_device(kmers, None, kmers.numel(), rank), a.steps)
        counts = last["counts"]
    else:
        counts = torch.zeros(nk, dtype=torch.int32, device=dev)

        def tally():
            counts.zero_()
            torch.cuda.synchronize()
            last["r"] = g.abundance_seqs_device(b, o, n, counts)

        out["dup_abundance_seqs_device_ms"] = timed(tally, a.steps)
        assert last["r"][1] == last["r"][2] == out["occurrences"]
    out["counts_sum"], out["counts_max"] = int(counts.to(torch.int64).sum()), int(counts.max())
    assert out["counts_sum"] == out["occurrences"]
    print(json.dumps(out), flush=True)
    return 0


def parts(a):
    import torch

    import cbl_amd
    import dev_tips_rate
    from dev_tips_rate import timed

    dev = torch.device("cuda", 0)
    g, empty = dev_tips_rate.build(a, dev)
    n = g.count()
    b, o = batch(torch, a, dev)
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "index_kmers": n}
    kmers = packed_kmers(torch, b, a.reads)
    out["occurrences"] = int(kmers.numel())
    rank = torch.empty(kmers.numel(), dtype=torch.int64, device=dev)
    last = {}

    def rank_bincount():
        g.rank_device(kmers, None, kmers.numel(), rank)
        last["counts"] = torch.bincount(rank[rank >= 0], minlength=n)

    out["rank_bincount_ms"] = timed(rank_bincount, a.steps)
    out["rank_device_ms"] = timed(lambda: g.rank_device(kmers, None, kmers.numel(), rank), a.steps)
    counts = last.pop("counts")
    half = (a.reads // 2) * (LENGTH - K + 1)
    g.rank_device(kmers[:half], None, half, rank[:half])
    counts += torch.bincount(rank[:half][rank[:half] >= 0], minlength=n)
    del kmers, rank
    out["tips_mark_device_ms"] = timed(lambda: g.tips_mark_device(), a.steps)
    with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
        out["gfa_to_file_ms"] = timed(lambda: g.gfa_to_file(os.path.join(tmp, "g.gfa")), a.steps)
    d_lo = torch.empty(n, dtype=torch.int64, device=dev)
    out["export_sweep_ms"] = timed(lambda: g.export_kmers_range_device(0, n, d_lo), a.steps)
    del d_lo
    mc = a.min_count or cbl_amd_solid(torch, counts)
    out["min_count"] = mc
    sel = counts < mc
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

    def remove(h):
        if ns:
            h.remove_words_device(w_lo, w_hi, ns)
        last["left"], last["checksum"] = h.count(), h.checksum()

    h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
    out["remove_words_ms"] = timed(remove, a.steps, before=lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h))
    out["kmers_left"], out["checksum_left"] = last["left"], last["checksum"]
    out["filter_parts_sum_ms"] = round(min(out["export_sweep_ms"]) + min(out["remove_words_ms"]), 3)
    print(json.dumps(out), flush=True)
    return 0


def cbl_amd_solid(torch, counts):
    """CBL.solid_threshold's rule on a torch array of counts (so that --parts needs no new method): 1 when the spectrum has no valley."""
    h = torch.bincount(counts.clamp(max=255).to(torch.int64), minlength=256).tolist()
    j = 1
    while j + 1 < len(h):
        if h[j + 1] > h[j]:
            while j > 1 and h[j - 1] == h[j]:
                j -= 1
            return j
        j += 1
    return 1


def child(a):
    import torch

    import cbl_amd
    import dev_tips_rate
    from dev_tips_rate import timed

    dev = torch.device("cuda", 0)
    g, empty = dev_tips_rate.build(a, dev)
    n = g.count()
    b, o = batch(torch, a, dev)
    out = {"lib": str(cbl_amd.LIB_PATH), "canonical": a.canonical, "reads": a.reads, "index_kmers": n}
    counts = torch.zeros(n, dtype=torch.int32, device=dev)
    last = {}

    def tally():
        counts.zero_()
        torch.cuda.synchronize()
        last["r"] = g.abundance_seqs_device(b, o, a.reads, counts)

    if a.only in (None, "tally"):
        out["abundance_seqs_device_ms"] = timed(tally, a.steps)
        _, total, found = last["r"]
        out["total"], out["found"] = total, found
        assert int(counts.to(torch.int64).sum()) == found and total == a.reads * (LENGTH - K + 1)
        out["tally_ns_per_occurrence"] = round(min(out["abundance_seqs_device_ms"]) * 1e6 / total, 3)
        # (d) the contended batch: poly-A reads against an index that holds poly-A
        ga = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
        ga.insert_seq(b"A" * K)
        ga.flush()
        m = a.reads // 10
        pa = torch.full((m * LENGTH + 16,), ord("A"), dtype=torch.uint8, device=dev)
        ca = torch.zeros(1, dtype=torch.int32, device=dev)
        out["poly_a_tally_ms"] = timed(lambda: last.update(pa=ga.abundance_seqs_device(pa, o[: m + 1].clone(), m, ca)), a.steps)
        out["poly_a_occurrences"] = last["pa"][1]
        out["poly_a_ns_per_occurrence"] = round(min(out["poly_a_tally_ms"]) * 1e6 / last["pa"][1], 3)
        assert last["pa"][1] == last["pa"][2] == m * (LENGTH - K + 1)
        ga.close()
    if a.only == "tally":
        print(json.dumps(out), flush=True)
        return 0
    counts = two_peak_counts(torch, g, b, o, a.reads)
    hist = g.abundance_histogram(counts)
    assert int(hist.sum()) == n
    mc = a.min_count or cbl_amd.CBL.solid_threshold(hist) or 1
    out["min_count"], out["spectrum_head"] = mc, [int(v) for v in hist[:6]]
    if a.only in (None, "coverage"):
        out["unitig_coverage_device_ms"] = timed(lambda: last.update(kc=g.unitig_coverage_device(counts)), a.steps)
        assert int(last["kc"].sum()) == int(counts.to(torch.int64).sum())
        out["unitigs"] = int(last.pop("kc").numel())
        with tempfile.TemporaryDirectory(dir="/dev/shm" if os.path.isdir("/dev/shm") else None) as tmp:
            out["gfa_tagged_to_file_ms"] = timed(lambda: last.update(t=g.gfa_tagged_to_file(os.path.join(tmp, "g.gfa"), counts)), a.steps)
            out["gfa_to_file_ms"] = timed(lambda: g.gfa_to_file(os.path.join(tmp, "g.gfa")), a.steps)
        out["tagged_text_bytes"] = last["t"][2]
    if a.only in (None, "filter"):
        h = cbl_amd.CBL(K, PB, canonical=a.canonical, device=0)
        copy = lambda: cbl_amd.CBL.set_op(g, empty, "or", out=h)  # noqa: E731
        for name, unitigs in (("kmer_rule", False), ("unitig_rule", True)):
            def run(h, unitigs=unitigs):
                last["st"] = h.abundance_filter(counts, mc, unitigs=unitigs)
                last["checksum"] = h.checksum()
            out[f"filter_{name}_ms"] = timed(run, a.steps, before=copy)
            st = out[f"filter_{name}_stats"] = last["st"]
            out[f"filter_{name}_checksum"] = last["checksum"]
            assert st["kmers_left"] == n - st["removed_kmers"]
    print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--canonical", action="store_true", help="a canonical index: the bidirected form")
    ap.add_argument("--reads", type=int, default=1_000_000)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--min-count", type=int, default=0, help="the threshold of row (c); 0: what solid_threshold picks (1 when the spectrum has no valley)")
    ap.add_argument("--only", choices=("tally", "coverage", "filter"), help="only those calls (for a kernel trace)")
    ap.add_argument("--parts", action="store_true", help="the rows a library without the feature can run")
    ap.add_argument("--dup", action="store_true", help="only row (d)'s duplicate-heavy batch (with --parts: its rank_device + bincount)")
    ap.add_argument("--dup-reads", type=int, default=8_000_000)
    ap.add_argument("--dup-genome", type=int, default=40_000_000)
    ap.add_argument("--timeout", type=float, default=1100.0, help="seconds the child may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return dup(a) if a.dup else parts(a) if a.parts else child(a)
    cmd = [sys.executable, str(Path(__file__).resolve()), "--child", "--reads", str(a.reads), "--steps", str(a.steps), "--min-count", str(a.min_count)] + \
        (["--only", a.only] if a.only else []) + (["--parts"] if a.parts else []) + (["--canonical"] if a.canonical else []) + \
        (["--dup", "--dup-reads", str(a.dup_reads), "--dup-genome", str(a.dup_genome)] if a.dup else [])
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
