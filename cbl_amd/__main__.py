"""`python -m cbl_amd <command>` — the build / insert / remove / merge / inter / diff / sym-diff / count / query / list / repartition subcommands of the
reference CLI (/root/reference/examples/cbl.rs:147-167,230-269,270-309,168-229,310-366) on the MI355X path, and merge-all / inter-all: the library's `CBL::merge` and
`CBL::intersect` (src/cbl.rs:106-124) over two or more index files, which the reference's CLI does not expose; `compare` prints the shared k-mers, Jaccard and
containment of every pair of two or more index files; `classify` assigns every record of a FASTA/Q file to one of two or more index files; `graph` prints
the degree table of the de Bruijn graph whose nodes are the k-mers of an index; `unitigs` writes the non-branching paths of that graph, one line each
(of a canonical index: the bidirected unitigs); `clip` removes the short dead-end unitigs (tips) of that graph from an index; `components`
prints the connected components of that graph, or removes the small ones (or all but the largest) from an index; `abundance` counts how often
the reads of FASTA/Q files hold every k-mer of an index, and prints the spectrum, writes the GFA text with LN / KC tags or removes the weak k-mers; `pop`
removes the weaker arms of the simple bubbles of that graph from an index, judged by the coverage of reads where they are given, by length otherwise.

K and PREFIX_BITS are compile-time constants of the reference (env K / PREFIX_BITS at cargo build time, build.rs:9-56);
here they are flags with the same defaults (K=25, PREFIX_BITS=24). Index files are interchangeable with the reference's.
"""
import argparse
import sys

from . import CBL


def _f1(x):
    """Rust's `{:.1}` of an f64 (a quotient by zero prints as NaN / inf there)."""
    if x != x:
        return "NaN"
    return ("inf" if x > 0 else "-inf") if x in (float("inf"), float("-inf")) else f"{x:.1f}"


def _div(a, b):
    a, b = int(a), int(b)
    return a / b if b else (float("nan") if a == 0 else float("inf"))


def repartition_report(prefix_bits, prefix, length, nodes):
    """The lines `cbl repartition` prints to stderr (examples/cbl.rs:313-365, same order and formatting) and the machine-readable stdout line
    `prefix_load n_buckets n_items max_prefix max_size vec_count vec_nodes trie_count trie_nodes total_nodes`, from the bucket table (numpy arrays,
    ascending prefixes). As in the reference a bucket counts as a "vec" when its NODE count is <= 1024, and the total adds the bucket count to the
    node counts. An empty index gives the load line and zeros (the reference panics on it)."""
    import numpy as np

    nb = len(prefix)
    load = nb / float(1 << prefix_bits)
    lines = [f"{_f1(load * 100.0)}% of the available prefixes are used"]
    if nb == 0:
        return lines, f"{load} 0 0 0 0 0 0 0 0 0"
    sizes, counts = np.unique(np.asarray(length, dtype=np.int64), return_counts=True)
    sizes, counts = sizes.tolist(), counts.tolist()
    total_buckets, total_items = sum(counts), sum(s * c for s, c in zip(sizes, counts))
    lines.append(f"The average bucket size is {_f1(_div(total_items, total_buckets))} items")
    bucket_count = item_count = 0
    for size, count in zip(sizes, counts):
        bucket_count += count
        item_count += size * count
        if count > total_buckets // 100 // 2 or size * count > total_items // 100 // 2 or bucket_count == total_buckets:
            lines.append(f"{_f1(_div(item_count * 100, total_items))}% of items are in a bucket of size \u2264 {size} ({_f1(_div(bucket_count * 100, total_buckets))}% of buckets)")
    ln = np.asarray(length, dtype=np.int64)
    at = nb - 1 - int(np.argmax(ln[::-1]))  # Iterator::max_by_key keeps the last of equal maxima
    max_prefix, max_size = int(prefix[at]), int(ln[at])
    lines.append(f"The biggest bucket (of size {max_size}) corresponds to prefix {max_prefix}")
    nd = np.asarray(nodes, dtype=np.uint64)
    small = nd <= 1024
    vec_count, trie_count = int(small.sum()), int((~small).sum())
    vec_nodes, trie_nodes = sum(nd[small].tolist()), sum(nd[~small].tolist())
    lines.append(f"{vec_count} vecs, average node count = {_f1(_div(vec_nodes, vec_count))}")
    lines.append(f"{trie_count} tries, average node count = {_f1(_div(trie_nodes, trie_count))}")
    total = total_buckets + vec_nodes + trie_nodes
    lines.append(f"{total} nodes in total")
    return lines, f"{load} {total_buckets} {total_items} {max_prefix} {max_size} {vec_count} {vec_nodes} {trie_count} {trie_nodes} {total}"


def compare_report(counts):
    """What `cbl compare` prints, from the (n, n) matrix of CBL.intersection_matrix (diagonal: the counts). Per unordered pair i < j one stdout line
    `i j count_i count_j common union jaccard containment_i_in_j containment_j_in_i`, tab-separated, the three ratios with six decimals, and one
    sentence for stderr. Host only."""
    n = len(counts)
    lines, human = [], []
    for i in range(n):
        for j in range(i + 1, n):
            ci, cj = int(counts[i][i]), int(counts[j][j])
            s = CBL.similarity(ci, cj, int(counts[i][j]))
            lines.append("\t".join([str(i), str(j), str(ci), str(cj), str(s["common"]), str(s["union"]), f"{s['jaccard']:.6f}",
                                    f"{s['containment_a_in_b']:.6f}", f"{s['containment_b_in_a']:.6f}"]))
            human.append(f"Indexes {i} and {j} share {s['common']} of {ci} and {cj} k-mers (Jaccard {s['jaccard']:.6f})")
    return lines, human


def occupancy_report(hist):
    """What `cbl occupancy` prints, from CBL.occupancy's hist[0 .. n]: one stdout line `j<TAB>count` for j = 1 .. n — the distinct k-mers exactly j of
    the n indexes hold — and sentences for stderr: the size of the union, of the core (held by all) and of the cloud (held by one). Host only."""
    hist = [int(v) for v in hist]
    n = len(hist) - 1
    if n < 1 or hist[0] != 0:
        raise ValueError("occupancy_report: hist[0 .. n] of n >= 1 indexes, hist[0] = 0")
    lines = [f"{j}\t{hist[j]}" for j in range(1, n + 1)]
    human = [f"The {n} indexes hold {sum(hist)} distinct k-mers", f"{hist[n]} are held by all of them, {hist[1]} by exactly one"]
    return lines, human


def classify_report(total, positive, assigned):
    """What `cbl classify` prints, from the table of CBL.contains_seqs_counts_many (total[nseq], positive[n][nseq]) and CBL.classify's
    assigned[nseq]: one stdout line per record — its 0-based position in the file, the k-mers queried, the n hit counts and the assigned index or
    `-`, tab-separated — then the summary: one line `index<TAB>reads` per index and `unassigned<TAB>reads`; and sentences for stderr. Host only."""
    total = [int(t) for t in total]
    positive = [[int(v) for v in row] for row in positive]
    assigned = [int(a) for a in assigned]
    n = len(positive)
    if any(len(row) != len(total) for row in positive) or len(assigned) != len(total) or any(not -1 <= a < n for a in assigned):
        raise ValueError("classify_report: positive[n][nseq] and assigned[nseq] in -1 .. n - 1 for total[nseq]")
    lines = ["\t".join([str(s), str(t)] + [str(row[s]) for row in positive] + [str(assigned[s]) if assigned[s] >= 0 else "-"]) for s, t in enumerate(total)]
    per = [sum(1 for a in assigned if a == j) for j in range(n)]
    none = sum(1 for a in assigned if a < 0)
    summary = [f"{j}\t{per[j]}" for j in range(n)] + [f"unassigned\t{none}"]
    human = [f"{len(total)} records against {n} indexes: {len(total) - none} assigned, {none} unassigned"]
    human += [f"Index {j} takes {per[j]} records" for j in range(n)]
    return lines, summary, human


def graph_report(table):
    """What `cbl graph` prints, from CBL.degree_table's table[out][in]: five stdout lines, row `out` = 0 .. 4 with its five counts for `in` = 0 .. 4,
    tab-separated, then one line `key<TAB>value` per entry of CBL.degree_summary in its order; and sentences for stderr. Host only."""
    rows = [[int(v) for v in row] for row in table]
    if len(rows) != 5 or any(len(row) != 5 for row in rows):
        raise ValueError("graph_report: table[5][5], indexed [out][in]")
    s = CBL.degree_summary(rows)
    lines = ["\t".join(str(v) for v in row) for row in rows]
    summary = [f"{key}\t{value}" for key, value in s.items()]
    human = [f"The de Bruijn graph of the index has {s['nodes']} nodes, {s['out_edges']} outgoing and {s['in_edges']} incoming edges",
             f"{s['simple']} nodes lie on simple paths, {s['branching']} branch, {s['sources']} are sources, {s['sinks']} sinks and {s['isolated']} isolated"]
    return lines, summary, human


def unitigs_report(summary):
    """What `cbl unitigs --stats` prints, from CBL.unitig_summary: one stdout line `key<TAB>value` per entry in its order; and a sentence for stderr.
    Host only."""
    lines = [f"{key}\t{value}" for key, value in summary.items()]
    human = [f"The {summary['kmers']} k-mers of the index form {summary['unitigs']} unitigs ({summary['circular']} circular) of {summary['bases']} bases; "
             f"the longest has {summary['longest']} k-mers, N50 is {summary['n50']} bases"]
    return lines, human


def abundance_report(total, found, hist):
    """What `cbl abundance` prints, from the totals of CBL.abundance_seqs* and the spectrum of CBL.abundance_histogram: the machine-readable lines and a
    human summary. `solid_threshold` is the first valley of the spectrum (CBL.solid_threshold), `none` when it has none."""
    h = [int(v) for v in hist]
    kmers = sum(h)
    solid = CBL.solid_threshold(h)
    lines = [f"total\t{int(total)}", f"found\t{int(found)}", f"kmers\t{kmers}", f"unseen\t{h[0]}", f"once\t{h[1]}", f"saturated_bin\t{h[255]}",
             f"solid_threshold\t{'none' if solid is None else solid}"]
    human = [f"# k-mers of the reads: {int(total)}", f"# of them in the index: {int(found)} ({int(found) * 100 / total if total else float('nan'):.2f}%)",
             f"# k-mers of the index never seen: {h[0]} of {kmers}"]
    return lines, human


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m cbl_amd")
    ap.add_argument("-k", type=int, default=25, help="k-mer size (odd, <= 59); the reference bakes it in at build time")
    ap.add_argument("--prefix-bits", type=int, default=24)
    ap.add_argument("--device", type=int, default=-1)
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="Build an index containing the k-mers of a FASTA/Q file")
    b.add_argument("input")
    b.add_argument("-o", "--output")
    b.add_argument("-c", "--canonical", action="store_true")
    i = sub.add_parser("insert", help="Add the k-mers of a FASTA/Q file to an index")
    i.add_argument("index")
    i.add_argument("input")
    i.add_argument("-o", "--output")
    r = sub.add_parser("remove", help="Remove the k-mers of a FASTA/Q file from an index")
    r.add_argument("index")
    r.add_argument("input")
    r.add_argument("-o", "--output")
    m = sub.add_parser("merge", help="Compute the union of two indexes")
    m.add_argument("first_index")
    m.add_argument("second_index")
    m.add_argument("-o", "--output")
    for name, what in (("inter", "intersection"), ("diff", "difference"), ("sym-diff", "symmetric difference")):  # examples/cbl.rs:280-309
        s = sub.add_parser(name, help=f"Compute the {what} of two indexes")
        s.add_argument("first_index")
        s.add_argument("second_index")
        s.add_argument("-o", "--output")
    for name, what in (("merge-all", "union"), ("inter-all", "intersection")):  # CBL::merge / CBL::intersect, src/cbl.rs:106-124
        s = sub.add_parser(name, help=f"Compute the {what} of two or more indexes")
        s.add_argument("indexes", nargs="+", metavar="index")
        s.add_argument("-o", "--output")
    al = sub.add_parser("at-least", help="Compute the k-mers held by at least T of two or more indexes")
    al.add_argument("-t", "--threshold", type=int, required=True, metavar="T")
    al.add_argument("indexes", nargs="+", metavar="index")
    al.add_argument("-o", "--output")
    oc = sub.add_parser("occupancy", help="Count the distinct k-mers held by exactly j of two or more indexes, j = 1 .. n. No index is built; Vec buckets on "
                                          "prefixes several indexes hold are sorted in memory, as a merge does")
    oc.add_argument("indexes", nargs="+", metavar="index")
    cmp_ = sub.add_parser("compare", help="Compare two or more indexes pairwise: shared k-mers, union, Jaccard, containment. Every file is loaded first, so "
                                           "all of them sit in device memory at once; no index is built or changed")
    cmp_.add_argument("indexes", nargs="+", metavar="index")
    cl = sub.add_parser("classify", help="Assign every record of a FASTA/Q file to the index, of two or more, that holds most of its k-mers. The whole "
                                         "file is staged in device memory at once; no index is changed")
    cl.add_argument("inputs", nargs="+", metavar="index ... reads", help="two or more index files, then the FASTA/Q file")
    cl.add_argument("--min-fraction", type=float, default=0.5, metavar="F", help="an index takes a record only if it holds at least this share of its k-mers")
    cl.add_argument("--min-hits", type=int, default=0, metavar="H", help="... and at least this many of them")
    cl.add_argument("-o", "--output", help="write the per-record lines and the summary there instead of stdout")
    c = sub.add_parser("count", help="Count the k-mers contained in an index")
    c.add_argument("index")
    q = sub.add_parser("query", help="Query an index for every k-mer contained in a FASTA/Q file")
    q.add_argument("index")
    q.add_argument("input")
    q.add_argument("--per-record", metavar="OUT", help="also write one line per record to OUT ('-': stdout): its 0-based position in the file, the k-mers "
                   "queried and the k-mers found, tab-separated")
    ls = sub.add_parser("list", help="List the k-mers contained in an index")
    ls.add_argument("index")
    ls.add_argument("-o", "--output")
    rp = sub.add_parser("repartition", help="Show statistics about the buckets of an index: sizes, node counts. An empty index prints the prefix load "
                                            "and zeros (the reference panics on an empty index)")
    rp.add_argument("index")
    gr = sub.add_parser("graph", help="Show the degree table of the de Bruijn graph whose nodes are the k-mers of an index: how many k-mers have `out` "
                                      "successors and `in` predecessors in the index, and a summary. The index is not changed")
    gr.add_argument("index")
    un = sub.add_parser("unitigs", help="Write the unitigs of an index, one line each: the maximal non-branching paths (and cycles) of the de Bruijn "
                                        "graph whose nodes are its k-mers; of a canonical index the bidirected unitigs, each in one of its two "
                                        "orientations. The index is not changed")
    un.add_argument("index")
    un.add_argument("-o", "--output")
    un_form = un.add_mutually_exclusive_group()
    un_form.add_argument("--stats", action="store_true", help="print a summary (unitigs, circular, k-mers, bases, longest, N50) instead of the lines")
    un_form.add_argument("--gfa", action="store_true", help="write the compacted graph as GFA 1.0 instead of the lines: an S line per unitig and an L line "
                                                            "per link between two unitigs, with an overlap of K - 1")
    cp = sub.add_parser("clip", help="Remove the tips of an index: the unitigs of at most N k-mers that are linked to the rest of the de Bruijn graph at "
                                     "one end only. A round removes every tip of one compaction together")
    cp.add_argument("index")
    cp.add_argument("-o", "--output", required=True)
    cp.add_argument("--max-kmers", type=int, default=None, metavar="N", help="the longest unitig that counts as a tip, in k-mers (default: K - 1)")
    cp.add_argument("--isolated", action="store_true", help="also remove the unitigs of at most N k-mers that are linked to nothing")
    cp.add_argument("--rounds", type=int, default=1, metavar="R", help="compact and clip up to R times (default 1); 0: until a round finds no tip")
    cc = sub.add_parser("components", help="Show the connected components of the de Bruijn graph whose nodes are the k-mers of an index, or, with -o, remove "
                                           "whole components from it: those of fewer than N k-mers, or all but the largest")
    cc.add_argument("index")
    cc.add_argument("-o", "--output", help="write the filtered index to OUT (needs --min-kmers or --largest)")
    cc.add_argument("--sizes", action="store_true", help="also print one line per component: its number, its k-mers and its unitigs, tab-separated")
    cc_rule = cc.add_mutually_exclusive_group()
    cc_rule.add_argument("--min-kmers", type=int, default=None, metavar="N", help="remove every component of fewer than N k-mers (N is at least 1)")
    cc_rule.add_argument("--largest", action="store_true", help="remove every component but the one of most k-mers")
    ab = sub.add_parser("abundance", help="Count how often the reads of one or more FASTA/Q files hold every k-mer of an index (both strands for a canonical "
                                          "index), print the abundance spectrum, write the compacted graph as GFA with LN and KC tags, or, with "
                                          "--min-count and -o, remove the weakly supported k-mers. Every file is staged in device memory at once")
    ab.add_argument("index")
    ab.add_argument("reads", nargs="+", help="FASTA/Q files, tallied one after the other into one array of counts")
    ab.add_argument("--hist", action="store_true", help="print the spectrum: a line `j<TAB>k-mers` for j = 0 .. 255 (the last one: 255 and more)")
    ab.add_argument("--min-count", type=int, default=None, metavar="N", help="remove every k-mer counted fewer than N times (N is at least 1; needs -o)")
    ab.add_argument("--unitigs", action="store_true", help="with --min-count: remove whole unitigs, those whose mean count is below N")
    ab.add_argument("-o", "--output", help="write the filtered index to OUT (needs --min-count)")
    ab.add_argument("--gfa", metavar="OUT.gfa", help="write the compacted graph of the index as loaded as GFA 1.0 with LN:i: and KC:i: tags on the S lines")
    pb = sub.add_parser("pop", help="Pop the simple bubbles of an index: where two to four unitigs of at most N k-mers each lead from one end of a unitig to "
                                    "the same end of another, keep the one of the highest mean coverage in the reads (without reads: the longest) and "
                                    "remove the others. A round removes every such arm of one compaction together")
    pb.add_argument("index")
    pb.add_argument("reads", nargs="*", help="FASTA/Q files, tallied one after the other into one array of counts; none: the longer arm is kept")
    pb.add_argument("-o", "--output", required=True)
    pb.add_argument("--max-kmers", type=int, default=None, metavar="N", help="the longest unitig that counts as an arm, in k-mers (default: 2 K)")
    pb.add_argument("--rounds", type=int, default=1, metavar="R", help="compact and pop up to R times (default 1); 0: until a round pops nothing")
    a = ap.parse_args(argv)
    if a.cmd == "pop" and ((a.max_kmers is not None and a.max_kmers < 1) or a.rounds < 0):  # refused before anything is loaded
        ap.error("pop: --max-kmers is at least 1 and --rounds at least 0")
    if a.cmd == "abundance":  # refused before anything is loaded
        if a.min_count is not None and a.min_count < 1:
            ap.error("abundance: --min-count is at least 1")
        if a.unitigs and a.min_count is None:
            ap.error("abundance: --unitigs needs --min-count")
        if (a.min_count is not None) != (a.output is not None):
            ap.error("abundance: --min-count needs -o, and -o needs --min-count")
    if a.cmd == "components":  # refused before anything is loaded
        if a.min_kmers is not None and a.min_kmers < 1:
            ap.error("components: --min-kmers is at least 1")
        if (a.min_kmers is not None or a.largest) != (a.output is not None):
            ap.error("components: -o needs exactly one of --min-kmers and --largest, and they need -o")

    if a.cmd == "build":
        cbl = CBL(a.k, a.prefix_bits, canonical=a.canonical, device=a.device)
        print(f"Building the index of {'canonical ' if a.canonical else ''}{a.k}-mers contained in {a.input}", file=sys.stderr)
        cbl.insert_fastx_file(a.input)
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd == "insert":
        print(f"Reading the index stored in {a.index}", file=sys.stderr)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"Adding the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.input} to the index", file=sys.stderr)
        cbl.insert_fastx_file(a.input)
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd == "remove":  # examples/cbl.rs:250-269
        print(f"Reading the index stored in {a.index}", file=sys.stderr)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"Removing the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.input} from the index", file=sys.stderr)
        cbl.remove_fastx_file(a.input)
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd == "merge":
        cbl = CBL.load_from_file(a.first_index, a.k, a.prefix_bits, device=a.device)
        cbl2 = CBL.load_from_file(a.second_index, a.k, a.prefix_bits, device=a.device)
        cbl |= cbl2
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd in ("inter", "diff", "sym-diff"):  # `cbl &= &mut cbl2`, `cbl -= &mut cbl2`, `cbl ^= &mut cbl2`
        cbl = CBL.load_from_file(a.first_index, a.k, a.prefix_bits, device=a.device)
        cbl2 = CBL.load_from_file(a.second_index, a.k, a.prefix_bits, device=a.device)
        cbl.set_op_assign(cbl2, {"inter": "and", "diff": "sub", "sym-diff": "xor"}[a.cmd])
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd in ("merge-all", "inter-all"):
        if len(a.indexes) < 2:
            ap.error(f"{a.cmd} takes two or more index files")
        cbls = [CBL.load_from_file(path, a.k, a.prefix_bits, device=a.device) for path in a.indexes]
        cbl = CBL.merge(cbls) if a.cmd == "merge-all" else CBL.intersect(cbls)
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd == "at-least":
        if len(a.indexes) < 2:
            ap.error("at-least takes two or more index files")
        if not 1 <= a.threshold <= len(a.indexes):
            ap.error(f"at-least: the threshold is 1 to the number of index files ({len(a.indexes)})")
        cbls = [CBL.load_from_file(path, a.k, a.prefix_bits, device=a.device) for path in a.indexes]
        cbl = CBL.at_least(cbls, a.threshold)
        print(f"{cbl.count()} {a.k}-mers are held by at least {a.threshold} of the {len(cbls)} indexes", file=sys.stderr)
        if a.output:
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
    elif a.cmd == "occupancy":
        if len(a.indexes) < 2:
            ap.error("occupancy takes two or more index files")
        cbls = [CBL.load_from_file(path, a.k, a.prefix_bits, device=a.device) for path in a.indexes]
        lines, human = occupancy_report(CBL.occupancy(cbls))
        print("\n".join(human), file=sys.stderr)
        print("\n".join(lines))
    elif a.cmd == "compare":
        if len(a.indexes) < 2:
            ap.error("compare takes two or more index files")
        cbls = [CBL.load_from_file(path, a.k, a.prefix_bits, device=a.device) for path in a.indexes]
        lines, human = compare_report(CBL.intersection_matrix(cbls))
        print("\n".join(human), file=sys.stderr)
        print("\n".join(lines))
    elif a.cmd == "classify":
        if len(a.inputs) < 3:
            ap.error("classify takes two or more index files and a FASTA/Q file")
        import torch

        cbls = [CBL.load_from_file(path, a.k, a.prefix_bits, device=a.device) for path in a.inputs[:-1]]
        reads = a.inputs[-1]
        print(f"Classifying the records of {reads} against {len(cbls)} indexes of {'canonical ' if cbls[0].is_canonical() else ''}{a.k}-mers", file=sys.stderr)
        stager = cbls[0]  # the whole file at once: one rank, one block no smaller than the record count
        nrec = stager.count_fastx_records(reads)
        d_bases, d_offsets, n, _ = stager.stage_fastx_blocks(reads, max(nrec, 1), 0, 1)
        try:
            dev = torch.device("cuda", stager.device())
            d_total = torch.empty(n, dtype=torch.int32, device=dev)
            d_positive = torch.empty((len(cbls), n), dtype=torch.int32, device=dev)
            if n:
                CBL.contains_seqs_counts_many_device(cbls, d_bases, d_offsets, n, d_total, d_positive)
        finally:
            stager.stage_release()
        total, positive = d_total.cpu().numpy().view("uint32"), d_positive.cpu().numpy().view("uint32")
        lines, summary, human = classify_report(total, positive, CBL.classify(total, positive, min_fraction=a.min_fraction, min_hits=a.min_hits))
        print("\n".join(human), file=sys.stderr)
        out = open(a.output, "w") if a.output else sys.stdout
        try:
            out.write("".join(line + "\n" for line in lines + summary))
        finally:
            if out is not sys.stdout:
                out.close()
    elif a.cmd == "count":
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"It contains {cbl.count()} {a.k}-mers", file=sys.stderr)
        print(cbl.count())
    elif a.cmd == "query":  # examples/cbl.rs:205-228
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"Querying the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.input}", file=sys.stderr)
        if a.per_record is None:
            _, total, positive = cbl.query_fastx_file(a.input)
        else:  # the parser keeps no record names: a record is known by its position in the file
            rec_total, rec_positive = cbl.query_fastx_file_counts(a.input)
            total, positive = int(rec_total.sum(dtype="uint64")), int(rec_positive.sum(dtype="uint64"))
            out = sys.stdout if a.per_record == "-" else open(a.per_record, "w")
            try:
                out.write("".join(f"{i}\t{t}\t{p}\n" for i, (t, p) in enumerate(zip(rec_total.tolist(), rec_positive.tolist()))))
            finally:
                if out is not sys.stdout:
                    out.close()
        print(f"# queries: {total}", file=sys.stderr)
        print(f"# positive queries: {positive} ({positive * 100 / total if total else float('nan'):.2f}%)", file=sys.stderr)
        print(total, positive)
    elif a.cmd == "list":  # examples/cbl.rs:177-203: one k-mer per line, IntKmer::to_nucs (first base most significant), streamed from the device
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"Listing {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.index}", file=sys.stderr)
        if a.output:
            cbl.list_to_file(a.output)
        else:
            sys.stdout.flush()
            cbl.list_to_fd(sys.stdout.fileno())
    elif a.cmd == "repartition":  # examples/cbl.rs:310-366
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        prefix, length, _ = cbl.bucket_table_np()
        lines, summary = repartition_report(a.prefix_bits, prefix, length, cbl.bucket_nodes_np())
        sys.stderr.flush()
        sys.stderr.buffer.write(("\n".join(lines) + "\n").encode("utf-8"))
        sys.stderr.buffer.flush()
        print(summary)
    elif a.cmd == "graph":  # ours (the reference's CLI has no such command): Kmer::successors / predecessors (src/kmer.rs:82-90) over CBL::iter
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"Counting the neighbours of the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.index}", file=sys.stderr)
        lines, summary, human = graph_report(cbl.degree_table())
        print("\n".join(human), file=sys.stderr)
        print("\n".join(lines + summary))
    elif a.cmd == "unitigs":  # ours (the reference's CLI has no such command): compaction over Kmer::successors / predecessors (src/kmer.rs:82-90)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        bi = cbl.is_canonical()  # a canonical index: the bidirected unitigs, over oriented k-mers
        print(f"Compacting the {'canonical ' if bi else ''}{a.k}-mers contained in {a.index} into {'bidirected ' if bi else ''}unitigs", file=sys.stderr)
        if a.stats:
            t = cbl.biunitig_table_np() if bi else cbl.unitig_table_np()
            lines, human = unitigs_report(CBL.unitig_summary(t["length"], t["flags"], a.k))
            print("\n".join(human), file=sys.stderr)
            out = "\n".join(lines) + "\n"
            if a.output:
                with open(a.output, "w") as f:
                    f.write(out)
            else:
                sys.stdout.write(out)
        elif a.gfa:
            if a.output:
                cbl.gfa_to_file(a.output)
            else:
                sys.stdout.flush()
                cbl.gfa_to_fd(sys.stdout.fileno())
        elif a.output:
            (cbl.biunitigs_to_file if bi else cbl.unitigs_to_file)(a.output)
        else:
            sys.stdout.flush()
            (cbl.biunitigs_to_fd if bi else cbl.unitigs_to_fd)(sys.stdout.fileno())
    elif a.cmd == "clip":  # ours (the reference's CLI has no such command): the removal is one WordSet::remove_batch per round (src/wordset/mod.rs:218-237)
        if (a.max_kmers is not None and a.max_kmers < 1) or a.rounds < 0:
            ap.error("clip: --max-kmers is at least 1 and --rounds at least 0")
        print(f"Reading the index stored in {a.index}", file=sys.stderr)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        print(f"Clipping the tips of the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.index}", file=sys.stderr)
        st = cbl.clip_tips(a.max_kmers, isolated=a.isolated, rounds=a.rounds)
        print(f"{st['rounds']} rounds removed {st['tips']} tips of {st['tip_kmers']} k-mers and {st['isolated']} isolated unitigs of {st['isolated_kmers']} "
              f"k-mers; {st['kmers_left']} k-mers are left{'' if st['fixpoint'] else ' (tips may remain)'}", file=sys.stderr)
        print(f"Writing the index to {a.output}", file=sys.stderr)
        cbl.save_to_file(a.output)
        print("\n".join(f"{key}\t{value}" for key, value in st.items()))
    elif a.cmd == "components":  # ours (the reference's CLI has no such command): the removal is one WordSet::remove_batch (src/wordset/mod.rs:218-237)
        print(f"Reading the index stored in {a.index}", file=sys.stderr)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        if a.output is None:
            print(f"Labelling the components of the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.index}", file=sys.stderr)
            t = cbl.components_np()
            sm = CBL.component_summary(t["kmers"], t["unitigs"])
            print(f"kmers\t{t['n_kmers']}\nunitigs\t{t['n_unitigs']}\nlinks\t{t['n_links']}\ncomponents\t{sm['components']}\nlargest\t{sm['largest']}\n"
                  f"singletons\t{sm['singletons']}\nlargest_fraction\t{sm['largest_fraction']:.6f}")
            if a.sizes:
                sys.stdout.write("".join(f"{c}\t{k}\t{u}\n" for c, (k, u) in enumerate(zip(t["kmers"].tolist(), t["unitigs"].tolist()))))
        else:
            print(f"Filtering the components of the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.index}", file=sys.stderr)
            st = cbl.components_filter(a.min_kmers, largest=a.largest)
            print(f"Removed {st['removed_components']} of {st['components']} components, {st['removed_kmers']} k-mers; {st['kmers_left']} k-mers are left",
                  file=sys.stderr)
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
            print("\n".join(f"{key}\t{value}" for key, value in st.items()))

    elif a.cmd == "abundance":  # ours (the reference's CLI has no such command): the counts live beside the index, never in it
        import torch

        print(f"Reading the index stored in {a.index}", file=sys.stderr)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        counts = torch.zeros(cbl.count(), dtype=torch.int32, device=torch.device("cuda", cbl.device()))
        total = found = 0
        for reads in a.reads:
            print(f"Counting the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers of {reads}", file=sys.stderr)
            nrec = cbl.count_fastx_records(reads)  # the whole file at once: one rank, one block no smaller than the record count
            d_bases, d_offsets, n, _ = cbl.stage_fastx_blocks(reads, max(nrec, 1), 0, 1)
            try:
                if n:
                    _, t, f = cbl.abundance_seqs_device(d_bases, d_offsets, n, counts)
                    total, found = total + t, found + f
            finally:
                cbl.stage_release()
        hist = cbl.abundance_histogram(counts)
        lines, human = abundance_report(total, found, hist)
        print("\n".join(human), file=sys.stderr)
        print("\n".join(lines))
        if a.hist:
            sys.stdout.write("".join(f"{j}\t{v}\n" for j, v in enumerate(hist.tolist())))
        if a.gfa:
            print(f"Writing the tagged GFA text to {a.gfa}", file=sys.stderr)
            cbl.gfa_tagged_to_file(a.gfa, counts)
        if a.output:
            st = cbl.abundance_filter(counts, a.min_count, unitigs=a.unitigs)
            print(f"Removed {st['removed_kmers']} of {st['kmers']} k-mers counted below {a.min_count}{' on average over their unitig' if a.unitigs else ''}; "
                  f"{st['kmers_left']} k-mers are left", file=sys.stderr)
            print(f"Writing the index to {a.output}", file=sys.stderr)
            cbl.save_to_file(a.output)
            print("\n".join(f"{key}\t{value}" for key, value in st.items()))

    elif a.cmd == "pop":  # ours (the reference's CLI has no such command): the removal is one WordSet::remove_batch per round (src/wordset/mod.rs:218-237)
        if a.reads:
            import torch  # (before the index is loaded, as in `abundance`: the counts are a torch tensor)

        print(f"Reading the index stored in {a.index}", file=sys.stderr)
        cbl = CBL.load_from_file(a.index, a.k, a.prefix_bits, device=a.device)
        counts = None
        if a.reads:
            counts = torch.zeros(cbl.count(), dtype=torch.int32, device=torch.device("cuda", cbl.device()))
            for reads in a.reads:
                print(f"Counting the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers of {reads}", file=sys.stderr)
                nrec = cbl.count_fastx_records(reads)  # the whole file at once, as `abundance` stages it
                d_bases, d_offsets, n, _ = cbl.stage_fastx_blocks(reads, max(nrec, 1), 0, 1)
                try:
                    if n:
                        cbl.abundance_seqs_device(d_bases, d_offsets, n, counts)
                finally:
                    cbl.stage_release()
        print(f"Popping the bubbles of the {'canonical ' if cbl.is_canonical() else ''}{a.k}-mers contained in {a.index}, by "
              f"{'coverage' if a.reads else 'length'}", file=sys.stderr)
        st = cbl.pop_bubbles(a.max_kmers, counts, rounds=a.rounds)
        st = st[0] if a.reads else st
        print(f"{st['rounds']} rounds popped {st['popped']} arms of {st['popped_kmers']} k-mers in {st['bubbles']} bubbles; {st['kmers_left']} k-mers are "
              f"left{'' if st['fixpoint'] else ' (bubbles may remain)'}", file=sys.stderr)
        print(f"Writing the index to {a.output}", file=sys.stderr)
        cbl.save_to_file(a.output)
        print("\n".join(f"{key}\t{value}" for key, value in st.items()))


if __name__ == "__main__":
    main()
