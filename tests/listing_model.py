"""CPU models of what reading an index out gives: a k-mer's text line, a bucket's node count, the `repartition` report. Pure Python;
tests/test_listing_model.py checks the closed form of the node count against a plain count and against the serialized Tries of the
CPU oracle, tests/test_gpu_listing.py checks the GPU path against these functions.

Reference: IntKmer::to_nucs /root/reference/src/kmer.rs:26-27,204-214 (code 0 -> A, 1 -> C, 2 -> T, 3 -> G, first base most
significant), TrieVec::count_nodes src/trievec/mod.rs:37-42, TrieNode::count_nodes src/trie.rs:90-102, the `Repartition` subcommand
examples/cbl.rs:310-366.
"""
from __future__ import annotations

from collections import Counter

NUCS = b"ACTG"
VEC, TRIE = 0, 1
REPARTITION_VEC_MAX_NODES = 1024  # examples/cbl.rs:348: a bucket counts as a "vec" when its NODE count is <= 1024


def to_nucs(kmer: int, k: int) -> bytes:
    """The k bases of a packed k-mer: base j is bits 2(k-1-j)+1 .. 2(k-1-j)."""
    return bytes(NUCS[(kmer >> (2 * (k - 1 - j))) & 3] for j in range(k))


def line(kmer: int, k: int) -> bytes:
    return to_nucs(kmer, k) + b"\n"


def text(kmers, k: int) -> bytes:
    return b"".join(line(x, k) for x in kmers)


def lcp_bytes(a: int, b: int, nbytes: int) -> int:
    """Leading big-endian bytes two nbytes-byte strings share."""
    n = 0
    for d in range(1, nbytes + 1):
        if a >> (8 * (nbytes - d)) != b >> (8 * (nbytes - d)):
            break
        n = d
    return n


def trie_nodes(suffixes, nbytes: int) -> int:
    """Nodes of the Trie over ascending, distinct suffixes of nbytes bytes, closed form: nbytes for the first suffix (the root and
    one node per proper prefix of length 1 .. nbytes - 1), then nbytes - 1 - lcp with the previous suffix for every other one."""
    s = list(suffixes)
    if not s:
        return 1  # an empty Trie still has its root (not reachable in an index: empty buckets leave it)
    return nbytes + sum(nbytes - 1 - lcp_bytes(s[j], s[j - 1], nbytes) for j in range(1, len(s)))


def trie_nodes_plain(suffixes, nbytes: int) -> int:
    """The same by counting: the root plus the distinct proper byte prefixes of every length."""
    s = list(suffixes)
    return 1 + sum(len({x >> (8 * (nbytes - d)) for x in s}) for d in range(1, nbytes))


def bucket_nodes(kind: int, suffixes, nbytes: int) -> int:
    """TrieVec::count_nodes: a Vec's length, a Trie's nodes."""
    return len(suffixes) if kind == VEC else trie_nodes(sorted(suffixes), nbytes)


# ---- the serialized index: node counts by walking the bytes --------------------------------------------
def _varint(b, p):
    t = b[p]
    if t <= 250:
        return t, p + 1
    n = {251: 2, 252: 4, 253: 8}[t]
    return int.from_bytes(b[p + 1 : p + 1 + n], "little"), p + 1 + n


def serialized_bucket_nodes(blob: bytes, nbytes: int):
    """[(prefix, kind, length, nodes)] of a serialized index: a Vec entry is varint(n) and n length-prefixed suffixes; a Trie entry
    is its root node — varint(c), c child bytes, varint(#children), the children in order — and varint(length)."""
    n_entries, p = _varint(blob, 1)  # blob[0]: canonical
    out = []
    for _ in range(n_entries):
        prefix, p = _varint(blob, p)
        kind, p = _varint(blob, p)
        if kind == VEC:
            n, p = _varint(blob, p)
            p += n * (1 + nbytes)
            out.append((prefix, VEC, n, n))
            continue
        nodes, pending = 0, 1
        while pending:  # pre-order: every node announces its children
            c, p = _varint(blob, p)
            p += c
            kids, p = _varint(blob, p)
            nodes += 1
            pending += kids - 1
        length, p = _varint(blob, p)
        out.append((prefix, TRIE, length, nodes))
    assert p == len(blob), (p, len(blob))
    return out


# ---- `cbl repartition` --------------------------------------------------------------------------------------------------
def _f1(x: float) -> str:
    """Rust's {:.1} of an f64."""
    if x != x:
        return "NaN"
    if x in (float("inf"), float("-inf")):
        return "inf" if x > 0 else "-inf"
    return f"{x:.1f}"


def _div(a: int, b: int) -> float:
    """`a as f64 / b as f64`."""
    if b == 0:
        return float("nan") if a == 0 else float("inf")
    return a / b


def repartition_report(prefix_bits: int, table):
    """(stderr lines, stdout line) of `repartition` for a bucket table [(prefix, length, kind, nodes)] in ascending prefix order.
    An empty table gives the load line alone (the reference panics there) and a stdout line of zeros."""
    load = len(table) / float(1 << prefix_bits)
    lines = [f"{_f1(load * 100.0)}% of the available prefixes are used"]
    if not table:
        return lines, f"{load} 0 0 0 0 0 0 0 0 0"
    size_count = sorted(Counter(length for _, length, _, _ in table).items())
    total_buckets = sum(c for _, c in size_count)
    total_items = sum(s * c for s, c in size_count)
    lines.append(f"The average bucket size is {_f1(_div(total_items, total_buckets))} items")
    bucket_count = item_count = 0
    for size, count in size_count:
        bucket_count += count
        item_count += size * count
        if count > total_buckets // 100 // 2 or size * count > total_items // 100 // 2 or bucket_count == total_buckets:
            lines.append(f"{_f1(_div(item_count * 100, total_items))}% of items are in a bucket of size ≤ {size} "
                         f"({_f1(_div(bucket_count * 100, total_buckets))}% of buckets)")
    max_prefix, max_size = 0, -1
    for prefix, length, _, _ in table:  # Iterator::max_by_key keeps the LAST of equal maxima
        if length >= max_size:
            max_prefix, max_size = prefix, length
    lines.append(f"The biggest bucket (of size {max_size}) corresponds to prefix {max_prefix}")
    vec_count = vec_nodes = trie_count = trie_nodes_ = 0
    for nodes, count in sorted(Counter(nd for _, _, _, nd in table).items()):
        if nodes <= REPARTITION_VEC_MAX_NODES:
            vec_count += count
            vec_nodes += nodes * count
        else:
            trie_count += count
            trie_nodes_ += nodes * count
    lines.append(f"{vec_count} vecs, average node count = {_f1(_div(vec_nodes, vec_count))}")
    lines.append(f"{trie_count} tries, average node count = {_f1(_div(trie_nodes_, trie_count))}")
    total = total_buckets + vec_nodes + trie_nodes_
    lines.append(f"{total} nodes in total")
    return lines, f"{load} {total_buckets} {total_items} {max_prefix} {max_size} {vec_count} {vec_nodes} {trie_count} {trie_nodes_} {total}"
