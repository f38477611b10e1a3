"""The reference's removal — `CBL::remove`, `CBL::remove_seq` — restated on `oracle.pyref.PyCBL.buckets` (prefix -> [kind, items]): a helper, not a test file.
The literal part follows the Rust line by line, so that the two can be read side by side:
  * src/trievec/mod.rs:91-108 `TrieVec::remove`: on a Vec the position of the first equal element and `swap_remove`; on a Trie — kept here as a sorted
    list, which is what the file stores (src/trie.rs:133-162: `remove` prunes empty nodes, so the trie is a function of its set) — a deletion;
  * src/wordset/mod.rs:218-237 `remove_batch`: `chunk_by` on equal prefixes, `remove_iter`, the bucket deleted when it comes out empty, and
    `adapt_container_shrink` (:246-251) after the group: a Trie of <= THRESHOLD words becomes a Vec in ascending order (`as_vec`, src/trievec/mod.rs:180-188),
    a Vec stays a Vec. Container ids, the tiered vector and `empty_containers` never reach the file, so `del buckets[p]` stands for all three;
  * src/wordset/mod.rs:122-137 `remove`; src/cbl.rs:343-354 `remove_seq`: one `remove_batch` per chunk of `get_seq_words`.
The closed forms are what the device path computes (cbl_amd/csrc/kernels_remove.hpp): `groups_of` (the group number of every word of a call that holds
several batches), `effective_removals` (the first stream occurrence of each stored suffix), `replay_bucket` (deletions up to the end of the group that converts
a Trie, then swap_remove with position tracking) and `remove_batches_closed`, which puts them together for a whole call."""
import bisect

from oracle.pyref import CHUNK, THRESHOLD, PyCBL, chunk_words


# ---------------------------------------------------------------- the literal replay
def trievec_remove(bucket, x) -> bool:  # src/trievec/mod.rs:91-108
    kind, items = bucket
    if kind == "trie":  # :93-99 Trie::remove
        k = bisect.bisect_left(items, x)
        if k < len(items) and items[k] == x:
            items.pop(k)
            return True
        return False
    try:
        i = items.index(x)  # :101 vec.iter().position(|y| y == x)
    except ValueError:
        return False  # :105
    items[i] = items[-1]  # :102 Vec::swap_remove
    items.pop()
    return True


def adapt_container_shrink(bucket):  # src/wordset/mod.rs:246-251 -> as_vec, src/trievec/mod.rs:180-188
    if len(bucket[1]) <= THRESHOLD and bucket[0] == "trie":
        bucket[0] = "vec"  # trie.iter() is ascending: the sorted list is the Vec


def remove_batch(cbl: PyCBL, words):  # src/wordset/mod.rs:218-237
    sb = cbl.P["SB"]
    mask = (1 << sb) - 1
    i = 0
    while i < len(words):  # :223 chunk_by(|(p1, _), (p2, _)| p1 == p2)
        p = words[i] >> sb
        j = i
        while j < len(words) and (words[j] >> sb) == p:
            j += 1
        if p in cbl.buckets:  # :225
            b = cbl.buckets[p]
            for w in words[i:j]:  # :228 remove_iter
                trievec_remove(b, w & mask)
            if not b[1]:  # :229-233
                del cbl.buckets[p]
            adapt_container_shrink(b)  # :234 (on the emptied container too: nothing of it is stored)
        i = j


def remove_word(cbl: PyCBL, word) -> bool:  # src/wordset/mod.rs:122-137
    sb = cbl.P["SB"]
    p, s = word >> sb, word & ((1 << sb) - 1)
    present = p in cbl.buckets  # :124
    if present:
        b = cbl.buckets[p]
        present = trievec_remove(b, s)  # :128
        adapt_container_shrink(b)  # :129
        if not b[1]:  # :130-134
            del cbl.buckets[p]
    return present


def seq_batches(cbl: PyCBL, seq: bytes):
    """The word lists of the remove_batch calls of one remove_seq: one per chunk, fwd ++ rc in a canonical index."""
    k = cbl.P["K"]
    if len(seq) < k:  # src/cbl.rs:344-349
        raise ValueError("Sequence size (%d) is smaller than K (%d)" % (len(seq), k))
    return [chunk_words(seq[start : min(start + CHUNK + k - 1, len(seq))], cbl.P, cbl.canonical) for start in range(0, len(seq) - k + 1, CHUNK)]  # :350-351


def remove_seq(cbl: PyCBL, seq: bytes):  # src/cbl.rs:343-354
    for words in seq_batches(cbl, seq):
        remove_batch(cbl, words)  # :352


# ---------------------------------------------------------------- closed forms (what the kernels compute)
def groups_of(batches, sb):
    """(word, group number) for every word of the batches in stream order: a group starts at the first word of a batch and wherever the prefix changes."""
    out = []
    g = 0
    for words in batches:
        for i, w in enumerate(words):
            if i == 0 or (w >> sb) != (words[i - 1] >> sb):
                g += 1
            out.append((w, g))
    return out


def effective_removals(items, stream):
    """stream: [(ordinal, group, suffix)] aimed at one bucket, in stream order. Returns [(ordinal, group, stored position)] of the removals that change the
    bucket — the first occurrence of each suffix it holds — in stream order: nothing is inserted meanwhile, so a suffix once gone stays gone."""
    where = {s: t for t, s in enumerate(items)}
    first = {}
    for o, g, s in stream:
        t = where.get(s)
        if t is not None and t not in first:
            first[t] = (o, g)
    return sorted((o, g, t) for t, (o, g) in first.items())


def conversion_group(kind, length, eff, first_group):
    """The group at whose end a Trie becomes a Vec, or None (a Vec, or a Trie that stays longer than THRESHOLD)."""
    if kind != "trie":
        return None
    j0 = length - THRESHOLD
    if j0 <= 0:
        return first_group  # adapt_container_shrink runs after every group that finds the prefix, hit or no hit
    if len(eff) < j0:
        return None
    return eff[j0 - 1][1]


def replay_bucket(kind, items, stream):
    """(kind, items) after the removals of `stream` (see effective_removals), without replaying them one by one through the container."""
    if not stream:
        return kind, list(items)
    eff = effective_removals(items, stream)
    gc = conversion_group(kind, len(items), eff, min(g for _, g, _ in stream))
    if kind == "trie" and gc is None:
        n1 = len(eff)  # plain set difference, stays a Trie
    elif kind == "trie":
        n1 = sum(1 for _, g, _ in eff if g <= gc)  # deletions up to the end of the group that converts
    else:
        n1 = 0
    gone = {t for _, _, t in eff[:n1]}
    elem = [t for t in range(len(items)) if t not in gone]  # elem[p]: which stored word stands at p
    pos = {t: p for p, t in enumerate(elem)}  # pos[t]: where stored word t stands now
    for _, _, t in eff[n1:]:  # swap_remove in stream order, O(1) each
        p = pos[t]
        f = elem.pop()
        if p < len(elem):
            elem[p] = f
            pos[f] = p
    out_kind = "trie" if (kind == "trie" and gc is None) else "vec"
    return out_kind, [items[t] for t in elem]


def remove_batches_closed(cbl: PyCBL, batches):
    """All the remove_batch calls of one device call at once: per bucket, independent of the others. Returns the `was effective` flag of every word."""
    sb = cbl.P["SB"]
    mask = (1 << sb) - 1
    tagged = groups_of(batches, sb)
    per = {}
    for o, (w, g) in enumerate(tagged):
        if (w >> sb) in cbl.buckets:
            per.setdefault(w >> sb, []).append((o, g, w & mask))
    flags = [False] * len(tagged)
    for p, stream in per.items():
        kind, items = cbl.buckets[p]
        for o, _, _ in effective_removals(items, stream):
            flags[o] = True
        nk, ni = replay_bucket(kind, items, stream)
        if ni:
            cbl.buckets[p] = [nk, ni]
        else:
            del cbl.buckets[p]
    return flags


def copy_cbl(c: PyCBL) -> PyCBL:
    d = PyCBL(c.P["K"], c.P["PB"], c.canonical)
    d.buckets = {p: [b[0], list(b[1])] for p, b in c.buckets.items()}
    return d
