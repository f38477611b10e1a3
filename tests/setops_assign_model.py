"""The reference's ASSIGNING forms `a &= &mut b`, `a -= &mut b`, `a ^= &mut b` restated on `oracle.pyref.PyCBL.buckets` (prefix -> [kind, items]) — a
helper, not a test file. It mutates both operands and follows the Rust line by line, so that the two can be read side by side:
  * src/wordset/set_ops.rs:192-239 (`&=`), 281-317 (`-=`), 366-410 (`^=`): the walk over the two prefix sets. Container ids, the tiered vector and
    `empty_containers` never reach the file (oracle/pyref.py::serialize), so `del buckets[p]` stands for all three;
  * src/trievec/set_ops.rs:101-129, 163-187, 226-257: `iter_sorted` on both sides — `list.sort()` on a Vec, a Trie iterates ascending — then the
    two-pointer loop that collects deletions (and, for `^=`, insertions);
  * src/trievec/mod.rs:118-136 `insert_sorted_iter` and 146-168 `remove_sorted_iter`: on a Vec, pushes at the end and `swap_remove` on the ascending
    indices in reverse; on a Trie, `insert` / `remove` one by one — a Trie is kept here as a sorted list, which is what the file stores
    (src/trie.rs:133-162: `remove` prunes empty nodes, so the trie is a function of its set).
Also here: `swap_remove_closed_form`, the layout without the replay, and `fixup_by_doubling`, the restatement `k_bucket_setop_assign` computes."""
import bisect

from oracle.pyref import PyCBL

OPS = ("and", "sub", "xor")


# ---------------------------------------------------------------- src/trievec/mod.rs
def insert_sorted_iter(bucket, it):
    kind, items = bucket
    if kind == "vec":  # :120-131
        stop = len(items)
        i = 0
        for x in it:
            while i < stop and x > items[i]:
                i += 1
            if i == stop or x < items[i]:
                items.append(x)
    else:  # :132-134 insert_iter -> Trie::insert
        for x in it:
            k = bisect.bisect_left(items, x)
            if k == len(items) or items[k] != x:
                items.insert(k, x)


def remove_sorted_iter(bucket, it):
    kind, items = bucket
    if kind == "vec":  # :148-163
        stop = len(items)
        i = 0
        deletions = []
        for x in it:
            while i < stop and x > items[i]:
                i += 1
            if i < stop and x == items[i]:
                deletions.append(i)
        for i in reversed(deletions):  # Vec::swap_remove
            items[i] = items[-1]
            items.pop()
    else:  # :164-166 remove_iter -> Trie::remove
        for x in it:
            k = bisect.bisect_left(items, x)
            if k < len(items) and items[k] == x:
                items.pop(k)


def iter_sorted(bucket):  # :209-220
    if bucket[0] == "vec":
        bucket[1].sort()
    return list(bucket[1])


# ---------------------------------------------------------------- src/trievec/set_ops.rs
def bitand_assign(self, other):  # :101-129
    A, B = iter_sorted(self), iter_sorted(other)
    i = j = 0
    deletions = []
    while i < len(A) and j < len(B):
        if A[i] < B[j]:
            deletions.append(A[i])
            i += 1
        elif A[i] > B[j]:
            j += 1
        else:
            i += 1
            j += 1
    while i < len(A):
        deletions.append(A[i])
        i += 1
    remove_sorted_iter(self, deletions)


def sub_assign(self, other):  # :163-187
    A, B = iter_sorted(self), iter_sorted(other)
    i = j = 0
    deletions = []
    while i < len(A) and j < len(B):
        if A[i] < B[j]:
            i += 1
        elif A[i] > B[j]:
            j += 1
        else:
            deletions.append(A[i])
            i += 1
            j += 1
    remove_sorted_iter(self, deletions)


def bitxor_assign(self, other):  # :226-257
    A, B = iter_sorted(self), iter_sorted(other)
    i = j = 0
    insertions, deletions = [], []
    while i < len(A) and j < len(B):
        if A[i] < B[j]:
            i += 1
        elif A[i] > B[j]:
            insertions.append(B[j])
            j += 1
        else:
            deletions.append(A[i])
            i += 1
            j += 1
    while j < len(B):
        insertions.append(B[j])
        j += 1
    insert_sorted_iter(self, insertions)
    remove_sorted_iter(self, deletions)


_BUCKET_OP = {"and": bitand_assign, "sub": sub_assign, "xor": bitxor_assign}


# ---------------------------------------------------------------- src/wordset/set_ops.rs
def set_op_assign(a: PyCBL, b: PyCBL, op: str) -> PyCBL:
    """`a OP= &mut b`; returns a"""
    assert op in OPS
    assert a.canonical == b.canonical, "One of the index is canonical while the other isn't"  # src/cbl.rs:483-486, 523-526, 563-566
    assert (a.P["K"], a.P["PB"]) == (b.P["K"], b.P["PB"])
    prefixes = sorted(a.buckets)  # self.prefixes.iter(): taken before the walk
    k = 0
    for other_prefix in sorted(b.buckets):
        while k < len(prefixes) and prefixes[k] < other_prefix:
            if op == "and":  # :203-210 remove container
                del a.buckets[prefixes[k]]
            k += 1  # (`-=`, `^=`: keep container)
        if k < len(prefixes) and prefixes[k] == other_prefix:
            p = prefixes[k]
            _BUCKET_OP[op](a.buckets[p], b.buckets[other_prefix])
            if not a.buckets[p][1]:  # is_empty(): the prefix leaves the bitvector
                del a.buckets[p]
            k += 1
        elif op == "xor":  # :395-403 insert container
            a.buckets[other_prefix] = [b.buckets[other_prefix][0], list(b.buckets[other_prefix][1])]
    if op == "and":
        while k < len(prefixes):  # :226-233 remove container
            del a.buckets[prefixes[k]]
            k += 1
    return a


# ---------------------------------------------------------------- the Vec layout without the replay
def replay(v, D):
    """remove_sorted_iter's second loop, literally: D ascending indices into v"""
    v = list(v)
    for i in reversed(D):
        v[i] = v[-1]
        v.pop()
    return v


def swap_remove_closed_form(v, D):
    """r[i] = v[i] outside D; a hole h < L takes v[s], s = n - ge(h), and while s is in D, s = n - ge(s)"""
    n, m = len(v), len(D)
    L = n - m
    inD = set(D)
    ge = lambda p: m - bisect.bisect_left(D, p)
    r = []
    for i in range(L):
        s = i
        if i in inD:
            s = n - ge(i)
            while s in inD:
                s = n - ge(s)
        r.append(v[s])
    return r


def fixup_by_doubling(v, D, cs):
    """What k_bucket_setop_assign computes (cbl_amd/csrc/kernels_setops.hpp): v = sorted a (cs words) ++ pushed words, D inside [0, cs).
    dl[p] = deleted indices below p (dl[cs] = m); next[] over the tail [L, cs) — beyond cs nothing is deleted — doubled until nothing moves;
    r[i] = v[i] or v[next*(L + dl[i])]. -> (r, rounds of doubling)"""
    n, m = len(v), len(D)
    assert all(d < cs for d in D) and cs <= n
    L = n - m
    inD = set(D)
    dl = [0] * (cs + 1)
    for p in range(cs):
        dl[p + 1] = dl[p] + (p in inD)
    rounds = 0
    cur = []
    if L < cs:
        cur = [L + dl[p] if dl[p + 1] != dl[p] else p for p in range(L, cs)]
        while True:
            nxt = [cur[x - L] if x < cs else x for x in cur]
            moved = nxt != cur
            cur = nxt
            rounds += 1
            if not moved:
                break
    r = []
    for i in range(min(L, cs)):
        s = i
        if dl[i + 1] != dl[i]:
            s = L + dl[i]
            if s < cs:
                s = cur[s - L]
        r.append(v[s])
    return r + list(v[cs:L]), rounds


def named_shapes(n):
    """the named deletion sets for a Vec of n words: name -> ascending indices"""
    half = n // 2
    shapes = {
        "nothing": [],
        "everything": list(range(n)),
        "run_at_the_end": list(range(n - max(1, n // 3), n)),
        "run_ending_at_n_minus_2": list(range(1 if n > 3 else 0, n - 1)),  # one chain of about n - 2 hops
        "alternating": list(range(0, n, 2)),
        "alternating_odd": list(range(1, n, 2)),
    }
    # with m = half deletions L = n - half: only inside [L, n), only below L
    shapes["only_in_tail"] = list(range(n - half, n))
    shapes["only_below_L"] = list(range(0, half))
    return {k: [d for d in D if 0 <= d < n] for k, D in shapes.items()}
