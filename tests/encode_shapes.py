"""Crafted batches of reads for the encode stage (KRN-1: cbl_amd/csrc/kernels_encode.hpp; plan_chunks and encode in pipeline.hpp): reads whose
chunks, tiles, K-mer widths and invalid bytes sit exactly on the limits k_encode and k_encode_dirty_wave are built around. Pure CPU: `random`
and `oracle.pyref`; a helper, not a test file. tests/test_encode_shapes.py proves from the model below that every batch lands on its edge and
that the C++ oracle's words equal pyref's; tests/test_gpu_encode_edges.py compares the GPU's words, in order, and index bytes with them.

What this file restates from the kernels (`geometry`), from (read lengths, lead, K) and the bytes alone:
  * plan_chunks: everything is relative to bias = offsets[0] & ~15, the 16-byte aligned position below the first read (lead = offsets[0]);
  * k_seq_chunk_count / k_chunk_fill: a read of nk = len - K + 1 k-mers has ceil(nk / 2048) chunks, chunk j starts 2048 j bases into the read, is
    min(2048 + K - 1, len - 2048 j) bytes long and holds length - K + 1 k-mers; consecutive chunks of a read share K - 1 bytes;
  * k_scan_invalid / mark_dirty and k_dirty_count_wave: a chunk with a byte outside ACGTacgt is dirty and holds 1 + (valid bytes of chunk[K:])
    k-mers, the K-windows of zeros(K - n0) ++ its valid bases, n0 = valid bytes among the first K;
  * k_tile_first_chunk: tile t of 4096 bytes owns the chunks that START in [4096 t, 4096 (t + 1)); a tile may own none;
  * k_encode, per tile: A0 = first chunk start & ~15, the bytes it spans up to the end of its last chunk, the packed dwords it loads, its k-mers Q,
    the in-tile uniform test (every chunk clean, nk0 k-mers, len0 bytes after its predecessor) with the loop's dci = 256 / nk0 and
    dj = 256 - dci nk0, its first output slot modulo 4096 and the windows of the fused histogram its clean outputs touch;
  * uniform_plan.hpp: the plan is arithmetic for reads of one length L, K <= L <= K + 2047, without an invalid byte.
`lds_bounds` lists every LDS capacity of the two kernels with the largest index the batch reaches.

Expected words are `oracle.pyref.seq_words` of every read, concatenated (reference_words), computed once per process and read, and shared by the
batches that repeat a read. Reads are random ACGT from a generator seeded by the batch's name unless the batch says otherwise.
"""
from __future__ import annotations

import random
from collections import namedtuple

import numpy as np

from oracle import pyref

CHUNK_KMERS = 2048                                        # common.hpp:30 CHUNK_KMERS
ENC_TILE_BYTES = 4096                                     # kernels_encode.hpp:93
ENC_THREADS = 256                                         # kernels_encode.hpp:94
ENC_MAX_CHUNKS = 1024                                     # kernels_encode.hpp:95: s_koff, s_cstart, s_cfwd
ENC_MAX_BASES = ENC_TILE_BYTES + CHUNK_KMERS + 64 + 32    # kernels_encode.hpp:96
ENC_CODE_WORDS = (ENC_MAX_BASES + 15) // 16 + 8           # kernels_encode.hpp:97: s_codes
ENC_MAX_KMERS = ENC_MAX_BASES                             # kernels_encode.hpp:98
ENC_HIST_WINDOW = 4096                                    # kernels_encode.hpp:101
ENC_HIST_WINDOWS = ENC_MAX_KMERS // ENC_HIST_WINDOW + 2   # kernels_encode.hpp:102: s_hist rows of 256
ENC_READ_AHEAD = 6                                        # kernels_encode.hpp:446: dwords zeroed behind the tile's packed stream
ENC_PAR_WORDS = (ENC_MAX_KMERS + ENC_THREADS) // 64 + 2   # kernels_encode.hpp:392-393: s_par, s_parpre
DIRTY_MAX_BASES = CHUNK_KMERS + 64 + 64                   # kernels_encode.hpp:594
DIRTY_CB_BYTES = DIRTY_MAX_BASES + 16                     # kernels_encode.hpp:601: s_cb_all
DIRTY_CODE_WORDS = DIRTY_MAX_BASES // 16 + 8              # kernels_encode.hpp:600: CW
DIRTY_PAR_WORDS = DIRTY_MAX_BASES // 64 + 2               # kernels_encode.hpp:600: PW
DIRTY_HIST_WINDOWS = 2                                    # kernels_encode.hpp:604: s_hist_all
DIRTY_WAVES = 4                                           # kernels_encode.hpp:600: NWV, dirty chunks per workgroup
DIRTY_LIST_THREADS = 256                                  # kernels_encode.hpp:278: chunks per k_dirty_list workgroup
VALID = frozenset(b"ACGTacgt")                            # common.hpp: nuc_valid

ALL_K = tuple(range(5, 60, 2))                            # the legal K: odd, 5 .. 59


def prefix_bits(k):
    """PREFIX_BITS of every case: 24, or 8 where the word (2 K + POS_BITS: 14, 18 and 23 bits at K = 5, 7, 9) is no longer than that"""
    return 8 if k <= 9 else 24


def is_wide(k):
    """ctx.hpp: dispatch. K >= 33: the k-mer takes 128 bits and extract_kmer reads 5 dwords instead of 3"""
    return 2 * k > 64


# ---- the geometry of a batch, restated ---------------------------------------------------------------------------------------------------------
Chunk = namedtuple("Chunk", "read j start length nk dirty koff")  # start: relative to bias; koff: first output slot of the chunk in the batch
Tile = namedtuple("Tile", "t c0 c1 nc A0 span nwords Q kbase uniform nk0 len0 dci dj hbase windows last_word")
Geometry = namedtuple("Geometry", "K lead bias total offsets chunks tiles n_kmers arithmetic")


def geometry(reads, lead, K):
    offsets = [lead]
    for r in reads:
        assert len(r) >= K
        offsets.append(offsets[-1] + len(r))
    bias = lead & ~15
    chunks, koff = [], 0
    for ri, r in enumerate(reads):
        nk_read = len(r) - K + 1
        for j in range((nk_read + CHUNK_KMERS - 1) // CHUNK_KMERS):            # k_seq_chunk_count
            a = j * CHUNK_KMERS
            b = min(a + CHUNK_KMERS + K - 1, len(r))                          # k_chunk_fill
            body = r[a:b]
            dirty = any(c not in VALID for c in body)                         # k_scan_invalid
            nk = 1 + sum(c in VALID for c in body[K:]) if dirty else b - a - K + 1  # k_dirty_count_wave
            chunks.append(Chunk(ri, j, offsets[ri] + a - bias, b - a, nk, dirty, koff))
            koff += nk
    total = offsets[-1] - bias
    ntiles = (total + ENC_TILE_BYTES - 1) // ENC_TILE_BYTES
    starts = [c.start for c in chunks]
    first = [int(np.searchsorted(starts, t * ENC_TILE_BYTES, side="left")) for t in range(ntiles + 1)]  # k_tile_first_chunk
    tiles = []
    for t in range(ntiles):
        c0, c1 = first[t], first[t + 1]
        if c0 == c1:  # no chunk starts here: the workgroup leaves at once (kernels_encode.hpp:423)
            tiles.append(Tile(t, c0, c1, 0, None, 0, 0, 0, None, False, 0, 0, 0, 0, None, (), None))
            continue
        cs = chunks[c0:c1]
        B0, B1 = cs[0].start, cs[-1].start + cs[-1].length
        A0 = B0 & ~15
        kbase = cs[0].koff
        Q = cs[-1].koff + cs[-1].nk - kbase
        nk0, len0 = cs[0].nk, (cs[1].start - cs[0].start if len(cs) > 1 else 0)
        uniform = all(not c.dirty and c.koff - kbase == i * nk0 and c.nk == nk0 and c.start == B0 + i * len0 for i, c in enumerate(cs))  # :465-469
        dci = ENC_THREADS // nk0
        hbase = kbase % ENC_HIST_WINDOW                                      # :519, out_base = 0 (pipeline.hpp: insert_device_one)
        windows = sorted({(hbase + c.koff - kbase + d) // ENC_HIST_WINDOW for c in cs if not c.dirty for d in (0, c.nk - 1)})
        clean = [c for c in cs if not c.dirty]
        last_word = max(((c.start - A0 + c.nk - 1) >> 4) + (4 if is_wide(K) else 2) for c in clean) if clean else None  # extract_kmer, :351-362
        tiles.append(Tile(t, c0, c1, c1 - c0, A0, B1 - A0, (B1 - A0 + 15) >> 4, Q, kbase, uniform, nk0, len0, dci, ENC_THREADS - dci * nk0, hbase,
                          tuple(windows), last_word))
    L = len(reads[0])
    arithmetic = all(len(r) == L for r in reads) and L - K + 1 <= CHUNK_KMERS and not any(c.dirty for c in chunks)  # uniform_plan.hpp:30, k_uniform_probe
    return Geometry(K, lead, bias, total, offsets, chunks, tiles, koff, arithmetic)


def lds_bounds(g):
    """{name: (largest value the batch reaches, capacity)}; every value must stay at or below its capacity"""
    live = [t for t in g.tiles if t.nc]
    qpad = [(t.Q + ENC_THREADS - 1) // ENC_THREADS * ENC_THREADS for t in live]
    out = {
        "chunks of a tile (s_koff, s_cstart, s_cfwd)": (max(t.nc for t in live), ENC_MAX_CHUNKS),
        "bytes a tile spans": (max(t.span for t in live), ENC_MAX_BASES),
        "packed dwords with the read-ahead (s_codes)": (max(t.nwords + ENC_READ_AHEAD for t in live), ENC_CODE_WORDS),
        "k-mers of a tile": (max(t.Q for t in live), ENC_MAX_KMERS),
        "strand words (s_par, s_parpre)": (max(q // 64 + 1 for q in qpad), ENC_PAR_WORDS),
        "histogram windows (s_hist)": (max((t.windows[-1] + 1 for t in live if t.windows), default=0), ENC_HIST_WINDOWS),
    }
    # the highest dword a k-mer reads must have been written: below the packed stream's zeroed read-ahead
    out["last dword a k-mer reads"] = (max((t.last_word - (t.nwords + ENC_READ_AHEAD - 1) for t in live if t.last_word is not None), default=-1), 0)
    dirty = [c for c in g.chunks if c.dirty]
    if dirty:  # k_encode_dirty_wave: the cleaned string is K - 1 + nk bases long
        fill = max(g.K - 1 + c.nk for c in dirty)
        out["cleaned bases of a dirty chunk (s_cb)"] = (fill, DIRTY_CB_BYTES)
        out["packed dwords of a dirty chunk"] = ((fill + 15) // 16 + ENC_READ_AHEAD, DIRTY_CODE_WORDS)
        out["strand words of a dirty chunk"] = (max((c.nk + 63) // 64 for c in dirty), DIRTY_PAR_WORDS)
        out["histogram windows of a dirty chunk"] = (max((c.koff % ENC_HIST_WINDOW + c.nk - 1) // ENC_HIST_WINDOW + 1 for c in dirty), DIRTY_HIST_WINDOWS)
    return out


def uniform_walk(nk0, Q, strict_wrap=False):
    """(chunk, position) of every k-mer of an in-tile uniform tile as k_encode's loop carries them from trip to trip (:547-554); strict_wrap: the
    wrap test written `>` instead of `>=`, a mistake every nk0 that does not divide 256 shows 256 k-mers into the tile and no divisor can"""
    dci = ENC_THREADS // nk0
    dj = ENC_THREADS - dci * nk0
    out = [None] * Q
    for tid in range(min(ENC_THREADS, Q)):
        ci = tid // nk0
        j = tid - ci * nk0
        for q in range(tid, Q, ENC_THREADS):
            out[q] = (ci, j)
            j += dj
            ci += dci
            if (j > nk0) if strict_wrap else (j >= nk0):
                j -= nk0
                ci += 1
    return out


def locate(g, slot):
    """where output slot `slot` of the batch comes from: for a failure message"""
    c = max((c for c in g.chunks if c.koff <= slot), key=lambda c: c.koff)
    t = c.start // ENC_TILE_BYTES
    return "read %d (%d bases), chunk %d of it (%s, %d k-mers, first byte %d of tile %d), slot %d of the chunk's %s" % (
        c.read, g.offsets[c.read + 1] - g.offsets[c.read], c.j, "dirty" if c.dirty else "clean", c.nk, c.start % ENC_TILE_BYTES, t, slot - c.koff,
        "outputs (forward-strand words first in canonical mode)")


# ---- reads ---------------------------------------------------------------------------------------------------------------------------------------
def _rng(*key):
    return random.Random("encode " + "/".join(str(k) for k in key))


def _rand(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def _with(read, at, byte):
    b = bytearray(read)
    for a in (at if isinstance(at, (list, tuple, range)) else (at,)):
        b[a] = byte
    return bytes(b)


# ---- 1. LDS capacities ---------------------------------------------------------------------------------------------------------------------------
FULLEST_K = (5, 31, 59)


def fullest_tile(K):
    """Reads of 4096, 4095 and 2048 + K - 1 bases. Tile 1 owns both chunks of the second read (2048 and 2048 - K k-mers, the first at its byte 0)
    and the one full chunk of the third, which starts at its byte 4095: 6144 - K k-mers over 4095 + 2048 + K - 1 bytes, the most the chunk rules
    allow. Its first output slot is 4096 - (K - 1), so its outputs touch three histogram windows."""
    rng = _rng("fullest", K)
    return [_rand(rng, n) for n in (4096, 4095, CHUNK_KMERS + K - 1)], 0


MOST_CHUNKS_LENGTHS = (5, 7, 8, 9)
MOST_CHUNKS_READS = 900


def most_chunks(L):
    """K = 5: 900 reads of L bases. L = 5: one k-mer per chunk, and tile 0 owns the chunks that start at bytes 0, 5, .. 4095: ceil(4096 / 5) = 820,
    the most a tile can own. L = 7, 8, 9: nk0 = 3, 4, 5."""
    rng = _rng("most_chunks", L)
    return [_rand(rng, L) for _ in range(MOST_CHUNKS_READS)], 0


# ---- 2. the in-tile uniform loop -----------------------------------------------------------------------------------------------------------------
UNIFORM_K = (21, 31, 59)
UNIFORM_NK0 = (1, 2, 3, 127, 128, 129, 255, 256, 257, 511, 2047, 2048)
_uniform = {}


def _uniform_reads(K, nk0):
    if (K, nk0) not in _uniform:
        L = nk0 + K - 1
        rng = _rng("uniform", K, nk0)
        reads = [_rand(rng, L) for _ in range(max(3, -(-3 * ENC_TILE_BYTES // L)))]
        extra = _rand(rng, 1)
        while True:  # as many reads as it takes for the longer twin's last read to share a tile with a chunk of another size
            twin = reads[:-1] + [reads[-1] + extra]
            g = geometry(twin, 0, K)
            if any(not g.tiles[c.start // ENC_TILE_BYTES].uniform for c in g.chunks if c.read == len(twin) - 1):
                break
            reads.append(_rand(rng, L))
        _uniform[K, nk0] = (reads, twin)
    return _uniform[K, nk0]


def uniform_nk0(K, nk0, twin=False):
    """Reads of nk0 + K - 1 bases over at least three tiles: every tile is in-tile uniform and the plan arithmetic. twin: the last read one base
    longer, which takes the batch to the chunk tables and its last tile to the loop that reads them."""
    return _uniform_reads(K, nk0)[1 if twin else 0], 0


# ---- 3. chunk seams and tile phases --------------------------------------------------------------------------------------------------------------
SEAM_K = (5, 29, 31, 33, 59)
SEAM_KMERS = (1, 2, 2047, 2048, 2049, 4095, 4096, 4097, 6145)
SEAM_ORDERS = ("plain", "reversed", "tail")


def chunk_seams(K, order):
    """One read each of 1, 2, 2047, 2048, 2049, 4095, 4096, 4097 and 6145 k-mers (last chunks of 1, 2047 and 2048 k-mers; chunks of exactly K
    bytes) in this order, in reverse order (other tile phases), or with the read of 4095 k-mers moved to the end ("tail": the stream's last tile
    holds the end of its second chunk and no chunk start; 6145 k-mers end in a chunk of K bytes, which never leaves such a tile behind)."""
    rng = _rng("seams", K)
    reads = [_rand(rng, nk + K - 1) for nk in SEAM_KMERS]
    if order == "tail":
        reads.append(reads.pop(SEAM_KMERS.index(4095)))
    return (reads[::-1] if order == "reversed" else reads), 0


PHASE_AT = (4094, 4095, 4096, 4097)
PHASE_LEADS = (0, 1, 8, 15)


def tile_phase(lead, at):
    """K = 31: a read that ends where a read of one full chunk starts, at byte `at` of the stream; offsets[0] = lead bytes past a 16-byte boundary"""
    K = 31
    p = at - lead
    return [_rand(_rng("phase first", p), p), _rand(_rng("phase second"), CHUNK_KMERS + K - 1)], lead


# ---- 4. invalid bytes ----------------------------------------------------------------------------------------------------------------------------
DIRTY_K = (5, 31, 33, 59)
DIRTY_READ_KMERS = 2 * CHUNK_KMERS + 7


def dirty_positions_at(K):
    L = DIRTY_READ_KMERS + K - 1
    return (0, K - 1, K, 63, 64, 2047, 2048, 2048 + K - 2, 2048 + K - 1, 2048 + K, 4096, L - 1)


def dirty_overlap(K, at):
    """whether byte `at` of a read lies in two chunks"""
    return at >= CHUNK_KMERS and at % CHUNK_KMERS <= K - 2


DIRTY_SHORT = tuple((n, at) for n in (63, 64, 65, 127, 128, 129) for at in (62, 63, 64) if at < n)


def dirty_positions(K):
    """Reads 0 .. 11: three chunks (2 * 2048 + 7 k-mers) with one N at byte 0, K - 1, K, 63, 64, 2047, 2048, 2048 + K - 2, 2048 + K - 1, 2048 + K,
    4096, the last. Read 12: its first K bytes N. Read 13: only N (one word, the zero k-mer). Read 14: K - 1 valid bytes spread over 2 K.
    Reads 15 ..: 63, 64, 65, 127, 128, 129 bytes with an `n` at byte 62, 63 or 64 (the dirty kernel's 64-byte steps)."""
    rng = _rng("dirty", K)
    L = DIRTY_READ_KMERS + K - 1
    reads = [_with(_rand(rng, L), at, ord("N")) for at in dirty_positions_at(K)]
    reads.append(b"N" * K + _rand(rng, 40))
    reads.append(b"N" * (K + 3))
    reads.append(bytes(rng.choice(b"ACGT") if i % 2 == 1 and i < 2 * K - 1 else ord("N") for i in range(2 * K)))  # valid at 1, 3, .. 2 K - 3
    reads += [_with(_rand(rng, n), at, ord("n")) for n, at in DIRTY_SHORT]
    return reads, 0


AMONG_DIRTY_READS = (0, 1, 26, 27, 28, 40, 41, 42, 43, 44)


def dirty_among_clean(variant):
    """K = 31, reads of 150 bases (a tile holds 27.3). "few": 60 reads, those at 0, 1, 26, 27, 28 and 40 .. 44 with an N: 10 dirty chunks, so the
    third workgroup of the dirty kernel has two idle waves. "alternating": 600 reads, every second one with an N: the dirty chunks of three
    k_dirty_list workgroups."""
    rng = _rng("among", variant)
    n, dirty = (60, AMONG_DIRTY_READS) if variant == "few" else (600, tuple(range(1, 600, 2)))
    reads = [_rand(rng, 150) for _ in range(n)]
    for i in dirty:
        reads[i] = _with(reads[i], rng.randrange(150), ord("N"))
    return reads, 0


# ---- 5. the necklace on the device ---------------------------------------------------------------------------------------------------------------
NECKLACE_RUNS = (1, 2, 5, 6)  # and K - 1
NECKLACE_RANDOM = 200
NECKLACE_INDEX_K = (27, 31, 33, 59)


def necklace_families(K):
    """Reads of exactly K bases, one k-mer each, the word families of tests/host/necklace_fused_unit.cpp as k-mers: one run of 1, 2, 5, 6 or K - 1
    A (2 r zero bits, 2 r + 1 beside a C or a T: either side of the L = 11 step) at every offset of the ring, wrapping ones included, among C, G or T;
    poly-A / C / G / T; every repeat of period 2 and 3 at every phase; A^(K-1) C at every rotation; 200 random k-mers. Repeats of a read are dropped."""
    rng = _rng("necklace", K)
    reads = []
    for r in NECKLACE_RUNS + (K - 1,):
        if r >= K:
            continue
        for bg in b"CGT":
            for o in range(K):
                reads.append(_with(bytes([bg]) * K, [(o + i) % K for i in range(r)], ord("A")))
    reads += [bytes([b]) * K for b in b"ACGT"]
    for period in (2, 3):
        for unit in range(4 ** period):
            u = bytes(b"ACGT"[(unit >> (2 * i)) & 3] for i in range(period))
            reads += [(u * (K // period + 2))[ph:ph + K] for ph in range(period)]
    reads += [_with(b"A" * K, o, ord("C")) for o in range(K)]
    reads += [_rand(rng, K) for _ in range(NECKLACE_RANDOM)]
    return list(dict.fromkeys(reads)), 0


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------------
BATCHES = {"fullest_tile": fullest_tile, "most_chunks": most_chunks, "uniform_nk0": uniform_nk0, "chunk_seams": chunk_seams, "tile_phase": tile_phase,
           "dirty_positions": dirty_positions, "dirty_among_clean": dirty_among_clean, "necklace_families": necklace_families}


def _k_of(name, args):
    return {"most_chunks": 5, "tile_phase": 31, "dirty_among_clean": 31}.get(name) or args[0]


CASES = ([("fullest_tile", (k,)) for k in FULLEST_K] + [("most_chunks", (L,)) for L in MOST_CHUNKS_LENGTHS]
         + [("uniform_nk0", (k, n, twin)) for k in UNIFORM_K for n in UNIFORM_NK0 for twin in (False, True)]
         + [("chunk_seams", (k, order)) for k in SEAM_K for order in SEAM_ORDERS]
         + [("tile_phase", (lead, at)) for lead in PHASE_LEADS for at in PHASE_AT]
         + [("dirty_positions", (k,)) for k in DIRTY_K] + [("dirty_among_clean", (v,)) for v in ("few", "alternating")])
NECKLACE_CASES = [("necklace_families", (k,)) for k in ALL_K]


def case_id(case):
    name, args = case
    return name + "-" + "-".join(("twin" if a else "plain") if isinstance(a, bool) else str(a) for a in args)


Batch = namedtuple("Batch", "name args K pb reads lead bases offsets geometry")
_cache, _read_words = {}, {}


def batch(case):
    """the batch of a case with its arrays (bases: `lead` bytes of N, then the reads back to back; offsets[0] = lead) and geometry: computed once per
    process and left unchanged by its users"""
    if case not in _cache:
        name, args = case
        reads, lead = BATCHES[name](*args)
        K = _k_of(name, args)
        bases = np.frombuffer(b"N" * lead + b"".join(reads), dtype=np.uint8)
        offsets = (np.concatenate([[0], np.cumsum([len(r) for r in reads])]) + lead).astype(np.uint64)
        _cache[case] = Batch(name, args, K, prefix_bits(K), tuple(reads), lead, bases, offsets, geometry(reads, lead, K))
    return _cache[case]


def reference_words(b, canonical):
    """pyref.seq_words of every read of the batch, concatenated: Python integers (one list per (K, strand mode, read), shared between batches)"""
    P = pyref.params(b.K, b.pb)
    out = []
    for r in b.reads:
        key = (b.K, canonical, r)
        if key not in _read_words:
            _read_words[key] = pyref.seq_words(r, P, canonical)
        out += _read_words[key]
    return out


def warm_reference(cases, processes):
    """reference_words of the cases in both strand modes, every distinct read once, spread over worker processes (for a process that has not
    touched a GPU: the workers are forks)"""
    import multiprocessing as mp

    keys = list(dict.fromkeys((batch(c).K, canonical, r) for c in cases for canonical in (False, True) for r in batch(c).reads))
    keys = [k for k in keys if k not in _read_words]
    keys.sort(key=lambda k: -len(k[2]))
    if processes <= 1 or not keys:
        return
    with mp.get_context("fork").Pool(processes) as pool:
        for key, words in zip(keys, pool.map(_words_of, keys, chunksize=4)):
            _read_words[key] = words


def _words_of(key):
    k, canonical, read = key
    return pyref.seq_words(read, pyref.params(k, prefix_bits(k)), canonical)


def words_as_arrays(words):
    """(lo, hi) uint64 arrays of a list of words"""
    lo = np.array([w & 0xFFFFFFFFFFFFFFFF for w in words], dtype=np.uint64)
    hi = np.array([w >> 64 for w in words], dtype=np.uint64)
    return lo, hi
