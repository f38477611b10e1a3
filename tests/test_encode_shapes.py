"""What the crafted batches of tests/encode_shapes.py deliver, on the CPU: (a) the constants the model restates are the ones kernels_encode.hpp
defines; (b) for every batch the C++ oracle's words equal oracle.pyref's, canonical and not, the model's chunk k-mer counts add up to them read by
read, and every LDS capacity of k_encode and k_encode_dirty_wave holds; (c) every batch lands on the edge it is named after: the fullest tile and
the most chunks of a tile reach their maxima exactly, the equal-length batches are in-tile uniform with the expected loop strides and their
longer twins are not, the seams, phases and invalid bytes sit where the docstrings say; (d) the carried (chunk, position) of the in-tile uniform
loop, restated, equals the division it replaces, and the loop with its wrap test written `>` goes wrong exactly where a lane lands on j = nk0."""
import os
import re
from pathlib import Path

import numpy as np
import pytest

import encode_shapes as es
from oracle import Oracle, pyref

SRC = (Path(__file__).resolve().parent.parent / "cbl_amd" / "csrc" / "kernels_encode.hpp").read_text()
ALL_CASES = es.CASES + es.NECKLACE_CASES


def _cases(name):
    return [c for c in ALL_CASES if c[0] == name]


def _param(cases):
    return pytest.mark.parametrize("case", cases, ids=[es.case_id(c) for c in cases])


@pytest.fixture(scope="module", autouse=True)
def _reference():
    """every read's pyref words, computed once for the module on the CPUs this process may use"""
    es.warm_reference(ALL_CASES, min(8, len(os.sched_getaffinity(0))))


def test_constants_are_the_kernels():
    for text in ("ENC_TILE_BYTES = 4096;", "ENC_THREADS = 256;", "ENC_MAX_CHUNKS = 1024;", "ENC_MAX_BASES = ENC_TILE_BYTES + CHUNK_KMERS + 64 + 32;",
                 "ENC_CODE_WORDS = (ENC_MAX_BASES + 15) / 16 + 8;", "ENC_MAX_KMERS = ENC_MAX_BASES;", "ENC_HIST_WINDOW = 4096;",
                 "ENC_HIST_WINDOWS = ENC_MAX_KMERS / ENC_HIST_WINDOW + 2;", "DIRTY_MAX_BASES = CHUNK_KMERS + 64 + 64;", "DIRTY_LIST_THREADS = 256;",
                 "NWV = 4, CW = DIRTY_MAX_BASES / 16 + 8, PW = DIRTY_MAX_BASES / 64 + 2;", "s_cb_all[NWV][DIRTY_MAX_BASES + 16]", "s_hist_all[NWV][2 * 256]",
                 "i < nwords + 6 && i < ENC_CODE_WORDS", "s_par[(ENC_MAX_KMERS + ENC_THREADS) / 64 + 2]", "s_parpre[(ENC_MAX_KMERS + ENC_THREADS) / 64 + 2]",
                 "const u32 dci = ENC_THREADS / nk0, dj = ENC_THREADS - dci * nk0", "if (j >= nk0) { j -= nk0; ++ci;"):
        assert text in SRC, text
    common = (Path(__file__).resolve().parent.parent / "cbl_amd" / "csrc" / "common.hpp").read_text()
    assert re.search(r"CHUNK_KMERS = 2048;", common)
    assert (es.ENC_MAX_BASES, es.ENC_CODE_WORDS, es.ENC_HIST_WINDOWS, es.ENC_PAR_WORDS) == (6240, 398, 3, 103)


def _oracle_words(o, reads):
    cap = sum(len(r) for r in reads) + 1
    lo, hi = np.zeros(cap, dtype=np.uint64), np.zeros(cap, dtype=np.uint64)
    at, per_read = 0, []
    for r in reads:
        n = o._L.oracle_seq_words(o._h, r, len(r), 0, lo[at:].ctypes.data, hi[at:].ctypes.data, cap - at)
        assert n >= 0
        per_read.append(n)
        at += n
    return lo[:at], hi[:at], per_read


@_param(ALL_CASES)
def test_oracle_is_pyref_and_the_model_counts_its_words(case):
    b = es.batch(case)
    g = b.geometry
    assert g.offsets == [int(x) for x in b.offsets] and g.offsets[0] == b.lead and g.bias == b.lead & ~15 and len(b.bases) == g.offsets[-1]
    assert bytes(b.bases[:b.lead]) == b"N" * b.lead
    per_read_model = [sum(c.nk for c in g.chunks if c.read == i) for i in range(len(b.reads))] if len(g.chunks) < 2000 else None
    for canonical in (False, True):
        want = es.reference_words(b, canonical)
        assert len(want) == g.n_kmers == sum(c.nk for c in g.chunks)
        lo, hi, per_read = _oracle_words(Oracle(b.K, b.pb, canonical), b.reads)
        wlo, whi = es.words_as_arrays(want)
        bad = np.flatnonzero((lo != wlo) | (hi != whi)) if len(lo) == len(wlo) else [min(len(lo), len(wlo))]
        assert len(lo) == len(wlo) and not len(bad), "canonical %s: the oracle and pyref differ at word %d: %s" % (canonical, bad[0], es.locate(g, int(bad[0])))
        if per_read_model is not None:
            assert per_read == per_read_model
    assert g.n_kmers < 75_000
    for what, (reach, cap) in es.lds_bounds(g).items():
        assert reach <= cap, (what, reach, cap)
    starts = [c.start for c in g.chunks]
    assert starts == sorted(starts) and len(set(starts)) == len(starts)
    for t in g.tiles:  # a tile owns the chunks that start inside it, all of them
        assert all(t.t * es.ENC_TILE_BYTES <= c.start < (t.t + 1) * es.ENC_TILE_BYTES for c in g.chunks[t.c0:t.c1])
    assert sum(t.nc for t in g.tiles) == len(g.chunks) and sum(t.Q for t in g.tiles) == g.n_kmers


# ---- 1. LDS capacities ---------------------------------------------------------------------------------------------------------------------------
@_param(_cases("fullest_tile"))
def test_fullest_tile(case):
    b = es.batch(case)
    K, g = b.K, b.geometry
    assert [len(r) for r in b.reads] == [4096, 4095, 2048 + K - 1]
    t = g.tiles[1]
    assert [(c.read, c.j, c.start % es.ENC_TILE_BYTES, c.nk) for c in g.chunks[t.c0:t.c1]] == [(1, 0, 0, 2048), (1, 1, 2048, 2048 - K), (2, 0, 4095, 2048)]
    assert (t.nc, t.Q, t.span, t.A0) == (3, 6144 - K, 4095 + 2048 + K - 1, 4096)
    assert t.hbase == (4096 - (K - 1)) % 4096 and t.windows == (0, 1, 2) and not t.uniform
    reach = es.lds_bounds(g)
    assert reach["k-mers of a tile"] == (6144 - K, es.ENC_MAX_KMERS) and reach["bytes a tile spans"] == (4095 + 2048 + K - 1, es.ENC_MAX_BASES)
    assert reach["histogram windows (s_hist)"] == (3, es.ENC_HIST_WINDOWS)
    assert reach["strand words (s_par, s_parpre)"][0] == 6144 // 64 + 1
    assert (t.span + 15) // 16 + es.ENC_READ_AHEAD < es.ENC_CODE_WORDS and t.last_word < t.nwords + es.ENC_READ_AHEAD
    # no legal tile is fuller: its chunks start at bytes 0 .. 4095 behind A0, the last one holds 2048 + K - 1 bytes at the most, and its k-mers start at
    # distinct bytes in front of the last chunk's last k-mer
    assert 4095 + 2048 + 59 - 1 <= es.ENC_MAX_BASES and 4095 + 2048 <= es.ENC_MAX_KMERS and (4095 + 4095 + 2047) // es.ENC_HIST_WINDOW < es.ENC_HIST_WINDOWS


@_param(_cases("most_chunks"))
def test_most_chunks(case):
    b = es.batch(case)
    g, L = b.geometry, case[1][0]
    assert b.K == 5 and len(b.reads) == es.MOST_CHUNKS_READS and all(len(r) == L for r in b.reads) and g.arithmetic
    per_tile = -(-es.ENC_TILE_BYTES // L)
    assert g.tiles[0].nc == per_tile and g.tiles[1].nc == es.MOST_CHUNKS_READS - per_tile
    if L == 5:  # chunks of K bytes at the smallest K: no tile owns more
        assert per_tile == 820 <= es.ENC_MAX_CHUNKS and es.lds_bounds(g)["chunks of a tile (s_koff, s_cstart, s_cfwd)"][0] == 820
    for t in g.tiles:
        assert t.uniform and (t.nk0, t.len0, t.dci, t.dj) == (L - 4, L, 256 // (L - 4), 256 % (L - 4))


# ---- 2. the in-tile uniform loop -----------------------------------------------------------------------------------------------------------------
@_param(_cases("uniform_nk0"))
def test_uniform_nk0(case):
    K, nk0, twin = case[1]
    b = es.batch(case)
    g, L = b.geometry, nk0 + K - 1
    plain = es.batch(("uniform_nk0", (K, nk0, False)))
    live = [t for t in g.tiles if t.nc]
    assert len(b.reads) >= 3 and g.total >= 3 * es.ENC_TILE_BYTES and len(live) >= 3
    if not twin:
        assert all(len(r) == L for r in b.reads) and g.arithmetic
        for t in live:
            assert t.uniform and (t.nk0, t.dci, t.dj) == (nk0, 256 // nk0, 256 - (256 // nk0) * nk0) and (t.nc == 1 or t.len0 == L)
            assert es.uniform_walk(nk0, t.Q) == [divmod(q, nk0) for q in range(t.Q)]
        return
    assert b.reads[:-1] == plain.reads[:-1] and b.reads[-1][:-1] == plain.reads[-1] and not g.arithmetic
    last = [c for c in g.chunks if c.read == len(b.reads) - 1]
    first_tile = last[0].start // es.ENC_TILE_BYTES
    assert first_tile >= 2 and g.tiles[:first_tile] == plain.geometry.tiles[:first_tile] and all(t.uniform for t in g.tiles[:first_tile] if t.nc)
    assert any(not g.tiles[c.start // es.ENC_TILE_BYTES].uniform for c in last)


@pytest.mark.parametrize("nk0", es.UNIFORM_NK0 + tuple(es.MOST_CHUNKS_LENGTHS[i] - 4 for i in (2, 3)))
def test_the_wrap_test_matters_where_a_lane_lands_on_nk0(nk0):
    """A k-mer at position 0 of a chunk, 256 or more k-mers into the tile, is reached by a wrap from j + dj == nk0 unless dj == 0: every nk0 that
    does not divide 256 tells `>=` from `>`; 1, 2, 128 and 256 (and 4) cannot."""
    Q = min(6000, 30 * nk0 + 999)
    want = [divmod(q, nk0) for q in range(Q)]
    assert es.uniform_walk(nk0, Q) == want
    assert (es.uniform_walk(nk0, Q, strict_wrap=True) != want) == (256 % nk0 != 0)
    if nk0 in es.UNIFORM_NK0 and 256 % nk0:  # and the crafted tiles are long enough to show it (at nk0 = 3 not those of K = 59: 204 k-mers, one trip)
        tiles = [t for k in es.UNIFORM_K for t in es.batch(("uniform_nk0", (k, nk0, False))).geometry.tiles if t.nc]
        assert any(es.uniform_walk(nk0, t.Q, strict_wrap=True) != es.uniform_walk(nk0, t.Q) for t in tiles)


# ---- 3. chunk seams and tile phases --------------------------------------------------------------------------------------------------------------
@_param(_cases("chunk_seams"))
def test_chunk_seams(case):
    K, order = case[1]
    b = es.batch(case)
    g = b.geometry
    kmers = [len(r) - K + 1 for r in b.reads]
    assert sorted(kmers) == sorted(es.SEAM_KMERS)
    assert kmers == {"plain": list(es.SEAM_KMERS), "reversed": list(es.SEAM_KMERS[::-1]), "tail": [1, 2, 2047, 2048, 2049, 4096, 4097, 6145, 4095]}[order]
    for i, nk in enumerate(kmers):
        mine = [c for c in g.chunks if c.read == i]
        assert [c.nk for c in mine] == [2048] * ((nk - 1) // 2048) + [(nk - 1) % 2048 + 1]
        assert all(a.start + a.length - b2.start == K - 1 for a, b2 in zip(mine, mine[1:]))  # neighbours share K - 1 bytes
    assert sum(c.length == K for c in g.chunks) == 4  # the read of one k-mer and the last chunks of 2049, 4097 and 6145
    phases = {o: {c.start % es.ENC_TILE_BYTES for c in es.batch(("chunk_seams", (K, o))).geometry.chunks} for o in es.SEAM_ORDERS}
    assert phases["plain"] != phases["reversed"] != phases["tail"] != phases["plain"]
    # a tile without a chunk start: only the stream's last, behind a chunk that crosses into it
    assert [t.t for t in g.tiles if t.nc == 0] == ([len(g.tiles) - 1] if order == "tail" else [])
    if order == "tail":
        assert g.chunks[-1].nk == 2047 and g.chunks[-1].start // es.ENC_TILE_BYTES == len(g.tiles) - 2


@_param(_cases("tile_phase"))
def test_tile_phase(case):
    lead, at = case[1]
    b = es.batch(case)
    g = b.geometry
    assert b.K == 31 and g.bias == 0 and g.offsets[0] == lead and len(b.reads[1]) == 2048 + 30
    second = [c for c in g.chunks if c.read == 1]
    assert len(second) == 1 and second[0].start == at and second[0].nk == 2048
    t = g.tiles[at // es.ENC_TILE_BYTES]
    assert g.chunks[t.c1 - 1] == second[0]
    # in front of a tile edge the full chunk is the last of tile 0, which then spans 4094 | 4095 + 2078 bytes from the first read's second chunk on;
    # behind it the chunk has tile 1 to itself, 0 | 1 bytes in
    assert (t.t, t.nc) == ((0, 3) if at < 4096 else (1, 1))
    if at >= 4096:
        assert t.A0 == 4096 and second[0].start - t.A0 == at - 4096 and t.uniform and t.nk0 == 2048 and (t.dci, t.dj) == (0, 256)
    if lead:
        assert g.chunks[0].start == lead


# ---- 4. invalid bytes ----------------------------------------------------------------------------------------------------------------------------
@_param(_cases("dirty_positions"))
def test_dirty_positions(case):
    b = es.batch(case)
    K, g = b.K, b.geometry
    L = es.DIRTY_READ_KMERS + K - 1
    at = es.dirty_positions_at(K)
    assert len(set(at)) == 12 and [es.dirty_overlap(K, a) for a in at] == [False] * 6 + [True, True, False, False, True, False]
    for i, a in enumerate(at):
        r = b.reads[i]
        assert len(r) == L and [j for j, c in enumerate(r) if c not in es.VALID] == [a] and r[a] == ord("N")
        mine = [c for c in g.chunks if c.read == i]
        assert [c.length for c in mine] == [2048 + K - 1, 2048 + K - 1, 7 + K - 1]
        dirty = [c.j for c in mine if c.dirty]
        assert dirty == [j for j in range(3) if 2048 * j <= a < 2048 * j + mine[j].length]
        assert len(dirty) == (2 if es.dirty_overlap(K, a) else 1)
        for c in mine:  # an N among the first K bytes of a chunk costs no k-mer, one behind them costs one
            assert c.nk == c.length - K + 1 - (1 if c.dirty and a - 2048 * c.j >= K else 0)
    all_n_head, only_n, sparse = b.reads[12:15]
    assert all_n_head[:K] == b"N" * K and all(c in es.VALID for c in all_n_head[K:])
    assert set(only_n) == {ord("N")} and [c.nk for c in g.chunks if c.read == 13] == [1]
    assert len(sparse) == 2 * K and sum(c in es.VALID for c in sparse) == K - 1
    for canonical in (False, True):  # the read of N alone gives the zero k-mer: necklace 0 at position 0
        assert pyref.seq_words(only_n, pyref.params(K, b.pb), canonical) == [0]
    short = b.reads[15:]
    assert [(len(r), [j for j, c in enumerate(r) if c not in es.VALID]) for r in short] == [(n, [a]) for n, a in es.DIRTY_SHORT]
    assert len(short) == 15 and all(r[a] == ord("n") for r, (_, a) in zip(short, es.DIRTY_SHORT))
    assert all(c.dirty for c in g.chunks if c.read >= 12)


@_param(_cases("dirty_among_clean"))
def test_dirty_among_clean(case):
    b = es.batch(case)
    g = b.geometry
    dirty = [c.read for c in g.chunks if c.dirty]
    assert b.K == 31 and all(len(r) == 150 for r in b.reads) and len(g.chunks) == len(b.reads)
    if case[1][0] == "few":
        assert tuple(dirty) == es.AMONG_DIRTY_READS and len(dirty) % es.DIRTY_WAVES == 2
        assert g.tiles[0].nc == 28 and g.tiles[1].c0 == 28  # reads 26, 27 close tile 0 and read 28 opens tile 1
        assert [t.uniform for t in g.tiles] == [False, False, True]
    else:
        assert dirty == list(range(1, 600, 2)) and len(b.reads) == 600 and dirty[-1] // es.DIRTY_LIST_THREADS == 2
        assert not any(t.uniform for t in g.tiles)


# ---- 5. the necklace on the device ---------------------------------------------------------------------------------------------------------------
def _zero_runs(read):
    """lengths of the runs of zero bits of the k-mer's ring (ACTG = 0, 1, 2, 3)"""
    code = {65: "00", 67: "01", 84: "10", 71: "11"}
    bits = "".join(code[c] for c in read)
    if "1" not in bits:
        return {len(bits)}
    at = bits.index("1")
    return {len(z) for z in (bits[at:] + bits[:at]).split("1") if z}


@_param(es.NECKLACE_CASES)
def test_necklace_families(case):
    K = case[1][0]
    b = es.batch(case)
    g = b.geometry
    reads = set(b.reads)
    assert all(len(r) == K for r in b.reads) and len(reads) == len(b.reads) and g.n_kmers == len(b.reads) >= 200 + K and g.arithmetic
    assert all(t.uniform and t.nk0 == 1 for t in g.tiles if t.nc)
    for r in es.NECKLACE_RUNS + (K - 1,):
        if r >= K:
            continue
        for bg in b"CGT":
            for o in range(K):
                want = bytearray([bg]) * K
                for i in range(r):
                    want[(o + i) % K] = ord("A")
                assert bytes(want) in reads
    for p in b"ACGT":
        assert bytes([p]) * K in reads
    assert all(((x + y) * K)[ph:ph + K] in reads for x in (b"A", b"C", b"G", b"T") for y in (b"A", b"C", b"G", b"T") for ph in (0, 1))
    assert all((u * K)[ph:ph + K] in reads for u in (b"ACG", b"TTA", b"GAT", b"CCG") for ph in range(3))
    assert all(b"A" * o + b"C" + b"A" * (K - 1 - o) in reads for o in range(K))
    runs = set().union(*[_zero_runs(r) for r in b.reads])
    assert {2 * K, 2 * K - 1, 2 * K - 2}.issubset(runs)  # poly-A, A^(K-1) C, A^(K-1) G
    if K >= 9:
        assert {10, 11, 12, 13}.issubset(runs)  # either side of the necklace's 11-bit step
    wrapping = [r for r in b.reads if r[0] == 65 and r[-1] == 65 and set(r[1:-1]) in ({67}, {71}, {84})]
    assert len(wrapping) >= 3
