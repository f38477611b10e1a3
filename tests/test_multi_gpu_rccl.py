"""The multi-GPU build on a REAL multi-rank RCCL group: one process per GPU, torch.distributed nccl backend (and the native
cblx_comm on RCCL), byte-identical to the one-process oracle. RCCL needs a GPU and a process per rank; at most 6 processes may
hold a GPU box at once, and this test process holds it too, so it runs a job of at most 5 ranks on at least as many GPUs. Any
other job (fewer GPUs than ranks: RCCL refuses two ranks on one GPU; more ranks than processes) runs every rank on GPU 0 with
the exchange staged through gloo (HostStagedGroup; cblx_comm over host callbacks), its ranks dealt to at most 5 processes
(tests/rank_threads.py), and the same assertions hold. DESIGN_HISTORY.md §5 states the multi-GPU path as unverified on hardware
until these have run on RCCL."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import cbl_amd  # noqa: E402
from cbl_amd import synth  # noqa: E402
from oracle import Oracle  # noqa: E402

import rank_threads  # noqa: E402
import dirty_reads  # noqa: E402  (tests/)


def _ngpu():
    return torch.cuda.device_count() if torch.cuda.is_available() else 0


def _port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, k, pb, canonical, protocol, native, per, L, q, groups=0, shared=False, dirty=None, threaded=False):
    """One rank. shared=False: its own GPU, RCCL. shared=True: GPU 0 with the other ranks, collectives staged through gloo."""
    import torch.distributed as dist

    from cbl_amd import sharded

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dev = 0 if shared else rank
    torch.cuda.set_device(dev)
    if shared:
        dist = rank_threads.group(rank, world, port, threaded)
        grp = sharded.HostStagedGroup(dist)
    else:
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", rank))
        grp = dist
    sharded.MAX_MSG_BYTES = 1 << 16  # force message splitting
    try:
        comm = None
        if native:
            if shared:
                comm = cbl_amd.Comm.over_group(dist, rank, world, dev)  # host callbacks: the ranks share this GPU
            else:
                box = [cbl_amd.Comm.unique_id() if rank == 0 else None]
                dist.broadcast_object_list(box, src=0)
                comm = cbl_amd.Comm.rccl(box[0], rank, world, rank)
            comm.set_recv_groups(groups)  # 0: the default (grouped receiver, 4 groups per rank), 1: everything waits for the last record
        g = cbl_amd.CBL(k, pb, canonical=canonical, device=dev)
        sb = sharded.ShardedBuilder(g, dist if native else grp, slices=3, protocol=protocol, comm=comm)
        for batch, n in enumerate(per[rank]):
            first = sum(per[r][bb] for r in range(world) for bb in range(batch)) + sum(per[r][batch] for r in range(rank))
            d_b, d_o = synth.reads_torch(23, n, L, first_read=first, device=f"cuda:{dev}")
            if dirty:
                d_b = dirty_reads.dirty_torch(d_b, first * L, n * L, **dirty)
            sb.insert_seqs_device(d_b, d_o, n)
        blob = sharded.gather_serialized(g.serialize(), dist)
        # cfg 5: a second index at other bounds, re-shard + merge
        A = sharded.ShardedIndex(k, pb, grp, canonical=canonical, device=dev, slices=2)
        B = sharded.ShardedIndex(k, pb, grp, canonical=canonical, device=dev, slices=2)
        a_b, a_o = synth.reads_torch(31, 400, L, first_read=rank * 400, device=f"cuda:{dev}")
        A.insert_seqs_device(a_b, a_o, 400)
        nb = np.asarray(A.bounds, dtype=np.uint64) * 3 // 2 + 1
        B.bounds = np.minimum(nb, (1 << pb) - 1).astype(np.uint32)
        b_b, b_o = synth.reads_torch(77, 400, L, first_read=rank * 400, device=f"cuda:{dev}")
        B.insert_seqs_device(b_b, b_o, 400)
        A.merge_assign(B)
        mblob = sharded.gather_serialized(A.cbl.serialize(), dist)
        if rank == 0:
            q.put((blob, mblob, sb.stats["sent_bytes"]))
        if comm is not None:
            comm.close()
    finally:
        rank_threads.release(dist)


@pytest.mark.parametrize("world,k,pb,canonical,protocol,native,groups,dirty", dirty_reads.cases([
    (2, 31, 24, False, "sorted", False, 0), (2, 31, 24, True, "words", False, 0), (2, 59, 28, False, "sorted", True, 0),
    (4, 31, 24, False, "sorted", True, 0), (8, 31, 28, False, "sorted", False, 0),
    (2, 31, 24, False, "bins", True, 0), (4, 59, 28, True, "bins", True, 0), (8, 31, 28, False, "bins", True, 0),
    (2, 31, 24, False, "bins", True, 1), (8, 31, 28, False, "bins", True, 1), (4, 31, 24, True, "bins", True, 3),
    (2, 31, 28, False, "auto", True, 0), (8, 31, 26, True, "auto", True, 0),  # the library's choice ("replicate" on 2 - 3 ranks, "sorted" on 4); FINE bins at PREFIX_BITS > 24 on 8
    # "replicate" (round 6): the reads cross as bit planes (one grouped exchange of planes and offsets), every rank transforms all of them
    (2, 31, 24, False, "replicate", True, 0), (3, 59, 28, True, "replicate", True, 0), (4, 31, 28, False, "replicate", True, 3), (8, 31, 26, False, "replicate", True, 0)], [
    (2, 31, 26, True, "auto", True, 0)]))  # N, lower case, IUPAC ... (tests/dirty_reads.py), dirt on the slice cuts: "replicate" packs its planes on the device
def test_sharded_build_and_merge_on_real_rccl(world, k, pb, canonical, protocol, native, groups, dirty):
    if _ngpu() == 0:
        pytest.fail("no GPU visible: the -m gpu tests must run on the MI355X box")
    # RCCL: a GPU and a process per rank. Otherwise every rank on GPU 0, the exchange through gloo, at most 5 processes
    shared = _ngpu() < world or world > rank_threads.MAX_PROCS
    import gc

    import torch.multiprocessing as mp

    from cbl_amd.sharded import ShardedBuilder

    L = 150 if k < 59 else 250
    per = [(700, 2), (300, 450), (1, 600), (512, 0), (64, 64), (0, 900), (333, 5), (90, 90)][:world]
    gc.collect()
    torch.cuda.empty_cache()  # ranks that share this GPU find what earlier tests left cached given back
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _port()
    spec = dict(seed=37, L=L, k=k, cuts=dirty_reads.slice_cuts(per, L, 3), all_n=[]) if dirty else None
    procs = rank_threads.processes(ctx, _worker, world, lambda r: (r, world, port, k, pb, canonical, protocol, native, per, L, q, groups, shared, spec))
    for p in procs:
        p.start()
    blob, mblob, sent = q.get(timeout=900)
    for p in procs:
        p.join(timeout=300)
        assert p.exitcode == 0
    one = Oracle(k, pb, canonical)
    for batch in range(2):
        first = sum(per[r][bb] for r in range(world) for bb in range(batch))
        starts = [first + sum(per[rr][batch] for rr in range(r)) for r in range(world)]
        sl = [ShardedBuilder.slice_bounds(per[r][batch], 3) for r in range(world)]
        for c in range(3):
            for r in range(world):
                a, b = sl[r][c]
                if b > a:
                    hb, ho = synth.reads(23, b - a, L, first_read=starts[r] + a)
                    if spec:
                        hb = dirty_reads.dirty_np(hb, (starts[r] + a) * L, **spec)
                    one.insert_seqs(hb, ho)
    assert blob == one.serialize() and sent > 0

    def one_process(seed):
        o = Oracle(k, pb, canonical)
        for a, b in ShardedBuilder.slice_bounds(400, 2):
            for r in range(world):
                hb, ho = synth.reads(seed, b - a, L, first_read=r * 400 + a)
                o.insert_seqs(hb, ho)
        return o

    oa, ob = one_process(31), one_process(77)
    oa.merge(ob)
    assert mblob == oa.serialize()
