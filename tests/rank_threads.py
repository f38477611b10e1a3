"""Ranks of a one-GPU multi-rank test in at most MAX_PROCS processes.

At most 6 processes may hold a GPU box at once, and the test process holds it too: a test starts at most MAX_PROCS = 5
processes. A job of more ranks runs several of them per process, each rank in a thread of its own with its own gloo group
(ThreadGroup: the torch.distributed calls the sharded code makes, bound to that group). A job of MAX_PROCS ranks or fewer
runs one rank per process on the default group, as before.

The worker `target(*args, threaded=False)` gets its group from `group(rank, world, port, threaded)` and gives it back with
`release(dist)`."""
import datetime
import os
import pickle
import threading

import torch
import torch.distributed as td

MAX_PROCS = 5
TIMEOUT = datetime.timedelta(seconds=900)


class ThreadGroup:
    """One rank's gloo group when several ranks share a process: the subset of torch.distributed that HostStagedGroup,
    Comm.over_group, ShardedBuilder / ShardedIndex and gather_serialized call."""

    ReduceOp = td.ReduceOp

    def __init__(self, rank: int, world: int, port: int):
        self.rank, self.world = rank, world
        store = td.TCPStore("127.0.0.1", port, world, rank == 0, timeout=TIMEOUT)
        opts = td.ProcessGroupGloo._Options()
        opts._devices = [td.ProcessGroupGloo.create_device(hostname="127.0.0.1")]
        opts._timeout = TIMEOUT
        self.pg = td.ProcessGroupGloo(td.PrefixStore("rank_threads", store), rank, world, opts)
        self.store = store

    def get_rank(self):
        return self.rank

    def get_world_size(self):
        return self.world

    def get_backend(self):
        return "gloo"

    def barrier(self):
        self.pg.barrier().wait()

    def all_reduce(self, t, op=td.ReduceOp.SUM):
        o = td.AllreduceOptions()
        o.reduceOp = op
        self.pg.allreduce([t], o).wait()

    def all_gather(self, outs, t):
        self.pg.allgather([outs], [t]).wait()

    def all_gather_object(self, outs, obj):
        data = torch.frombuffer(bytearray(pickle.dumps(obj)), dtype=torch.uint8)
        sizes = [torch.zeros(1, dtype=torch.int64) for _ in range(self.world)]
        self.all_gather(sizes, torch.tensor([data.numel()], dtype=torch.int64))
        n = max(int(s) for s in sizes)
        pad = torch.zeros(n, dtype=torch.uint8)
        pad[: data.numel()] = data
        bufs = [torch.empty(n, dtype=torch.uint8) for _ in range(self.world)]
        self.all_gather(bufs, pad)
        for i, (b, s) in enumerate(zip(bufs, sizes)):
            outs[i] = pickle.loads(b[: int(s)].numpy().tobytes())

    def all_to_all_single(self, out, inp):
        self.pg.alltoall_base(out, inp, [], [], td.AllToAllOptions()).wait()

    def isend(self, t, dst):
        return self.pg.send([t], dst, 0)

    def irecv(self, t, src):
        return self.pg.recv([t], src, 0)


def group(rank: int, world: int, port: int, threaded: bool):
    """The rank's group: torch.distributed itself (one rank per process) or a ThreadGroup."""
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    if threaded:
        return ThreadGroup(rank, world, port)
    td.init_process_group("gloo", rank=rank, world_size=world)
    return td


def release(dist):
    if dist is td:
        td.destroy_process_group()


def _host(target, arglists):
    """One process, several ranks: a thread each. The process fails if any of its ranks does."""
    errors = []

    def run(args):
        try:
            target(*args, threaded=True)
        except BaseException as e:  # noqa: BLE001 - reported below, the process exits non-zero
            import traceback

            traceback.print_exc()
            errors.append(e)

    threads = [threading.Thread(target=run, args=(a,)) for a in arglists]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    if errors:
        raise SystemExit(1)


def processes(ctx, target, world: int, args_of):
    """Unstarted processes for the `world` ranks of a job: one per rank up to MAX_PROCS ranks, else MAX_PROCS processes that
    deal the ranks out round-robin. `args_of(rank)` is the worker's positional arguments."""
    if world <= MAX_PROCS:
        return [ctx.Process(target=target, args=args_of(r)) for r in range(world)]
    return [ctx.Process(target=_host, args=(target, [args_of(r) for r in range(j, world, MAX_PROCS)])) for j in range(MAX_PROCS)]
