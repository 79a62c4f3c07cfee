"""Test infrastructure: `Comm` whose collectives run over gloo on HOST copies of the engine's CUDA tensors.

RCCL refuses two ranks on one device, so tests that put several ranks of the product engine (`HipEngine`) on the one GPU of
the box route the collectives of `ShardedKiez` through this class: the C-ABI kernels see real multi-shard data, the
exchange itself runs over gloo (the RCCL collectives are covered by tests/test_gpu_sharded_rccl.py and
tests/test_gpu_northstar.py with one rank and every collective forced).

`StagedComm(pg)` runs on one explicit gloo process group instead of the default one: several ranks can then live in ONE
process, one thread each (every rank its own `HipEngine`, i.e. its own stream and context), so that a run of many ranks keeps
the number of processes holding the GPU small."""
import torch
import torch.distributed as dist

from kiez_amd.distributed import Comm


class _GroupCalls:
    """The torch.distributed calls `Comm` issues on host tensors, bound to the process group `pg` (any `group=` is ignored)."""

    ReduceOp = dist.ReduceOp

    def __init__(self, pg):
        self.pg = pg

    def broadcast(self, t, src=0, group=None):
        opts = dist.BroadcastOptions()
        opts.rootRank, opts.rootTensor = src, 0
        self.pg.broadcast([t], opts).wait()

    def all_gather(self, parts, t, group=None):
        self.pg.allgather([parts], [t]).wait()

    def all_to_all_single(self, out, t, output_split_sizes=None, input_split_sizes=None, group=None):
        self.pg.alltoall_base(out, t, output_split_sizes, input_split_sizes, dist.AllToAllOptions()).wait()

    def all_reduce(self, t, op=dist.ReduceOp.SUM, group=None):
        opts = dist.AllreduceOptions()
        opts.reduceOp = op
        self.pg.allreduce([t], opts).wait()


class StagedComm(Comm):
    def __init__(self, pg=None):
        super().__init__()
        if pg is not None:
            self.dist = _GroupCalls(pg)
            self.rank, self.world = pg.rank(), pg.size()

    def broadcast(self, t, src=0):
        h = t.cpu()
        self.dist.broadcast(h, src=src)
        t.copy_(h)
        return t

    def broadcast_begin(self, t, src=0):
        self.broadcast(t, src)      # staged: nothing to overlap
        return None

    def all_gather_rows(self, t, counts):
        return super().all_gather_rows(t.cpu(), counts).to(t.device)

    def all_to_all_rows(self, t, counts):
        return super().all_to_all_rows(t.cpu(), counts).to(t.device)

    def all_gather_vec(self, values, device):
        return super().all_gather_vec(values, torch.device("cpu"))

    def all_reduce_min(self, t):
        h = t.cpu()
        self.dist.all_reduce(h, op=self.dist.ReduceOp.MIN)
        t.copy_(h)
        return t
