"""torch.distributed integration: one process per GPU (or per CPU rank).

Replaces the reference's MPI process layer (MPI_Init / Comm_rank / size /
Barrier / Finalize: stage2-mpi/poisson_mpi_decomp.cpp:464-500,
stage4-mpi+cuda/poisson_mpi_cuda2.cu:986-1036) and its transports:

* GPU ranks: torch.distributed provides the rendezvous (TCPStore from
  torchrun's MASTER_ADDR/PORT) and the process group (backend "nccl" = RCCL
  on ROCm); the solver's per-iteration traffic runs on a native RCCL
  communicator whose unique id travels through that same store, so the
  C++ loop enqueues ncclSend/ncclRecv/ncclAllReduce on its own HIP stream
  with no Python in the iteration (and the loop stays hipGraph-capturable).
* CPU ranks: the native CPU solver calls back into Python for halo
  exchange (batched isend/irecv) and scalar allreduce over a gloo group —
  the MPI_Isend/Irecv/Waitall + MPI_Allreduce pattern of stage2/3
  (:241-347, :396-439) on a transport that exists on every box.
"""

from __future__ import annotations

import atexit
import datetime
import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
import torch.distributed as dist

from .._loader import native


_GLOO = None
_COMMS: dict = {}  # one native communicator per (world, transport) for the whole process
_UID_CALLS = 0


@dataclass
class DistContext:
    rank: int
    world: int
    local_rank: int
    backend: str
    initialized_here: bool


def env_rank_world():
    rank = int(os.environ.get("RANK", os.environ.get("PE_RANK", "0")))
    world = int(os.environ.get("WORLD_SIZE", os.environ.get("PE_WORLD_SIZE", "1")))
    local = int(os.environ.get("LOCAL_RANK", os.environ.get("PE_LOCAL_RANK", str(rank))))
    return rank, world, local


def init(backend: Optional[str] = None, timeout_s: float = 300.0) -> DistContext:
    """Initialise torch.distributed from torchrun-style env vars (idempotent).

    backend=None → "cpu:gloo,cuda:nccl" when a GPU is visible, else "gloo".
    """
    rank, world, local = env_rank_world()
    if dist.is_available() and dist.is_initialized():
        return DistContext(dist.get_rank(), dist.get_world_size(), local, dist.get_backend(), False)
    if backend is None:
        backend = "cpu:gloo,cuda:nccl" if torch.cuda.is_available() else "gloo"
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    kw = dict(backend=backend, rank=rank, world_size=world, timeout=datetime.timedelta(seconds=timeout_s))
    if torch.cuda.is_available() and "nccl" in backend:
        torch.cuda.set_device(local % max(1, torch.cuda.device_count()))
    dist.init_process_group(**kw)
    # A rank process that ends with its process group alive races the
    # interpreter's teardown against the group's worker threads: a joinable
    # std::thread destroyed at exit is std::terminate ("terminate called
    # without an active exception", SIGABRT — seen on busy machines in one rank
    # of three after its solve had finished and its result was written, on CPU
    # ranks and on GPU ranks alike).  Destroy the group while the interpreter
    # is whole, as torch asks ("destroy_process_group() was not called before
    # program exit").  The native communicators do not depend on it.
    atexit.register(_destroy_at_exit)
    return DistContext(rank, world, local, backend, True)


def _destroy_at_exit():
    try:
        if dist.is_available() and dist.is_initialized():
            dist.destroy_process_group()
    except Exception:  # (a peer that is already gone: nothing left to tidy)
        pass


def shutdown(ctx: DistContext):
    if ctx.initialized_here and dist.is_initialized():
        dist.destroy_process_group()


def _store():
    from torch.distributed import distributed_c10d as c10d

    return c10d._get_default_store()


def rccl_comm(ctx: DistContext, tag: str = "pe/rccl_uid"):
    """Native device communicator over all ranks.

    Default: RCCL over xGMI, unique id via the torch store.  PE_COMM=host
    selects the host-staged gloo transport (several ranks on one GPU — RCCL
    refuses duplicate devices — for testing the multi-process path on a
    single-GPU box).

    Per-iteration sums (PE_ALLREDUCE): "p2p" (default on RCCL jobs) maps
    every peer's receive buffer over xGMI (IPC) and lets the solver's sweep
    sum its scalars over ranks inside its final reduction block — no
    allreduce launch per iteration (PE_XR=0: a one-shot P2P kernel instead).
    The set-up self-tests and every rank falls back to RCCL's allreduce if
    any rank cannot use it.  "rccl": ncclAllReduce on the device scalars."""
    nat = native()
    nat.set_device(ctx.local_rank % max(1, nat.device_count()))
    if ctx.world == 1:
        return None
    transport = os.environ.get("PE_COMM", "rccl")
    default = "rccl" if transport == "host" else "p2p"
    allreduce = os.environ.get("PE_ALLREDUCE", default)
    key = (ctx.world, ctx.rank, transport, allreduce, tag)
    if key in _COMMS:  # every solve of the job reuses it (one RCCL init, one IPC mapping)
        return _COMMS[key]
    if transport == "host":
        global _GLOO
        if _GLOO is None:
            _GLOO = dist.new_group(backend="gloo")
        comm = nat.make_host_staged_comm(ctx.rank, ctx.world, *gloo_callbacks(_GLOO))
    else:
        # a fresh store key per communicator creation (every rank counts its
        # calls identically), deleted once every rank has read it
        global _UID_CALLS
        _UID_CALLS += 1
        store = _store()
        skey = f"{tag}/{os.environ.get('TORCHELASTIC_RUN_ID', 'run')}/{_UID_CALLS}"
        if ctx.rank == 0:
            uid = nat.rccl_unique_id()
            store.set(skey, uid)
        else:
            uid = store.get(skey)
        comm = nat.make_rccl_comm(bytes(uid), ctx.rank, ctx.world)
        dist.barrier(group=_gloo_group())
        if ctx.rank == 0:
            try:
                store.delete_key(skey)
            except Exception:  # older stores: the unique key is enough
                pass
    if allreduce == "p2p":
        nat.use_p2p_allreduce(comm)  # one-shot xGMI allreduce of the per-iteration sums
    _COMMS[key] = comm
    return comm


def drop_comm(comm) -> None:
    """Forget a cached communicator after a solve that ended non-finite or
    aborted: its P2P sequence counter / slot flags may no longer match the
    peers', so the next solve of the job builds a fresh one (collectively —
    every rank sees the same non-finite status, which is computed from the
    same reduced sums, and an aborted rank ends its process)."""
    for k in [k for k, v in _COMMS.items() if v is comm]:
        del _COMMS[k]


def _gloo_group():
    global _GLOO
    if _GLOO is None:
        _GLOO = dist.new_group(backend="gloo")
    return _GLOO


# ---------------------------------------------------------------------------
# CPU ranks over gloo (callback transport of the native CPU solver)
# ---------------------------------------------------------------------------
def gloo_callbacks(group=None):
    """(reduce_fn, exchange_fn, barrier_fn) for native.cpu_solve_rank."""

    def reduce_fn(arr, is_max):
        t = torch.from_numpy(np.asarray(arr))
        dist.all_reduce(t, op=dist.ReduceOp.MAX if is_max else dist.ReduceOp.SUM, group=group)

    def exchange_fn(items):
        ops = []
        for _d, peer, send, recv in items:
            ops.append(dist.P2POp(dist.isend, torch.from_numpy(np.asarray(send)), int(peer), group=group))
            ops.append(dist.P2POp(dist.irecv, torch.from_numpy(np.asarray(recv)), int(peer), group=group))
        if ops:
            for req in dist.batch_isend_irecv(ops):
                req.wait()

    def barrier_fn():
        dist.barrier(group=group)

    return reduce_fn, exchange_fn, barrier_fn


def gather_blocks(ctx: DistContext, prob, block, w_local: np.ndarray, group=None) -> Optional[np.ndarray]:
    """Gather every rank's owned block of w into the global (M-1, N-1) array on rank 0."""
    meta = torch.tensor([block.i0, block.j0, block.nx, block.ny], dtype=torch.int64)
    metas = [torch.zeros(4, dtype=torch.int64) for _ in range(ctx.world)] if ctx.world > 1 else [meta]
    if ctx.world > 1:
        dist.all_gather(metas, meta, group=group)
    maxn = int(max(int(m[2] * m[3]) for m in metas))
    buf = torch.zeros(maxn, dtype=torch.float64)
    buf[: w_local.size] = torch.from_numpy(np.ascontiguousarray(w_local).reshape(-1))
    if ctx.world > 1:
        bufs = [torch.zeros(maxn, dtype=torch.float64) for _ in range(ctx.world)] if ctx.rank == 0 else None
        dist.gather(buf, bufs, dst=0, group=group)
    else:
        bufs = [buf]
    if ctx.rank != 0:
        return None
    out = np.zeros((prob.M - 1, prob.N - 1), dtype=np.float64)
    for m, b in zip(metas, bufs):
        i0, j0, nx, ny = (int(v) for v in m)
        out[i0 - 1 : i0 - 1 + nx, j0 - 1 : j0 - 1 + ny] = b[: nx * ny].numpy().reshape(nx, ny)
    return out
