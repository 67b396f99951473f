"""One entry point for every backend.

The reference ships five executables (stage0 serial, stage1 OpenMP, stage2
MPI, stage3 MPI+OpenMP, stage4 MPI+CUDA; README.md:7-13).  Here they are
backends of one solver:

==============  ==========================================================
backend         what runs
==============  ==========================================================
``serial``      native CPU oracle, 1 thread  (stage0; --norm unweighted = stage0's stop rule)
``omp``         native CPU, OpenMP threads   (stage1)
``ranks``       native CPU, P thread-ranks × T OpenMP threads (stage2 / stage3)
``dist-cpu``    one process per rank over torch.distributed gloo (stage2 / 3 multi-process)
``hip``         device-resident PCG on MI355X; one process per GPU over RCCL (stage4)
``hip-group``   P virtual ranks on one GPU (decomposition testing)
``torch``       PyTorch fp64 oracle (any torch device)
==============  ==========================================================
"""

from __future__ import annotations

import dataclasses
import time
from typing import Optional

import numpy as np

from ._loader import native
from .models.ellipse import EllipseProblem
from .parallel import decomp as _decomp

BACKENDS = ("serial", "omp", "ranks", "dist-cpu", "hip", "hip-group", "torch")


@dataclasses.dataclass
class SolveReport:
    backend: str
    M: int
    N: int
    ranks: int
    Px: int
    Py: int
    threads: int
    iters: int
    converged: bool
    breakdown: bool
    last_diff: float
    timers: dict
    l2_err: float
    max_err: float
    max_outside: float
    init: str = "zero"
    w: Optional[np.ndarray] = None
    rank: int = 0
    algo: str = ""
    nonfinite: bool = False
    history: Optional[list] = None  # ‖Δw‖ per iteration (keep_history=True)
    comm: str = ""  # device transport of a multi-rank HIP run (e.g. "rccl", "p2p-allreduce+rccl")
    xr: bool = False  # the sweep sums its scalars over ranks itself (P2P transport, no allreduce launch)
    halo_push: bool = False  # the sweep pushes its edge rows to the neighbours over xGMI (no exchange call)
    # first cross-device run diagnostics (this rank's): the P2P transport's set-up ("ok" / "fallback: why"),
    # the halo push's ("on" / "off: why" / "fallback: why"), the per-sweep sums' transport, and
    # hipDeviceCanAccessPeer toward every rank's device (1 / 0, -1 same device)
    overlap: bool = False  # the halo exchange runs on a second stream while the sweep's interior items run
    halo_put: bool = False  # the halo phases go through the peer-put kernel (p2p.hip kPut), not the comm
    # the halo path chosen at construction ("exchange" / "put" / "push" [+overlap]) and the candidates' timings
    # ([path, us per sweep], max over ranks), the peer put's set-up status
    halo_path: str = ""
    halo_candidates: Optional[list] = None
    put_status: str = ""
    p2p_sum_setup: str = ""
    push_status: str = ""
    sums: str = ""
    peer_access: Optional[list] = None
    resident_fallback: bool = False  # a resident launch aborted (barrier timeout); the solve finished streaming
    # end-of-solve true-residual check (device single-sweep-layout paths, -1: not computed): E-norm of
    # B - A w for the returned w, ||B||, and (three-step) the recurrence's ||r|| of the same iterate, the
    # gap ||B - A w - r|| / ||r||, and the restarts (residual replacement) the gap triggered
    res_true: float = -1.0
    res_rec: float = -1.0
    res_gap: float = -1.0
    b_norm: float = -1.0
    restarts: int = 0
    # return_w="device" on a multi-process hip job: w is this rank's owned block and (i0, j0) the global
    # 1-based node index of its first entry (None: w is the global array)
    w_origin: Optional[tuple] = None
    # return_grad: the gradient of w, float64 (2, M-1, N-1), [0] = d/dx, [1] = d/dy (True: numpy; "device": a GPU
    # tensor written by the solver, on a multi-process job this rank's block (2, nx, ny) at w_origin), and its
    # functionals h1 h2 sum_D w, h1 h2 sum_D |grad|^2 and max_D |grad| (-1: not requested)
    grad: Optional[np.ndarray] = None
    integral: float = -1.0
    energy: float = -1.0
    grad_max: float = -1.0
    # the problem's shift σ of (A + σI) w = B (to_dict() / --json carry it only when it is non-zero)
    shift: float = 0.0
    # the stop rule and, under "residual": atol, sqrt(g_0), sqrt(g_K) of the returned iterate of a converged solve and
    # the threshold used, g = h1·h2·(z, r) (-1: does not apply; to_dict() / --json carry the five only when stop != "step")
    stop: str = "step"
    atol: float = 0.0
    res_nat0: float = -1.0
    res_nat: float = -1.0
    stop_thr: float = -1.0
    # the solve had a reaction field (to_dict() / --json carry "reaction": true only then)
    reaction: bool = False

    @property
    def iters_per_s(self) -> float:
        t = self.timers.get("iterate") or self.timers.get("solver") or 0.0
        return self.iters / t if t > 0 else 0.0

    def to_dict(self) -> dict:
        # (w and grad, arrays or device tensors, are not copied)
        d = dataclasses.asdict(dataclasses.replace(self, w=None, grad=None))
        d.pop("w", None)
        d.pop("grad", None)
        d["iters_per_s"] = self.iters_per_s
        if not d.get("shift"):
            d.pop("shift", None)
        if not d.get("reaction"):
            d.pop("reaction", None)
        if d.get("stop") == "step":
            for key in ("stop", "atol", "res_nat0", "res_nat", "stop_thr"):
                d.pop(key, None)
        return d


@dataclasses.dataclass
class FieldResult:
    """What apply_operator() / residual() return.  ``field``: A v (or B − A w) over
    the global interior, float64 (M-1, N-1) — numpy (out="host"; None on the
    ranks of a multi-process job other than 0), a GPU tensor (out="device"; on a
    multi-process ``hip`` job this rank's owned block, ``origin`` = (i0, j0) the
    global 1-based node index of its first entry) or None (out="sum").
    ``sum``: h1·h2·Σ v·(A v), or h1·h2·Σ (B − A w)² = ‖B − A w‖²_E."""
    field: object
    sum: float
    origin: Optional[tuple] = None


ALGOS = {"auto": 0, "classic": 1, "fused": 2, "two-step": 3, "three-step": 4}


def _options(init="zero", seed=1234, threads=1, chunk=0, graph=False, timing=False, check_tol=True, variant=0,
             keep_history=False, log_every=0, algo="auto", checkpoint_every=0, checkpoint=None, resume=None):
    nat = native()
    o = nat.SolveOptions()
    o.init = nat.Init.Random if init == "random" else nat.Init.Zero
    o.seed = int(seed)
    o.threads = int(threads)
    o.chunk = int(chunk)
    o.use_graph = bool(graph)
    o.timing = bool(timing)
    o.check_tol = bool(check_tol)
    o.variant = int(variant)
    o.algo = ALGOS[algo] if isinstance(algo, str) else int(algo)
    o.keep_history = bool(keep_history)
    o.checkpoint_every = int(checkpoint_every)
    o.checkpoint_path = str(checkpoint or "")
    o.resume_path = str(resume or "")
    o.log_every = int(log_every)
    return o


def user_field(name: str, f, prob: EllipseProblem) -> Optional[np.ndarray]:
    """A user field (rhs / w0 / exact) as a C-contiguous float64 array of the global
    interior, shape (M-1, N-1), entry [i-1, j-1] at node (x_i, y_j) — or
    ValueError: wrong shape, data that float64 cannot hold without loss
    (wider floats, large integers, complex, non-numeric), non-finite values."""
    if f is None:
        return None
    if is_device_tensor(f):  # (the host path: one device → host copy)
        f = f.detach().cpu()
    if hasattr(f, "detach") and hasattr(f, "numpy"):  # a CPU torch tensor
        f = f.detach().numpy()
    a = np.asarray(f)
    if a.dtype.kind not in "biuf":
        raise ValueError(f"{name}: dtype {a.dtype} is not real numeric data")
    if a.shape != (prob.M - 1, prob.N - 1):
        raise ValueError(f"{name}: expected the global interior, shape {(prob.M - 1, prob.N - 1)}, got {a.shape}")
    out = np.ascontiguousarray(a, dtype=np.float64)
    if a.dtype != np.float64 and not np.array_equal(out.astype(a.dtype), a):
        raise ValueError(f"{name}: {a.dtype} values cannot be converted to float64 without loss")
    if not np.isfinite(out).all():
        raise ValueError(f"{name}: non-finite values")
    return out


def is_device_tensor(f) -> bool:
    """A torch tensor in GPU memory (what the hip backends take without a host copy)."""
    return hasattr(f, "data_ptr") and bool(getattr(f, "is_cuda", False))


def tensor_spec(name: str, t, prob: EllipseProblem):
    """(address of element [0, 0], stride_i, stride_j, is_float32) of a torch
    tensor holding a global interior field — what DeviceSolver.set_rhs_device /
    set_w0_device / set_exact_device take.  Strides are in elements; any are accepted (a
    transposed view, a window of a larger tensor, 0 for an expanded one).
    ValueError: a shape other than (M-1, N-1), a dtype other than float64 /
    float32."""
    import torch

    if t.dtype not in (torch.float64, torch.float32):
        raise ValueError(f"{name}: dtype {t.dtype} on the device must be torch.float64 or torch.float32")
    if tuple(t.shape) != (prob.M - 1, prob.N - 1):
        raise ValueError(f"{name}: expected the global interior, shape {(prob.M - 1, prob.N - 1)}, got {tuple(t.shape)}")
    si, sj = t.stride()
    return int(t.data_ptr()), int(si), int(sj), t.dtype == torch.float32


def device_field(name: str, f, prob: EllipseProblem, index: int):
    """tensor_spec of a GPU tensor for a solver running on cuda:`index`, after
    the checks of the host path: ValueError for a tensor on another device
    and for non-finite values (torch.isfinite over the whole global tensor, so
    every rank of a multi-process job decides alike without a collective)."""
    import torch

    t = f.detach()
    spec = tensor_spec(name, t, prob)
    if not t.is_cuda or t.device.index != index:
        raise ValueError(f"{name}: tensor on {t.device}, the solver runs on cuda:{index}")
    if not bool(torch.isfinite(t).all()):
        raise ValueError(f"{name}: non-finite values")
    return spec


def _field_arg(name, f, prob, on_device: bool):
    """A user field as solve() hands it on: None, a checked float64 host array,
    or (hip backends) the GPU tensor itself, checked where its device is known."""
    if on_device and is_device_tensor(f):
        tensor_spec(name, f, prob)  # shape / dtype now; device and values once the solver's device is known
        return f
    return user_field(name, f, prob)


def reaction_problem(prob: EllipseProblem, reaction, on_device: bool, algo="auto"):
    """(problem, field) of a call with ``reaction=``: the field checked — shape
    and dtype as ``rhs`` (a host array, or on the hip backends a GPU tensor,
    float64 / float32, any strides), every entry finite and >= 0 (on a GPU tensor
    with torch.isfinite / (c >= 0).all(), before any launch) — and the problem
    with its ``reaction`` flag set.  ValueError also for a field together with
    ``shift != 0`` and with ``algo`` fused / two-step / three-step, and for a
    problem flagged ``reaction`` without a field.  None with an unflagged
    problem passes through: today's call."""
    if reaction is None:
        if prob.reaction:
            raise ValueError("reaction: the problem has reaction=True but no field was given (pass reaction=c)")
        return prob, None
    if prob.check_shift() != 0.0:
        raise ValueError(f"reaction together with shift != 0 (got {prob.shift}): add the constant to the field")
    name = algo if isinstance(algo, str) else {v: k for k, v in ALGOS.items()}.get(int(algo), str(algo))
    if name in ("fused", "two-step", "three-step"):
        raise ValueError(f'algo "{name}": the single-sweep kernels carry no reaction field; a solve with reaction runs '
                         'algo "auto" or "classic"')
    c = _field_arg("reaction", reaction, prob, on_device)
    if is_device_tensor(c):
        import torch

        t = c.detach()
        if not bool(torch.isfinite(t).all()):
            raise ValueError("reaction: non-finite values")
        if not bool((t >= 0).all()):
            raise ValueError("reaction: negative values (the field must be >= 0 at every node: a negative coefficient "
                             "can make the system indefinite)")
    elif not bool((c >= 0.0).all()):
        raise ValueError("reaction: negative values (the field must be >= 0 at every node: a negative coefficient can "
                         "make the system indefinite)")
    return (prob if prob.reaction else dataclasses.replace(prob, reaction=True)), c


def _stream_handle(index: int) -> int:
    import torch

    return int(torch.cuda.current_stream(index).cuda_stream)


def _report(backend, prob, res, ranks, threads, init, w=None, rank=0) -> SolveReport:
    return SolveReport(
        backend=backend, M=prob.M, N=prob.N, ranks=ranks, Px=res.Px, Py=res.Py, threads=threads,
        iters=int(res.iters), converged=bool(res.converged), breakdown=bool(res.breakdown),
        last_diff=float(res.last_diff), timers=dict(res.timers), l2_err=float(res.l2_err),
        max_err=float(res.max_err), max_outside=float(res.max_outside), init=init, w=w, rank=rank,
        algo=str(getattr(res, "algo", "")), nonfinite=bool(getattr(res, "nonfinite", False)),
        history=list(res.history) if len(res.history) else None,
        resident_fallback=bool(getattr(res, "resident_fallback", False)),
        res_true=float(getattr(res, "res_true", -1.0)), res_rec=float(getattr(res, "res_rec", -1.0)),
        res_gap=float(getattr(res, "res_gap", -1.0)),
        b_norm=float(getattr(res, "b_norm", -1.0)), restarts=int(getattr(res, "restarts", 0)),
        shift=float(prob.shift), stop=str(prob.stop), atol=float(prob.atol),
        res_nat0=float(getattr(res, "res_nat0", -1.0)), res_nat=float(getattr(res, "res_nat", -1.0)),
        stop_thr=float(getattr(res, "stop_thr", -1.0)), reaction=bool(prob.reaction))


def _grad_mode(return_grad, on_device: bool, backend: str = "hip"):
    """return_grad as solve() takes it → False, "stats", True or "device"; ValueError otherwise."""
    if isinstance(return_grad, str):
        if return_grad not in ("stats", "device"):
            raise ValueError('return_grad must be True, False, "stats" or "device"')
        if return_grad == "device" and not on_device:
            raise ValueError(f'return_grad="device" needs backend "hip" or "hip-group", not "{backend}"')
        return return_grad
    return bool(return_grad)


def _set_grad(rep: SolveReport, stats, g=None) -> SolveReport:
    rep.integral, rep.energy, rep.grad_max = (float(v) for v in stats)
    rep.grad = g
    return rep


def _host_gradient(rep: SolveReport, prob: EllipseProblem, w, mode) -> SolveReport:
    """The gradient of the gathered w on the host (native.gradient_field): the CPU backends."""
    stats, g = native().gradient_field(prob.to_native(), w, mode is True)
    return _set_grad(rep, stats, None if g is None else np.asarray(g))


def solve(prob: EllipseProblem, backend: str = "hip", ranks: int = 1, threads: int = 1, decomp: str | None = None,
          init: str = "zero", seed: int = 1234, return_w: bool | str = False, device: str = "cuda", rhs=None,
          w0=None, exact=None, return_grad: bool | str = False, reaction=None, **kw) -> SolveReport:
    """Solve the fictitious-domain Poisson problem with the chosen backend.

    ``rhs`` / ``w0`` (every backend): a user right-hand side and initial guess
    as float64 arrays of the global interior, shape (M-1, N-1), entry
    [i-1, j-1] at node (x_i, y_j) — the shape ``return_w`` returns, so a
    returned ``w`` is a valid ``w0``.  B = rhs inside the ellipse and 0
    outside; r⁰ = B − A w⁰; ``w0`` overrides ``init`` (the report's ``init``
    is then "field").  With ``rhs`` the analytic solution does not apply and
    ``l2_err`` / ``max_err`` are −1 unless ``exact`` is given.  On multi-rank
    runs every rank passes the same global arrays and takes its slice.  A
    resumed solve (``resume=``) needs the same ``rhs`` (and ``exact``) again
    and ignores ``w0``.  None keeps the built-in constant F / ``init`` path bit
    for bit.

    ``prob.shift`` = σ > 0 (every backend) solves (A + σI) w = B, the discrete
    −Δu + σu = f, at every interior node of the box, with the preconditioner
    D + σ; the stop rules, norms and statuses are unchanged.  The analytic
    solution does not apply: ``l2_err`` / ``max_err`` are −1 unless ``exact``
    is given.  The device backends run the classic two-kernel path (``algo``
    "auto" or "classic"; the single-sweep kernels refuse a shift with
    ValueError).  A resumed solve needs the same shift again: checkpoints do
    not hold it.  σ must be finite and ≥ 0 (ValueError); 0 is today's solve
    bit for bit.

    ``reaction`` = c (every backend): a per-node coefficient c >= 0 over the
    global interior, in the forms ``rhs`` takes — (A + diag(c)) w = B, the
    discrete −Δu + c(x, y)·u = f, at every interior node of the box, with the
    preconditioner D + c: per node the shift's expressions with c_ij for σ
    (csrc/include/pe/fields.hpp), zeros included.  B, the stop rules, norms
    and statuses are unchanged; ``l2_err`` / ``max_err`` are −1 unless
    ``exact`` is given.  The device backends run the classic two-kernel path.
    ValueError before any work: a negative or non-finite entry, a wrong shape
    or dtype, a field together with ``shift != 0`` (add the constant to the
    field), ``algo`` fused / two-step / three-step.  A resumed solve needs the
    same field again.  None: today's solve bit for bit.

    ``prob.stop`` = "residual" (every backend) stops on the preconditioned
    residual instead of the step size: with g_k = h1·h2·Σ z_k·r_k, z = D⁻¹r —
    the scalar the recurrence forms for β anyway — iterate k is tested at the
    top of iteration k + 1, sqrt(g_k) <= max(``tol``·sqrt(g_0), ``atol``), and
    the solve ends converged with ``iters`` = k (0 for a ``w0`` that already
    meets it: ``w0`` comes back unchanged).  The iteration cap wins: the
    ``max_iter``-th iterate is not tested.  The report carries ``res_nat0`` =
    sqrt(g_0), ``res_nat`` = sqrt(g_K) and ``stop_thr``; ``last_diff`` /
    ``history`` still hold step sizes.  A time stepper passes ``atol`` =
    ``tol``·``res_nat0`` of its first step to the later, warm-started ones.  The
    device backends run one iteration per launch under it (classic, the
    resident kernel or the single sweep; ``algo`` "two-step" / "three-step"
    refuse with ValueError).  "step", the default, is the reference's rule.

    ``exact`` (every backend, same form): the solution to report the error
    against — a manufactured solution u with ``rhs`` = −Δu, say.  Then
    ``l2_err`` = sqrt(h1·h2·Σ_D (w − exact)²) and ``max_err`` = max_D
    |w − exact| over the nodes inside the ellipse, with or without ``rhs``
    (it takes the place of the analytic solution); values outside the ellipse
    are ignored.  It never enters the solve: iterations, ``w`` and every other
    figure are those of the same call without it.

    GPU tensors: on ``hip`` and ``hip-group`` any field may also be a torch
    tensor in GPU memory — float64 or float32, shape (M-1, N-1), any strides,
    on the device the solver runs on (cuda:0 for one process, the local
    rank's device otherwise).  The solver cuts its planes out of it on the
    device, ordered by events with ``torch.cuda.current_stream()``: no host
    copy, and the tensor may be overwritten or freed in that stream's order as
    soon as solve() returns.  The same values give the same bits as a host
    array.  Host arrays and GPU tensors may be mixed.  Every other backend
    copies a GPU tensor to the host first.  ``return_w="device"`` (``hip`` /
    ``hip-group`` only) returns ``w`` as a float64 GPU tensor written by the
    solver: the global array, or on a multi-process job this rank's owned
    block, with ``w_origin = (i0, j0)`` the global 1-based node index of its
    first entry (no gather).  DeviceSession keeps one constructed solver for a
    sequence of such solves.

    ``return_grad`` (every backend): the gradient of the returned ``w`` inside
    the ellipse and three functionals of it, from one definition
    (csrc/include/pe/fields.hpp): central differences where both neighbours
    are inside the ellipse, one-sided where one is (``w`` drops to O(ε)
    across the fictitious-domain boundary), 0 outside.  ``"stats"`` fills
    ``integral`` = h1·h2·Σ_D w, ``energy`` = h1·h2·Σ_D |∇w|² and ``grad_max``
    = max_D |∇w|; ``True`` also returns ``grad``, float64 (2, M-1, N-1),
    [0] = ∂x, [1] = ∂y (gathered onto rank 0 on a multi-process job, as w
    is); ``"device"`` (``hip`` / ``hip-group``) returns it as a GPU tensor
    written by the solver — on a multi-process job this rank's block
    (2, nx, ny) at ``w_origin``.  Every backend gives the same bits from the
    same ``w``.  The solve itself is that of the same call without it.

    For ``hip`` with torch.distributed initialised and world > 1 this is the
    per-rank call of a multi-GPU job (every rank calls it; rank 0's report
    carries the max-over-ranks timers and, with return_w, the gathered w).
    """
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}")
    on_device = backend in ("hip", "hip-group")
    grad = _grad_mode(return_grad, on_device, backend)
    if isinstance(return_w, str):
        if return_w != "device":
            raise ValueError('return_w must be True, False or "device"')
        if not on_device:
            raise ValueError(f'return_w="device" needs backend "hip" or "hip-group", not "{backend}"')
    rhs = _field_arg("rhs", rhs, prob, on_device)
    w0 = _field_arg("w0", w0, prob, on_device)
    exact = _field_arg("exact", exact, prob, on_device)
    prob, reaction = reaction_problem(prob, reaction, on_device, kw.get("algo", "auto"))
    if w0 is not None:
        init = "field"
    decomp = decomp or _decomp.default_spec(backend)
    nat = native()
    P = prob.to_native()
    if backend in ("serial", "omp", "ranks"):
        t = 1 if backend == "serial" else max(1, threads)
        nranks = ranks if backend == "ranks" else 1
        opt = _options(init, seed, t, keep_history=kw.get("keep_history", False), log_every=kw.get("log_every", 0))
        res, w = nat.cpu_solve_grid(P, _decomp.grid(nranks, prob.M, prob.N, decomp if backend == "ranks" else "reference"),
                                    opt, bool(return_w or grad), rhs, w0, exact, reaction)
        rep = _report(backend, prob, res, nranks, t, init, np.asarray(w) if return_w else None)
        return _host_gradient(rep, prob, w, grad) if grad else rep
    if backend == "torch":
        import torch

        from .ops import torch_ref

        if device.startswith("cuda") and not torch.cuda.is_available():
            device = "cpu"
        t0 = time.perf_counter()
        r = torch_ref.pcg(prob, device=device, w0=w0, keep_history=kw.get("keep_history", False), rhs=rhs,
                          exact=exact, reaction=reaction)
        dt = time.perf_counter() - t0
        timers = dict(solver=dt, iterate=dt)
        rep = SolveReport("torch", prob.M, prob.N, 1, 1, 1, 1, r.iters, r.converged, False,
                          r.history[-1] if r.history else 0.0, timers, r.l2_err, r.max_err, -1.0,
                          "zero" if w0 is None else "field",
                          r.w[1:-1, 1:-1].cpu().numpy() if return_w else None, shift=float(prob.shift),
                          stop=str(prob.stop), atol=float(prob.atol), res_nat0=r.res_nat0, res_nat=r.res_nat,
                          stop_thr=r.stop_thr, reaction=bool(prob.reaction))
        if grad:
            g, *stats = torch_ref.gradient(prob, r.w)
            _set_grad(rep, stats, g.cpu().numpy() if grad is True else None)
        return rep
    if backend == "hip-group":
        opt = _options(init, seed, chunk=kw.get("chunk", 0), timing=kw.get("timing", False),
                       variant=kw.get("variant", 0), check_tol=kw.get("check_tol", True),
                       algo=kw.get("algo", "auto"))
        pg = _decomp.grid(ranks, prob.M, prob.N, decomp)
        if not (is_device_tensor(rhs) or is_device_tensor(w0) or is_device_tensor(exact) or return_w == "device"
                or grad or is_device_tensor(reaction)):
            res, w = nat.device_solve_group_grid(P, pg, opt, return_w, rhs, w0, exact, reaction)
            return _report(backend, prob, res, ranks, 1, init, None if w is None else np.asarray(w))
        import torch

        index = nat.current_device()  # the virtual ranks run on the process's current device
        fields = (("rhs", rhs), ("w0", w0), ("exact", exact), ("reaction", reaction))
        dev = {n: device_field(n, f, prob, index) for n, f in fields if is_device_tensor(f)}
        host = {n: f for n, f in fields if n not in dev}
        wt = w_dev = None
        if return_w == "device":  # every block gathers into its position of this one tensor
            wt = torch.empty((prob.M - 1, prob.N - 1), dtype=torch.float64, device=f"cuda:{index}")
            w_dev = (wt.data_ptr(), wt.stride(0), wt.stride(1))
        if not grad:
            res, w = nat.device_solve_group_grid_device(P, pg, opt, bool(return_w) and wt is None, host.get("rhs"),
                                                        host.get("w0"), dev.get("rhs"), dev.get("w0"), w_dev,
                                                        _stream_handle(index), host.get("exact"), dev.get("exact"),
                                                        host.get("reaction"), dev.get("reaction"))
            if wt is None and w is not None:
                wt = np.asarray(w)
            return _report(backend, prob, res, ranks, 1, init, wt)
        gt = g_dev = None
        if grad == "device":  # every block's kernel writes its position of this one tensor
            gt = torch.empty((2, prob.M - 1, prob.N - 1), dtype=torch.float64, device=f"cuda:{index}")
            g_dev = (gt[0].data_ptr(), gt[1].data_ptr(), gt.stride(1), gt.stride(2))
        res, w, g = nat.device_solve_group_grad(P, pg, opt, bool(return_w) and wt is None, 1 if grad == "stats" else 2,
                                                host.get("rhs"), host.get("w0"), host.get("exact"), dev.get("rhs"),
                                                dev.get("w0"), dev.get("exact"), w_dev, g_dev, _stream_handle(index),
                                                host.get("reaction"), dev.get("reaction"))
        if wt is None and w is not None:
            wt = np.asarray(w)
        if gt is None and g is not None:
            gt = np.asarray(g)
        return _set_grad(_report(backend, prob, res, ranks, 1, init, wt), res.grad, gt)
    # distributed backends
    from .parallel import dist as _dist

    if backend == "dist-cpu":
        ctx = _dist.init("gloo")  # (CPU ranks need no device side; a gloo-only group is destroyed at exit)
        blk = _decomp.block(prob.M, prob.N, ctx.world, ctx.rank, decomp)
        opt = _options(init, seed, max(1, threads))
        res, w = nat.cpu_solve_rank(P, blk, *_dist.gloo_callbacks(), opt, True, rhs, w0, exact, reaction)
        wg = _dist.gather_blocks(ctx, prob, blk, np.asarray(w)) if return_w or grad else None
        rep = _report(backend, prob, res, ctx.world, threads, init, wg if return_w else None, ctx.rank)
        # (the gathered w lives on rank 0: its report carries the gradient and the figures)
        return _host_gradient(rep, prob, wg, grad) if grad and wg is not None else rep
    # hip
    with DeviceSession(prob, decomp, init=init, seed=seed, reaction=reaction, **kw) as session:
        return session._solve(rhs, w0, return_w, exact, grad)


def _out_mode(out, on_device: bool, backend: str = "hip") -> str:
    if out not in ("host", "device", "sum"):
        raise ValueError('out must be "host", "device" or "sum"')
    if out == "device" and not on_device:
        raise ValueError(f'out="device" needs backend "hip" or "hip-group", not "{backend}"')
    return out


def _operator(prob, v, rhs, residual_, backend, ranks, threads, decomp, out, device, kw, reaction=None) -> FieldResult:
    """apply_operator() / residual() on every backend."""
    name = "w" if residual_ else "v"
    if backend not in BACKENDS:
        raise ValueError(f"backend must be one of {BACKENDS}")
    on_device = backend in ("hip", "hip-group")
    out = _out_mode(out, on_device, backend)
    if v is None:
        raise ValueError(f"{name}: a field is required")
    v = _field_arg(name, v, prob, on_device)
    rhs = _field_arg("rhs", rhs, prob, on_device) if residual_ else None
    prob, reaction = reaction_problem(prob, reaction, on_device, kw.get("algo", "auto"))
    nat = native()
    P = prob.to_native()
    want = out != "sum"
    if backend in ("serial", "omp", "ranks", "dist-cpu"):
        # the host definition on the global array (every rank of a dist-cpu job holds it: no communication)
        t = 1 if backend == "serial" else max(1, threads)
        s, f = (nat.residual_field(P, v, rhs, want, t, reaction) if residual_
                else nat.apply_operator(P, v, want, t, reaction))
        rank = 0
        if backend == "dist-cpu":
            from .parallel import dist as _dist

            rank = _dist.init("gloo").rank
        return FieldResult(np.asarray(f) if want and rank == 0 else None, float(s))
    if backend == "torch":
        import torch

        from .ops import torch_ref

        if device.startswith("cuda") and not torch.cuda.is_available():
            device = "cpu"
        V = torch_ref.embed(prob, v, device)
        if residual_:
            f = torch_ref.residual(prob, V, rhs, device, reaction=reaction)[1:-1, 1:-1]
            s = float((f * f).sum())
        else:
            a, b, _ = torch_ref.assemble(prob, device)
            f = torch_ref.apply_A(V, a, b, prob.h1, prob.h2, torch_ref.reaction_coef(prob, reaction, device))[1:-1, 1:-1]
            s = float((V[1:-1, 1:-1] * f).sum())
        return FieldResult(f.cpu().numpy() if want else None, prob.h1 * prob.h2 * s)
    if backend == "hip-group":
        import torch

        opt = _options(chunk=kw.get("chunk", 0), variant=kw.get("variant", 0), algo=kw.get("algo", "auto"))
        pg = _decomp.grid(ranks, prob.M, prob.N, decomp or _decomp.default_spec(backend))
        index = nat.current_device()
        fields = ((name, v), ("rhs", rhs), ("reaction", reaction))
        dev = {n: device_field(n, f, prob, index) for n, f in fields if is_device_tensor(f)}
        host = {n: f for n, f in fields if n not in dev}
        ot = o_dev = None
        if out == "device":  # every block's kernel writes its position of this one tensor
            ot = torch.empty((prob.M - 1, prob.N - 1), dtype=torch.float64, device=f"cuda:{index}")
            o_dev = (ot.data_ptr(), ot.stride(0), ot.stride(1))
        s, f = nat.device_apply_group(P, pg, opt, residual_, host.get(name), dev.get(name), host.get("rhs"),
                                      dev.get("rhs"), o_dev, out == "host", _stream_handle(index), host.get("reaction"),
                                      dev.get("reaction"))
        return FieldResult(ot if ot is not None else (np.asarray(f) if f is not None else None), float(s))
    with DeviceSession(prob, decomp, reaction=reaction, **kw) as session:
        return session._operator(v, rhs, residual_, out, set_rhs=True)


_HIP_OPTIONS = ("chunk", "graph", "timing", "check_tol", "variant", "algo", "checkpoint_every", "checkpoint", "resume",
                "keep_history", "log_every")


class DeviceSession:
    """One constructed device solver (backend ``hip``) for a sequence of
    solves: what ``solve(backend="hip")`` does up to and including the
    construction of the native ``DeviceSolver`` — device, this rank's block,
    the communicator of a multi-process job, the options — done once and kept.

        with DeviceSession(prob) as s:
            first = s.solve(rhs=f, return_w="device")
            again = s.solve(rhs=1.01 * f, w0=first.w, return_w="device")

    ``options`` are solve()'s for the ``hip`` backend (``init``, ``seed``,
    ``algo``, ``check_tol``, ``graph``, ``chunk``, ...).  The construction time
    is reported by the first solve only (``timers["construct"]`` is 0 after).
    On a multi-process job every rank creates the session and calls solve()
    with the same global fields, as with ``solve()``.

    ``reaction=c`` (a host array or a GPU tensor, as in solve()) makes it a
    session of −Δu + c·u = f: the layout is fixed at construction, and
    ``solve(..., reaction=c2)`` replaces the field per call — a Newton loop
    passes its c = g′(u) there; left out, the last field stays.  ValueError for
    ``reaction=`` on a session constructed without one, and for None on one
    constructed with it."""

    def __init__(self, prob: EllipseProblem, decomp: str | None = None, reaction=None, **options):
        prob, reaction = reaction_problem(prob, reaction, True, options.get("algo", "auto"))  # (refusals before any work)
        nat = native()
        if nat.device_count() < 1:
            raise RuntimeError("backend 'hip' needs a visible MI355X (HIP device)")
        import torch.distributed as tdist

        from .parallel import dist as _dist

        self.prob = prob
        self.init = options.get("init", "zero")
        decomp = decomp or _decomp.default_spec("hip")
        if tdist.is_available() and tdist.is_initialized():
            self.world = tdist.get_world_size()
        else:
            self.world = _dist.env_rank_world()[1]
        opt = _options(self.init, options.get("seed", 1234), **{k: options[k] for k in _HIP_OPTIONS if k in options})
        if self.world == 1:
            self.rank, self.comm = 0, None
            nat.set_device(0)
            self.block = _decomp.block(prob.M, prob.N, 1, 0, decomp)
        else:
            ctx = _dist.init()
            self.rank = ctx.rank
            self.comm = _dist.rccl_comm(ctx)
            self.block = _decomp.block(prob.M, prob.N, self.world, self.rank, decomp)
        self.device_index = int(nat.current_device())  # device tensors must live here
        self.solver = nat.DeviceSolver(prob.to_native(), self.block, self.comm, opt)
        if reaction is not None:
            self._set_reaction(reaction)

    def _set_reaction(self, c) -> None:
        """A checked field (reaction_problem) into the solver's reaction plane."""
        if is_device_tensor(c):
            self.solver.set_reaction_device(*device_field("reaction", c, self.prob, self.device_index),
                                            _stream_handle(self.device_index))
        else:
            self.solver.set_reaction(native().block_field(self.prob.M, self.prob.N, self.block, c, 1))

    def _reaction_arg(self, reaction):
        """solve(reaction=)'s argument on this session: _KEEP passes, a field is checked; ValueError for a field on a
        session constructed without one and for None on one constructed with it."""
        if reaction is DeviceSession._KEEP:
            return reaction
        if not self.prob.reaction:
            if reaction is None:
                return DeviceSession._KEEP
            raise ValueError("reaction: this session was constructed without a reaction field (the layout is fixed at "
                             "construction: DeviceSession(prob, reaction=c))")
        if reaction is None:
            raise ValueError("reaction: None on a session constructed with a reaction field (pass a field, or leave it "
                             "out to keep the last one)")
        return reaction_problem(self.prob, reaction, True)[1]

    def close(self) -> None:
        """Release the solver (its device memory and stream); idempotent."""
        self.solver = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    _KEEP = object()

    def solve(self, rhs=None, w0=None, exact=None, return_w=False, return_grad=False, atol=None,
              reaction=_KEEP) -> SolveReport:
        """One solve on the kept solver.  ``rhs`` / ``w0`` / ``exact``: host
        arrays or GPU tensors of the global interior, per call and mixed
        freely; None clears a field back to F / ``init`` / the analytic error.  ``return_w``: False, True (numpy; on a
        multi-process job gathered onto rank 0) or "device" (a float64 GPU
        tensor written by the solver; on a multi-process job this rank's block,
        its position in the report's ``w_origin``).  ``return_grad``: False,
        "stats", True or "device", as in solve().  ``atol`` (``stop="residual"``
        only): the absolute floor of the threshold from this solve on — the
        session's problem takes it; the kept solver, and any graph it has
        captured, stay as they are (the threshold lives in device memory).
        ``reaction`` (a session constructed with one): the field of this and
        the following solves; left out, the last one stays."""
        if isinstance(return_w, str) and return_w != "device":
            raise ValueError('return_w must be True, False or "device"')
        reaction = self._reaction_arg(reaction)
        if atol is not None:
            prob = dataclasses.replace(self.prob, atol=atol)
            prob.check_stop()  # (ValueError before anything is set)
            if self.solver is None:
                raise RuntimeError("DeviceSession is closed")
            self.solver.set_atol(float(atol))
            self.prob = prob
        grad = _grad_mode(return_grad, True)
        rhs, w0, exact = (_field_arg(n, f, self.prob, True) for n, f in (("rhs", rhs), ("w0", w0), ("exact", exact)))
        if reaction is not DeviceSession._KEEP:
            if self.solver is None:
                raise RuntimeError("DeviceSession is closed")
            self._set_reaction(reaction)
        return self._solve(rhs, w0, return_w, exact, grad)

    def apply(self, v, out="host") -> FieldResult:
        """A v for a field of the caller's on the kept solver.  ``v``: a host array
        or a GPU tensor of the global interior, in the forms ``rhs`` takes
        (float64 or float32, any strides, shape (M-1, N-1), on ``device_index``).
        ``out``: "host" (numpy; on a multi-process job gathered onto rank 0),
        "device" (a float64 GPU tensor written by the kernel; on a multi-process
        job this rank's block at ``origin``) or "sum" (no field).  The result's
        ``sum`` is h1·h2·Σ v·(A v).  The pass reads the solver's tables only: the
        next solve is the same solve."""
        return self._operator(_field_arg("v", v, self.prob, True), None, False, _out_mode(out, True))

    def residual(self, w, rhs=_KEEP, out="host") -> FieldResult:
        """B − A w for an iterate of the caller's; ``sum`` is ‖B − A w‖²_E.
        ``rhs``: per call, as in solve(rhs=) — a field, or None for F; left out,
        the right-hand side of the last solve() / residual() stays.  ``w`` and
        ``out`` as in apply()."""
        if w is None:
            raise ValueError("w: a field is required")
        keep = rhs is DeviceSession._KEEP
        return self._operator(_field_arg("w", w, self.prob, True),
                              None if keep else _field_arg("rhs", rhs, self.prob, True), True, _out_mode(out, True),
                              set_rhs=not keep)

    def _operator(self, v, rhs, residual_, out, set_rhs=False) -> FieldResult:
        # v / rhs: checked host arrays or GPU tensors of checked shape and dtype (_field_arg)
        from .parallel import dist as _dist

        if self.solver is None:
            raise RuntimeError("DeviceSession is closed")
        if v is None:
            raise ValueError("v: a field is required")
        nat, s, prob, blk, comm = native(), self.solver, self.prob, self.block, self.comm
        name = "w" if residual_ else "v"
        # every refusal before anything is set or launched
        spec = device_field(name, v, prob, self.device_index) if is_device_tensor(v) else None
        rspec = device_field("rhs", rhs, prob, self.device_index) if is_device_tensor(rhs) else None
        try:
            if residual_ and set_rhs:
                if rspec is not None:
                    s.set_rhs_device(*rspec, _stream_handle(self.device_index))
                else:
                    s.set_rhs(None if rhs is None else nat.block_fields(prob.M, prob.N, blk, rhs, None)[0])
            f = origin = None
            if out == "device" or spec is not None:
                import torch

                stream = _stream_handle(self.device_index)
                if spec is None:  # a host array: one upload, then the device path
                    t = torch.tensor(v, device=f"cuda:{self.device_index}")
                    spec = tensor_spec(name, t, prob)
                dst = (0, 0, 0)
                if out != "sum":
                    f = torch.empty((blk.nx, blk.ny), dtype=torch.float64, device=f"cuda:{self.device_index}")
                    dst = (f.data_ptr(), f.stride(0), f.stride(1))
                total = s.apply_device(*spec, residual_, *dst, 0, 0, stream)
                if out == "device" and self.world > 1:
                    origin = (int(blk.i0), int(blk.j0))
                if out == "host":
                    f = f.cpu().numpy()
            else:
                total, f = s.apply(v, residual_, out == "host")
                f = None if f is None else np.asarray(f)
            if out == "host" and self.world > 1:
                f = _dist.gather_blocks(_dist.init(), prob, blk, f)
        except ValueError:
            raise  # (a refused field: nothing was launched, the session stays usable)
        except Exception:
            if comm is not None:
                _dist.drop_comm(comm)
            raise
        return FieldResult(f, float(total), origin)

    def _set_fields(self, rhs, w0, exact=None) -> None:
        """The three fields into the solver's planes; everything is checked
        before anything is set, so a refused field leaves the solver as it was."""
        nat, s, prob = native(), self.solver, self.prob
        dev = {n: device_field(n, f, prob, self.device_index) for n, f in (("rhs", rhs), ("w0", w0), ("exact", exact))
               if is_device_tensor(f)}
        host = nat.block_fields(prob.M, prob.N, self.block, None if "rhs" in dev else rhs, None if "w0" in dev else w0)
        local_exact = None if "exact" in dev or exact is None else nat.block_field(prob.M, prob.N, self.block, exact, 0)
        stream = _stream_handle(self.device_index) if dev else 0
        for n, local, set_host, set_dev in (("rhs", host[0], s.set_rhs, s.set_rhs_device),
                                            ("w0", host[1], s.set_w0, s.set_w0_device),
                                            ("exact", local_exact, s.set_exact, s.set_exact_device)):
            if n in dev:
                set_dev(*dev[n], stream)
            else:
                set_host(local)  # (None clears)

    def _gradient(self, rep: SolveReport, grad) -> None:
        """The gradient pass of the kept solver after its solve (collective on a
        multi-process job) into the report; `grad`: "stats", True or "device"."""
        from .parallel import dist as _dist

        s, blk = self.solver, self.block
        if grad == "device":
            import torch

            # single process: the block is the global interior; otherwise this rank's owned block
            g = torch.empty((2, blk.nx, blk.ny), dtype=torch.float64, device=f"cuda:{self.device_index}")
            stats = s.gradient_device(g[0].data_ptr(), g[1].data_ptr(), g.stride(1), g.stride(2), 0, 0,
                                      _stream_handle(self.device_index))
            if self.world > 1:
                rep.w_origin = (int(blk.i0), int(blk.j0))
        else:
            stats, gx, gy = s.gradient(grad is True)
            g = None
            if grad is True and self.world == 1:
                g = np.stack((np.asarray(gx), np.asarray(gy)))
            elif grad is True:
                parts = [_dist.gather_blocks(_dist.init(), self.prob, blk, np.asarray(c)) for c in (gx, gy)]
                g = None if parts[0] is None else np.stack(parts)
        _set_grad(rep, stats, g)

    def _solve(self, rhs, w0, return_w, exact=None, grad=False) -> SolveReport:
        # rhs / w0 / exact: None, checked host arrays or GPU tensors of checked shape and dtype (_field_arg)
        from .parallel import dist as _dist

        if self.solver is None:
            raise RuntimeError("DeviceSession is closed")
        nat, s, prob, comm = native(), self.solver, self.prob, self.comm
        try:
            self._set_fields(rhs, w0, exact)
            res = s.solve()
        except Exception:
            if comm is not None:
                _dist.drop_comm(comm)
            raise
        if comm is not None and (res.nonfinite or not np.isfinite(res.last_diff)):
            _dist.drop_comm(comm)  # its P2P sequence may be out of step with the peers'
        w = origin = None
        if return_w == "device":
            import torch

            # single process: the block is the global interior; otherwise this rank's owned block
            w = torch.empty((self.block.nx, self.block.ny), dtype=torch.float64, device=f"cuda:{self.device_index}")
            s.copy_w_device(w.data_ptr(), w.stride(0), w.stride(1), 0, 0, _stream_handle(self.device_index))
            if self.world > 1:
                origin = (int(self.block.i0), int(self.block.j0))
        elif return_w:
            wl = np.asarray(s.w())
            w = wl if self.world == 1 else _dist.gather_blocks(_dist.init(), prob, self.block, wl)
        rep = _report("hip", prob, res, self.world, 1, "field" if w0 is not None else self.init, w, self.rank)
        rep.w_origin = origin
        # (a multi-process solve that ended non-finite has dropped its communicator: no collective pass after it)
        if grad and (comm is None or (np.isfinite(res.last_diff) and not res.nonfinite)):
            try:
                self._gradient(rep, grad)
            except Exception:
                if comm is not None:
                    _dist.drop_comm(comm)
                raise
        rep.comm = comm.name if comm is not None else "self"
        rep.xr = bool(s.xr)
        rep.halo_push = bool(s.halo_push)
        rep.overlap = bool(s.overlap)
        rep.halo_put = bool(s.halo_put)
        rep.halo_path = str(s.halo_path)
        rep.halo_candidates = [[str(n), round(float(us), 2)] for n, us in s.halo_candidates]
        rep.put_status = str(s.put_status)
        rep.p2p_sum_setup = str(nat.p2p_setup_status())
        rep.push_status = str(s.push_status)
        rep.sums = str(s.xr_status)
        rep.peer_access = [int(v) for v in s.peer_access]
        return rep


def apply_operator(prob: EllipseProblem, v, backend: str = "hip", ranks: int = 1, threads: int = 1,
                   decomp: str | None = None, out: str = "host", device: str = "cuda", reaction=None,
                   **kw) -> FieldResult:
    """A v: the fictitious-domain operator (coefficients and expression of the
    solve) applied to a field of the caller's.  ``v``: the global interior,
    shape (M-1, N-1), 0 on the box boundary — a host array on every backend, or
    on ``hip`` / ``hip-group`` a GPU tensor in the forms ``rhs`` takes.  A v is
    taken at every interior node, inside or outside the ellipse.  ``out``:
    "host" (numpy), "device" (``hip`` / ``hip-group``: a float64 GPU tensor
    written by the kernel) or "sum" (no field); the result's ``sum`` is
    h1·h2·Σ v·(A v).  Every backend gives the definition of
    csrc/include/pe/fields.hpp; DeviceSession.apply() serves a sequence of
    calls from one constructed solver.  ``reaction`` = c: (A + diag(c)) v, the
    field as in solve()."""
    return _operator(prob, v, None, False, backend, ranks, threads, decomp, out, device, kw, reaction)


def residual(prob: EllipseProblem, w, rhs=None, backend: str = "hip", ranks: int = 1, threads: int = 1,
             decomp: str | None = None, out: str = "host", device: str = "cuda", reaction=None, **kw) -> FieldResult:
    """B − A w for an iterate of the caller's: B = ``rhs`` (None: F) inside the
    ellipse and 0 outside, as solve() masks it.  ``sum`` is h1·h2·Σ (B − A w)²,
    the square of the E-norm of the residual.  Arguments as apply_operator()
    (``reaction`` = c: B − (A + diag(c)) w)."""
    return _operator(prob, w, rhs, True, backend, ranks, threads, decomp, out, device, kw, reaction)
