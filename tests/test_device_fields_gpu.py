"""MI355X tests of user fields given as GPU tensors and of w returned on the
GPU (DeviceSolver.set_rhs_device / set_w0_device / copy_w_device — kSliceField,
kGatherW —, solve(rhs=, w0=, return_w="device"), DeviceSession).

The comparison is equality of bits throughout: a device tensor holding the
same values must give exactly what the host array gives, because both end in
the same dense planes (user_plane) that kInitField / kResidField read.  Inputs:
field_checks.py (asymmetric in x and y).  Shapes are the smallest at which
slicing can go wrong (one block, 2x2 and 2x3 blocks of 12-13 rows); every test
takes seconds."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import torch

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAME = ("iters", "last_diff", "res_true", "res_rec", "b_norm", "max_outside", "converged", "algo", "init",
        "l2_err", "max_err")


def cuda(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")  # (a copy: field_checks' arrays are read-only)


def stream():
    return torch.cuda.current_stream().cuda_stream


def same_report(dev, host, tag=""):
    """A device-field solve against the host-field solve of the same values."""
    for k in SAME:
        assert getattr(dev, k) == getattr(host, k), (tag, k, getattr(dev, k), getattr(host, k))
    assert isinstance(dev.w, torch.Tensor) and dev.w.is_cuda and dev.w.dtype == torch.float64
    assert torch.equal(dev.w.cpu(), torch.from_numpy(host.w)), tag


# ---- 1. planes ------------------------------------------------------------------------------------
def views(a):
    """The same values as differently laid out GPU tensors: (name, tensor, host values)."""
    r, c = a.shape
    t = cuda(a)
    big = torch.full((r + 6, 2 * c + 9), -7.0, dtype=torch.float64, device="cuda:0")
    big[3:3 + r, 5:5 + 2 * c:2] = t
    f32 = t.float()
    return [("contiguous", t, a),
            ("transposed", t.t().contiguous().t(), a),
            ("window", big[3:3 + r, 5:5 + 2 * c:2], a),
            ("float32", f32, f32.double().cpu().numpy())]


@pytest.mark.parametrize("M,N,ranks,decomp", [(10, 50, 1, None), (26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_planes_equal_block_fields(gpu, nat, M, N, ranks, decomp):
    """kSliceField against pe::block_field for every block: ring zeros on the
    box boundary, the neighbours' values inside, any strides, float32 widened."""
    P = EllipseProblem(M, N).to_native()
    fv, gv = views(fc.rhs(M, N)), views(fc.w0(M, N))
    assert fv[1][1].stride() == (1, M - 1) and fv[2][1].stride() == (2 * (N - 1) + 9, 2)
    for r in range(ranks):
        blk = D.block(M, N, ranks, r, decomp) if decomp else D.block(M, N, 1, 0)
        s = nat.DeviceSolver(P, blk, None, nat.SolveOptions())
        assert s.user_plane(0) is None and s.user_plane(1) is None
        for (name, f, fh), (_, g, gh) in zip(fv, gv):
            want_f, want_g = nat.block_fields(M, N, blk, fh, gh)
            s.set_rhs_device(f.data_ptr(), *f.stride(), f.dtype == torch.float32, stream())
            s.set_w0_device(g.data_ptr(), *g.stride(), g.dtype == torch.float32, stream())
            got_f, got_g = s.user_plane(0), s.user_plane(1)
            assert got_f.shape == (blk.nx, blk.ny) and got_g.shape == (blk.nx + 2, blk.ny + 2)
            assert np.array_equal(got_f, want_f), (name, r)
            assert np.array_equal(got_g, want_g), (name, r)
        s.set_rhs_device(0, 0, 0, False, 0)  # a null pointer clears
        assert s.user_plane(0) is None and not s.user_rhs and s.user_w0


# ---- 2. full solves against the host path ---------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "three-step", "two-step", "fused", "classic"])
@pytest.mark.parametrize("M,N", sorted(fc.COUNTS))
def test_full_solves_equal_the_host_path(gpu, M, N, algo):
    prob = EllipseProblem(M, N)
    f, g = fc.rhs(M, N), fc.w0(M, N)
    fd, gd = cuda(f), cuda(g)
    for warm in (False, True):
        host = solve(prob, backend="hip", algo=algo, rhs=f, w0=g if warm else None, return_w=True)
        dev = solve(prob, backend="hip", algo=algo, rhs=fd, w0=gd if warm else None, return_w="device")
        tag = f"{M}x{N} {dev.algo} {'w0' if warm else 'zero'}"
        assert dev.converged and dev.iters == fc.COUNTS[(M, N)][warm], (tag, dev.iters)
        assert dev.init == ("field" if warm else "zero") and dev.w_origin is None
        assert tuple(dev.w.shape) == (M - 1, N - 1)
        same_report(dev, host, tag)


# ---- 3. the tie to the built-in path --------------------------------------------------------------
@pytest.mark.parametrize("algo,M,N", [("three-step", 10, 50), ("fused", 10, 126)])
def test_expanded_constant_is_the_builtin_path(gpu, algo, M, N, monkeypatch):
    """rhs ≡ F as a stride-(0, 0) expanded tensor and w0 ≡ 0 on the device
    against no fields at all: the same bits."""
    if algo == "fused":
        monkeypatch.setenv("PE_RESIDENT", "0")
    prob = EllipseProblem(M, N)
    F = torch.tensor(prob.F, dtype=torch.float64, device="cuda:0").expand(M - 1, N - 1)
    Z = torch.zeros(M - 1, N - 1, dtype=torch.float64, device="cuda:0")
    assert F.stride() == (0, 0)
    a = solve(prob, backend="hip", algo=algo, return_w=True)
    b = solve(prob, backend="hip", algo=algo, rhs=F, w0=Z, return_w="device")
    assert a.algo == b.algo == algo and a.converged
    assert (a.iters, a.last_diff, a.res_true, a.b_norm) == (b.iters, b.last_diff, b.res_true, b.b_norm)
    assert torch.equal(b.w.cpu(), torch.from_numpy(a.w))


# ---- 4. virtual ranks -----------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_virtual_ranks_equal_the_host_path(gpu, M, N, ranks, decomp):
    """Every block slices its part of the one global tensor and gathers into
    its position of one global tensor."""
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    kw = dict(backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False)
    f, g = fc.rhs(M, N), fc.w0(M, N)
    host = solve(prob, rhs=f, w0=g, return_w=True, **kw)
    dev = solve(prob, rhs=cuda(f), w0=cuda(g), return_w="device", **kw)
    assert f"{dev.Px}x{dev.Py}" == decomp and dev.iters == 9 and not dev.converged
    same_report(dev, host, decomp)
    mixed = solve(prob, rhs=cuda(f), w0=g, return_w=True, **kw)  # a device and a host field, w on the host
    assert isinstance(mixed.w, np.ndarray) and np.array_equal(mixed.w, host.w)


# ---- 5. session -----------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
def test_session_equals_fresh_solves(gpu, flip):
    """One kept solver, fields set / replaced / cleared, host and device
    operands alternating: every solve equals a fresh solve() bit for bit and
    only the first one reports a construction time."""
    M = N = 40
    prob = EllipseProblem(M, N)
    f, g = fc.rhs(M, N), fc.w0(M, N)
    steps = [(f, None), (2.0 * f, g), (None, None)]
    n_op = flip
    with DeviceSession(prob) as session:
        for n, (a, b) in enumerate(steps):
            ops = []
            for v in (a, b):  # operands alternate between the device and the host
                ops.append(v if v is None or n_op % 2 else cuda(v))
                n_op += v is not None
            dev_w = (n + flip) % 2 == 0
            rep = session.solve(rhs=ops[0], w0=ops[1], return_w="device" if dev_w else True)
            ref = solve(prob, backend="hip", rhs=a, w0=b, return_w=True)
            assert rep.converged and (rep.timers["construct"] == 0) == (n > 0) and ref.timers["construct"] > 0
            assert (rep.l2_err == -1.0) == (a is not None)
            if dev_w:
                same_report(rep, ref, n)
            else:
                for k in SAME:
                    assert getattr(rep, k) == getattr(ref, k), (n, k)
                assert np.array_equal(rep.w, ref.w), n
        assert rep.iters == 50 and rep.init == "zero"
        assert session.solver.user_plane(0) is None and session.solver.user_plane(1) is None
    assert session.solver is None
    with pytest.raises(RuntimeError):
        session.solve()


def test_session_continuation_on_the_device(gpu):
    """w0 = the previous report's w, the tensor itself, against the same
    continuation through host arrays."""
    M = N = 40
    prob = EllipseProblem(M, N)
    f = fc.rhs(M, N)
    f2 = 1.01 * f
    with DeviceSession(prob) as session:
        d1 = session.solve(rhs=cuda(f), return_w="device")
        d2 = session.solve(rhs=cuda(f2), w0=d1.w, return_w="device")
    h1 = solve(prob, backend="hip", rhs=f, return_w=True)
    h2 = solve(prob, backend="hip", rhs=f2, w0=h1.w, return_w=True)
    same_report(d1, h1, "first")
    same_report(d2, h2, "continuation")
    assert d2.init == "field" and d2.iters < d1.iters


# ---- 6. stream ordering ---------------------------------------------------------------------------
def delay(ms=20.0):
    """Roughly `ms` of work on the current stream."""
    rate = getattr(torch.cuda.get_device_properties(0), "clock_rate", 0)  # kHz
    if hasattr(torch.cuda, "_sleep") and rate:
        torch.cuda._sleep(int(ms * rate))
        return
    x = torch.ones(1 << 26, dtype=torch.float32, device="cuda:0")  # 256 MB: ≥ 0.1 ms per pass
    for _ in range(int(ms * 10)):
        x.mul_(1.0001)


def test_producer_and_consumer_ordering(gpu, nat):
    """The tensor is produced on a side stream behind a delay and handed over
    at once: the solver stream must wait for the producer (without the event
    wait it slices the zeros), and the producer for the slice (the tensor is
    overwritten right after the call).  set_rhs_device is called directly —
    solve() runs torch.isfinite over the tensor first, which waits for the
    producer on the host and would hide a missing event wait.  (Measured on
    an MI355X: the delay is 15 ms, and a stream that reads the tensor without
    waiting for the producer sees the zeros.)"""
    M = N = 40
    prob = EllipseProblem(M, N)
    f = fc.rhs(M, N)
    host = solve(prob, backend="hip", rhs=f, return_w=True)
    fd = cuda(f)
    torch.cuda.synchronize()
    blk = D.block(M, N, 1, 0)
    s = nat.DeviceSolver(prob.to_native(), blk, None, nat.SolveOptions())
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        rhs = torch.zeros(M - 1, N - 1, dtype=torch.float64, device="cuda:0")
        delay()
        rhs.copy_(fd, non_blocking=True)
        s.set_rhs_device(rhs.data_ptr(), *rhs.stride(), False, torch.cuda.current_stream().cuda_stream)
        rhs.fill_(-3.0)  # stream order: after the slice
    res = s.solve()
    side.synchronize()
    assert np.array_equal(s.user_plane(0), f)
    assert (res.iters, res.last_diff, res.res_true, res.b_norm) == (host.iters, host.last_diff, host.res_true,
                                                                      host.b_norm)
    # the consumer side: w is used on the current stream with no synchronise in between.  (At this size the
    # gather is over long before the host enqueues the next operation, so a missing consumer wait would not
    # reliably show; this exercises the path.)
    w = torch.empty(M - 1, N - 1, dtype=torch.float64, device="cuda:0")
    s.copy_w_device(w.data_ptr(), *w.stride(), 0, 0, stream())
    twice = w * 2.0
    assert torch.equal(twice.cpu(), torch.from_numpy(host.w * 2.0))
    # and through solve(), on the side stream
    with torch.cuda.stream(side):
        rhs = torch.zeros(M - 1, N - 1, dtype=torch.float64, device="cuda:0")
        delay()
        rhs.copy_(fd, non_blocking=True)
        rep = solve(prob, backend="hip", rhs=rhs, return_w="device")
        rhs.fill_(-3.0)
        twice = rep.w * 2.0
    assert torch.equal(twice.cpu(), torch.from_numpy(host.w * 2.0))
    same_report(rep, host, "side stream")


# ---- 7. refusals ----------------------------------------------------------------------------------
def test_refusals(gpu, nat):
    M = N = 40
    prob = EllipseProblem(M, N)
    f = fc.rhs(M, N)
    nan = cuda(f).clone()
    nan[17, 23] = float("nan")
    bad = [torch.zeros(M - 1, N, dtype=torch.float64, device="cuda:0"),
           torch.zeros(M - 1, N - 1, dtype=torch.int64, device="cuda:0"),
           torch.zeros(M - 1, N - 1, dtype=torch.float16, device="cuda:0"),
           torch.zeros(M - 1, N - 1, dtype=torch.complex128, device="cuda:0"),
           nan]
    for t in bad:
        for backend, kw in (("hip", {}), ("hip-group", dict(ranks=4, decomp="2x2"))):
            with pytest.raises(ValueError, match="rhs"):
                solve(prob, backend=backend, rhs=t, **kw)
            with pytest.raises(ValueError, match="w0"):
                solve(prob, backend=backend, w0=t, **kw)
    with DeviceSession(prob) as session:
        session.solve(rhs=cuda(f), w0=fc.w0(M, N))
        before = session.solver.user_plane(0).copy(), session.solver.user_plane(1).copy()
        for t in bad:
            with pytest.raises(ValueError, match="rhs"):
                session.solve(rhs=t)
            with pytest.raises(ValueError, match="w0"):
                session.solve(rhs=cuda(2.0 * f), w0=t)  # (nothing is set before everything is checked)
        # a host pointer handed to the solver directly never reaches a kernel
        a = np.ascontiguousarray(f)
        for call in (session.solver.set_rhs_device, session.solver.set_w0_device):
            with pytest.raises(ValueError, match="device"):
                call(a.ctypes.data, N - 1, 1, False, stream())
        with pytest.raises(ValueError, match="device"):
            session.solver.copy_w_device(a.ctypes.data, N - 1, 1, 0, 0, stream())
        small = torch.zeros(M - 1, dtype=torch.float64, device="cuda:0")  # strides that leave the allocation
        with pytest.raises(ValueError):
            session.solver.set_rhs_device(small.data_ptr(), 1 << 40, 1, False, stream())
        assert np.array_equal(session.solver.user_plane(0), before[0])
        assert np.array_equal(session.solver.user_plane(1), before[1])
    with pytest.raises(ValueError, match="return_w"):
        solve(prob, backend="hip", return_w="gpu")


# ---- 8. two processes on one GPU ------------------------------------------------------------------
def test_two_processes_with_device_fields(gpu, tmp_path, monkeypatch):
    """Row slabs of 37×50 over the host-staged transport: every rank loads the
    same arrays onto its device, checks its planes against block_fields, solves
    with return_w="device" and saves its block with w_origin
    (device_fields_job.py).  Assembled here: the single-rank solve's count, w
    within 1e-10·max|w| of it (test_two_processes_with_fields' bound)."""
    from conftest import free_port

    M, N = 37, 50
    f, g = str(tmp_path / "f.npy"), str(tmp_path / "g.npy")
    np.save(f, fc.rhs(M, N))
    np.save(g, fc.w0(M, N))
    env = dict(os.environ, PE_COMM="host", PE_HALO="exchange", PE_OVERLAP="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "device_fields_job.py"),
           str(M), str(N), f, g, str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    w = np.full((M - 1, N - 1), np.nan)
    metas = []
    for r in range(2):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d = json.load(fh)
        blk = np.load(tmp_path / f"out.r{r}.npy")
        i0, j0 = d["w_origin"]
        assert d["planes_equal"] and d["ranks"] == 2 and d["Px"] == 2 and d["Py"] == 1 and d["converged"]
        assert d["init"] == "field" and d["l2_err"] == -1.0 and d["w_is_cuda"]
        w[i0 - 1:i0 - 1 + blk.shape[0], j0 - 1:j0 - 1 + blk.shape[1]] = blk
        metas.append(d)
    assert np.isfinite(w).all() and metas[0]["w_origin"] == [1, 1] and metas[1]["w_origin"][1] == 1
    assert metas[0]["iters"] == metas[1]["iters"] and metas[0]["algo"] == metas[1]["algo"]
    monkeypatch.setenv("PE_RESIDENT", "0")  # (the single-rank solve on the job's streaming sweep)
    one = solve(EllipseProblem(M, N), backend="hip", algo=metas[0]["algo"], rhs=fc.rhs(M, N), w0=fc.w0(M, N),
                return_w=True)
    dev = float(np.abs(w - one.w).max() / np.abs(one.w).max())
    print(f"device-field-two-process algo={metas[0]['algo']} iters={metas[0]['iters']} (one rank {one.iters}) "
          f"w_rel={dev:.2e}")
    assert one.algo == metas[0]["algo"] and metas[0]["iters"] == one.iters
    assert dev <= 1e-10
