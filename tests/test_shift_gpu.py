"""MI355X tests of the shifted operator A + σI (EllipseProblem.shift): the
operator pass (kApplyField's SHIFT instantiations), the classic two-kernel solve
(kInit / kInitField / kF / kG with SHIFT) on one rank, on virtual ranks and on
processes, the refusals.  Inputs, shapes and bounds: shift_checks.  Whether a
device field equals the host's bit for bit is printed, not asserted.  Every test
takes seconds and fails without the feature (EllipseProblem has no `shift`).

A solver for a shifted problem is always on the classic layout — the
single-sweep layouts refuse the shift at construction (test_algo_refusals) — so
the operator pass with a shift runs on the classic layout under both `algo`
values that reach it and both arithmetic variants; the pass on a three-step
layout exists only unshifted (test_operator_gpu.test_every_layout)."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import operator_checks as oc
import pytest
import shift_checks as sc
import torch
from test_device_fields_gpu import cuda

import poisson_ellipse_openmp_mpi_cuda_amd as pe
from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


# ---- 3. the operator pass -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("M,N,kw", sc.SHAPES, ids=sc.IDS)
def test_operator_pass(gpu, M, N, kw, sigma):
    """float64, float32 and a strided tensor; out= host, device and sum; apply, residual with F and with a user rhs."""
    prob = sc.problem(M, N, kw, sigma)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    t = cuda(v)
    big = torch.full((N + 4, M + 2), -7.0, dtype=torch.float64, device="cuda:0")
    big[3:3 + N - 1, 1:M] = t.T
    forms = [("host", v, False), ("f64", t, False), ("transposed", big[3:3 + N - 1, 1:M].T, False),
             ("f32", t.to(torch.float32), True)]
    assert not forms[2][1].is_contiguous()
    with DeviceSession(prob) as s:
        for resid, user in ((False, False), (True, False), (True, True)):
            first = {}
            for name, x, f32 in forms:
                extra = dict(rhs=cuda(f) if user else None) if resid else {}
                call = s.residual if resid else s.apply
                h, d, only = call(x, out="host", **extra), call(x, out="device", **extra), call(x, out="sum", **extra)
                sc.compare(f"{M}x{N} {name}", prob, h.field, h.sum, resid, user, f32)
                assert isinstance(d.field, torch.Tensor) and d.field.is_cuda and tuple(d.field.shape) == (M - 1, N - 1)
                assert np.array_equal(host(d.field), h.field) and d.sum == h.sum == only.sum and only.field is None
                ref = first.setdefault(f32, (h.field, h.sum))  # the same values: identical bits whatever the form
                assert np.array_equal(h.field, ref[0]) and h.sum == ref[1], name
    one = pe.apply_operator(prob, v, backend="hip")
    sc.compare(f"{M}x{N} one-shot", prob, one.field, one.sum)


@pytest.mark.parametrize("algo,variant", [("auto", 0), ("auto", 1), ("classic", 0), ("classic", 1)])
def test_operator_pass_on_the_classic_layout(gpu, algo, variant):
    """The pass reads only tables: before a solve, after one and after a gradient pass the same bits."""
    M, N, sigma = 10, 50, 40.0
    prob = sc.problem(M, N, None, sigma, max_iter=9)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    vt = cuda(v)
    with DeviceSession(prob, algo=algo, variant=variant) as s:
        def both():
            a, r = s.apply(vt), s.residual(vt, rhs=f)
            return a.field, a.sum, r.field, r.sum

        before = both()
        rep = s.solve(rhs=f, w0=v)
        assert rep.algo == "classic" and rep.iters == 9 and not rep.converged
        after = both()
        s.solve(rhs=f, w0=v, return_grad="stats")
        after_grad = both()
    sc.compare(f"classic v{variant}", prob, before[0], before[1])
    sc.compare(f"classic v{variant}", prob, before[2], before[3], True, True)
    for other in (after, after_grad):
        assert np.array_equal(other[0], before[0]) and np.array_equal(other[2], before[2])
        assert other[1] == before[1] and other[3] == before[3]


# ---- 4. device solves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("M,N,kw", sc.SHAPES, ids=sc.IDS)
def test_solve_against_serial(gpu, M, N, kw, sigma, variant):
    prob = sc.problem(M, N, kw, sigma)
    ref = sc.stop_margin(prob)
    rep = solve(prob, backend="hip", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True, variant=variant)
    print(f"shift-hip {M}x{N} shift={sigma} v{variant} iters={rep.iters}/{ref.iters} dw={np.abs(rep.w - ref.w).max():.2e} "
          f"algo={rep.algo}")
    assert rep.algo == "classic" and rep.converged and rep.iters == ref.iters
    assert np.abs(rep.w - ref.w).max() <= 1e-10
    assert rep.l2_err == -1.0 and rep.max_err == -1.0
    assert rep.res_true == -1.0 and rep.res_rec == -1.0 and rep.res_gap == -1.0
    assert rep.to_dict()["shift"] == sigma


@pytest.mark.parametrize("sigma", sc.SIGMAS)
def test_builtin_rhs_and_exact(gpu, sigma):
    """F and the zero start (kInit), and a user rhs + w0 + exact: the error is numpy's from the returned w."""
    M, N = 70, 129
    prob = sc.problem(M, N, None, sigma)
    ref = sc.stop_margin(prob, fields=False)
    rep = solve(prob, backend="hip", return_w=True)
    assert rep.algo == "classic" and rep.iters == ref.iters and np.abs(rep.w - ref.w).max() <= 1e-10
    assert rep.l2_err == -1.0 and rep.max_err == -1.0
    u = fc.exact(M, N)
    for fields in (dict(rhs=fc.rhs(M, N), w0=fc.w0(M, N)), dict(rhs=cuda(fc.rhs(M, N)), w0=cuda(fc.w0(M, N)))):
        for exact in (u, cuda(u)):
            got = solve(prob, backend="hip", return_w=True, exact=exact, **fields)
            l2, mx = sc.errors_from_w(prob, got.w, u)
            print(f"shift-exact {M}x{N} shift={sigma} l2={got.l2_err!r}/{l2!r} max={got.max_err!r}/{mx!r}")
            assert got.iters == sc.serial(prob).iters
            assert got.l2_err == pytest.approx(l2, rel=1e-12) and got.max_err == pytest.approx(mx, rel=1e-12)


@pytest.mark.parametrize("variant", [0, 1])
def test_iteration_cap(gpu, variant):
    M, N, sigma = 65, 258, 0.75
    prob = sc.problem(M, N, None, sigma, max_iter=7)
    a = solve(prob, backend="serial", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    b = solve(prob, backend="hip", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True, variant=variant)
    assert a.iters == b.iters == 7 and not a.converged and not b.converged and b.algo == "classic"
    assert np.abs(a.w - b.w).max() <= 1e-9 * np.abs(a.w).max()


def test_implicit_euler_steps_in_a_session(gpu):
    """Three steps of u' = Δu + f, (A + I/dt) u⁺ = u/dt + f, GPU tensors in and out of one session."""
    M, N, dt = 40, 40, 1.0 / 40.0
    prob = sc.problem(M, N, None, 1.0 / dt)
    f = fc.rhs(M, N)
    u_host = fc.w0(M, N)
    u, ft = cuda(u_host), cuda(f)
    with DeviceSession(prob) as s:
        for step in range(3):
            ref = solve(prob, backend="serial", rhs=u_host / dt + f, w0=u_host, return_w=True, keep_history=True)
            for d in ref.history[-2:]:  # (the step's stop test is no coin toss)
                assert abs(d - prob.tol) > 1e-3 * prob.tol, (step, ref.history[-2:])
            rep = s.solve(rhs=u / dt + ft, w0=u, return_w="device")
            assert isinstance(rep.w, torch.Tensor) and rep.w.is_cuda and rep.algo == "classic"
            dev = float(np.abs(host(rep.w) - ref.w).max())
            print(f"shift-heat step {step} iters={rep.iters}/{ref.iters} dw={dev:.2e}")
            assert rep.converged and rep.iters == ref.iters and dev <= 1e-10
            u, u_host = rep.w, ref.w


@pytest.mark.parametrize("variant", [0, 1])
def test_explicit_zero_shift_is_the_default(gpu, variant):
    M, N = 40, 40
    kw = dict(backend="hip", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True, variant=variant)
    a, b = solve(EllipseProblem(M, N), **kw), solve(EllipseProblem(M, N, shift=0.0), **kw)
    assert a.algo == b.algo != "" and a.iters == b.iters and np.array_equal(a.w, b.w) and a.last_diff == b.last_diff
    assert "shift" not in b.to_dict()
    c = solve(EllipseProblem(M, N), **dict(kw, algo="classic"))
    d = solve(EllipseProblem(M, N, shift=0.0), **dict(kw, algo="classic"))
    assert c.algo == d.algo == "classic" and c.iters == d.iters and np.array_equal(c.w, d.w)
    x = pe.apply_operator(EllipseProblem(M, N, shift=0.0), fc.w0(M, N), backend="hip")
    oc.compare("zero shift", EllipseProblem(M, N), x.field, x.sum)


# ---- 5. several ranks ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", sc.SIGMAS)
@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (37, 50, 3, "3x1")])
def test_virtual_ranks(gpu, M, N, ranks, decomp, sigma):
    prob = sc.problem(M, N, None, sigma)
    f, g = fc.rhs(M, N), fc.w0(M, N)
    one = solve(prob, backend="hip", rhs=f, w0=g, return_w=True)
    rep = solve(prob, backend="hip-group", ranks=ranks, decomp=decomp, rhs=f, w0=g, return_w=True)
    print(f"shift-group {decomp} {M}x{N} shift={sigma} iters={rep.iters}/{one.iters} dw={np.abs(rep.w - one.w).max():.2e}")
    assert rep.algo == one.algo == "classic" and rep.converged and abs(rep.iters - one.iters) <= 1
    assert np.abs(rep.w - one.w).max() <= 1e-9 and rep.l2_err == -1.0
    a = pe.apply_operator(prob, cuda(g), backend="hip-group", ranks=ranks, decomp=decomp, out="device")
    r = pe.residual(prob, g, rhs=f, backend="hip-group", ranks=ranks, decomp=decomp)
    sc.compare(f"group {decomp}", prob, host(a.field), a.sum)
    sc.compare(f"group {decomp}", prob, r.field, r.sum, True, True)


def test_processes_on_one_gpu(gpu, tmp_path):
    """Three processes, row slabs, the host-staged transport, on one GPU (shift_job.py) against serial."""
    from conftest import free_port

    M, N, world, sigma = 37, 50, 3, 40.0
    prob = sc.problem(M, N, None, sigma)
    ref = sc.stop_margin(prob)
    paths = [str(tmp_path / n) for n in ("f.npy", "g.npy")]
    for p, a in zip(paths, (fc.rhs(M, N), fc.w0(M, N))):
        np.save(p, a)
    env = dict(os.environ, PE_COMM="host", PE_HALO="exchange", PE_OVERLAP="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "shift_job.py"), str(M), str(N), repr(sigma), *paths, str(tmp_path / "out"), "rows"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    W = np.full((M - 1, N - 1), np.nan)
    for r in range(world):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d = json.load(fh)
        blk = np.load(tmp_path / f"out.r{r}.npy")
        i0, j0 = d["origin"]
        W[i0 - 1:i0 - 1 + blk.shape[0], j0 - 1:j0 - 1 + blk.shape[1]] = blk
        assert d["algo"] == "classic" and d["converged"] and d["iters"] == ref.iters and d["shift"] == sigma
        assert d["Px"] == world and d["Py"] == 1 and d["l2_err"] == -1.0
    print(f"shift-processes {M}x{N} shift={sigma} dw={np.abs(W - ref.w).max():.2e}")
    assert np.abs(W - ref.w).max() <= 1e-10


# ---- 6. refusals --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["fused", "two-step", "three-step"])
def test_algo_refusals(gpu, algo):
    """The single-sweep kernels do not carry the shift: ValueError at construction, before any kernel."""
    M, N = 40, 40
    prob = sc.problem(M, N, None, 0.75)
    with pytest.raises(ValueError, match="shift"):
        DeviceSession(prob, algo=algo)
    with pytest.raises(ValueError, match="shift"):
        solve(prob, backend="hip", algo=algo)
    with pytest.raises(ValueError, match="shift"):
        solve(prob, backend="hip-group", ranks=4, decomp="2x2", algo=algo)
    with pytest.raises(ValueError, match="shift"):
        pe.apply_operator(prob, fc.w0(M, N), backend="hip", algo=algo)
    with DeviceSession(EllipseProblem(M, N), algo=algo) as s:  # (unshifted: the layout exists as ever)
        assert s.solve().converged


@pytest.mark.parametrize("bad", [-1.0, float("nan"), float("inf")])
def test_bad_shift_never_reaches_the_device(gpu, bad):
    from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D
    from poisson_ellipse_openmp_mpi_cuda_amd.solver import _options

    P = EllipseProblem(40, 40).to_native()
    P.shift = bad  # (a native Problem filled in by hand: the constructor itself refuses)
    with pytest.raises(ValueError, match="shift"):
        gpu.DeviceSolver(P, D.block(40, 40, 1, 0), None, _options())
    with pytest.raises(ValueError, match="shift"):
        gpu.device_solve_group_grid(P, D.grid(4, 40, 40, "2x2"), _options(), False, None, None, None)
    with pytest.raises(ValueError, match="shift"):
        DeviceSession(EllipseProblem(40, 40, shift=bad))
