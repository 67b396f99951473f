"""MI355X tests of the solution's gradient on the device paths
(DeviceSolver.gradient / gradient_device, kGradField, solve(return_grad=),
DeviceSession, the virtual-rank group driver, a two-process job): the kernel
reading w with its ring in every live layout (classic, single-, two- and
three-step planes, after a resident launch), strided destinations, block seams.

Inputs: field_checks.rhs and w0 (asymmetric, w0 non-zero outside the ellipse)
and nine iterations where "far from convergence" is meant, so that a wrong
halo or mask is not yet healed.  The comparison (grad_checks.check_report):
gx, gy and grad_max bit for bit, energy to rel 1e-12, integral to abs
1e-12·h1·h2·Σ_D|w|, against fp64 numpy from the report's own w.  Every test
takes seconds, and fails without the feature (no return_grad, no
DeviceSolver.gradient)."""

import json
import os
import subprocess
import sys

import field_checks as fc
import grad_checks as gc
import numpy as np
import pytest
import torch
from test_device_fields_gpu import cuda, stream
from test_gradient import tie

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_figures(a, b):
    return (a.integral, a.energy, a.grad_max) == (b.integral, b.energy, b.grad_max)


# ---- 1. every layout, far from convergence ------------------------------------------------------
@pytest.mark.parametrize("algo,M,N,variant,want", [
    ("three-step", 10, 50, 0, "three-step"),   # a second strip with one output column
    ("three-step", 66, 49, 0, "three-step"),   # a 17-row last item; nine row tiles, the last of one row
    ("two-step", 10, 122, 0, "two-step"),
    ("fused", 10, 126, 0, "fused"),            # (the streaming single sweep: PE_RESIDENT=0)
    ("auto", 34, 250, 0, "resident"),
    ("classic", 10, 50, 0, "classic"),
    ("classic", 10, 50, 1, "classic")])
def test_every_layout_far_from_convergence(gpu, algo, M, N, variant, want, monkeypatch):
    if algo == "fused":
        monkeypatch.setenv("PE_RESIDENT", "0")
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    kw = dict(backend="hip", algo=algo, variant=variant, rhs=fc.rhs(M, N), w0=fc.w0(M, N))
    base = solve(prob, return_w=True, **kw)
    host = solve(prob, return_w=True, return_grad=True, **kw)
    dev = solve(prob, return_w="device", return_grad="device", **kw)
    stats = solve(prob, return_grad="stats", **kw)
    tag = f"{want} v{variant} {M}x{N}"
    assert host.algo == want and host.iters >= 9 and not host.converged, (tag, host.algo, host.iters)
    for rep, how in ((host, "host"), (dev, "device")):
        gc.same_solve(f"{tag} {how}", rep, base)
        gc.check_report(f"{tag} {how}", prob, rep)
    assert isinstance(host.grad, np.ndarray) and isinstance(dev.grad, torch.Tensor) and dev.grad.is_cuda
    assert tuple(dev.grad.shape) == (2, M - 1, N - 1) and dev.grad.dtype == torch.float64 and dev.w_origin is None
    assert np.array_equal(dev.grad.cpu().numpy(), host.grad) and same_figures(dev, host)
    assert stats.grad is None and stats.w is None and same_figures(stats, host)


# ---- 2. full solves, the analytic tie -----------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "three-step", "two-step", "fused", "classic"])
def test_full_solves(gpu, algo):
    M = N = 40
    prob = EllipseProblem(M, N)
    kw = dict(backend="hip", algo=algo, rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    base = solve(prob, **kw)
    rep = solve(prob, return_grad=True, **kw)
    assert rep.converged and rep.iters == fc.COUNTS[(M, N)][1], (rep.algo, rep.iters)
    gc.same_solve(rep.algo, rep, base)
    gc.check_report(f"full {rep.algo}", prob, rep)


def test_analytic_tie_on_the_device(gpu):
    """test_gradient.test_analytic_tie's bounds on the hip backend (F = 1, zero init)."""
    a = tie(solve(EllipseProblem(40, 40), backend="hip", return_grad="stats"))
    b = tie(solve(EllipseProblem(200, 200), backend="hip", return_grad="stats"))
    print(f"grad-tie hip 40x40 {a[0]:.3e} {a[1]:.3e}  200x200 {b[0]:.3e} {b[1]:.3e}")
    assert a[0] <= 6e-2 and a[1] <= 3e-2
    assert b[0] <= 1.3e-2 and b[1] <= 3e-4
    assert b[0] < a[0] and b[1] < a[1]


# ---- 3. the native entry points -----------------------------------------------------------------
def solved(nat, M, N, algo=0, fam=None):
    prob = EllipseProblem(M, N, **(fam or {}))
    prob.max_iter = 9
    opt = nat.SolveOptions()
    opt.algo = algo
    s = nat.DeviceSolver(prob.to_native(), D.block(M, N, 1, 0), None, opt)
    f = np.ascontiguousarray(fc.rhs(M, N)) if fam is None else None
    g = np.ascontiguousarray(fc.w0(M, N)) if fam is None else gc.random_w(prob)
    fl, gl = nat.block_fields(M, N, s.block, f, g)
    s.set_rhs(fl)
    s.set_w0(gl)
    s.solve()
    return prob, s


@pytest.mark.parametrize("M,N,algo", [(10, 50, 0), (10, 300, 0), (10, 50, 1)])
def test_strided_destinations(gpu, nat, M, N, algo):
    """gradient_device into a dense pair, a transposed view and a window of a
    larger sentinel-filled tensor (nothing outside the window changes); the
    functionals alone (STORE = false) are the same three numbers.  10×300: two
    column tiles, the second with idle lanes."""
    prob, s = solved(nat, M, N, algo)
    w = np.array(s.w())
    stats, gx, gy = s.gradient()
    gc.check_values(f"native host {M}x{N} algo {algo}", prob, w, np.stack((gx, gy)), *stats)
    s.solve()
    assert s.gradient(False) == (stats, None, None)
    s.solve()
    assert s.gradient_device(0, 0, 0, 0, 0, 0, 0) == stats
    nx, ny = M - 1, N - 1
    # transposed: element (i, j) at [j, i]
    tx, ty = (torch.full((ny, nx), -7.0, dtype=torch.float64, device="cuda:0") for _ in range(2))
    s.solve()
    assert s.gradient_device(tx.data_ptr(), ty.data_ptr(), 1, nx, 0, 0, stream()) == stats
    assert np.array_equal(tx.cpu().numpy().T, gx) and np.array_equal(ty.cpu().numpy().T, gy)
    # a window at (3, 5) of a larger tensor, the sentinel everywhere else
    big = torch.full((2, nx + 7, ny + 9), -7.0, dtype=torch.float64, device="cuda:0")
    s.solve()
    assert s.gradient_device(big[0].data_ptr(), big[1].data_ptr(), big.stride(1), big.stride(2), 3, 5, stream()) == stats
    b = big.cpu().numpy()
    assert np.array_equal(b[0, 3:3 + nx, 5:5 + ny], gx) and np.array_equal(b[1, 3:3 + nx, 5:5 + ny], gy)
    b[:, 3:3 + nx, 5:5 + ny] = -7.0
    assert (b == -7.0).all()


def test_neither_class_on_the_device(gpu, nat):
    """The 12×12 member with cx = cy = 30 (isolated inside nodes), a random w0."""
    prob, s = solved(nat, 12, 12, 0, dict(cx=30.0, cy=30.0))
    counts = gc.class_counts(prob)
    assert all(counts[(d, k)] > 0 for d in "xy" for k in range(4))
    w = np.array(s.w())
    stats, gx, gy = s.gradient()
    gc.check_values("tiny 12x12", prob, w, np.stack((gx, gy)), *stats)


def test_native_refusals(gpu, nat):
    prob, s = solved(nat, 10, 50)
    nx, ny = 9, 49
    host = np.zeros((2, nx, ny))
    with pytest.raises(ValueError, match="device"):  # a host pointer never reaches a kernel
        s.gradient_device(host[0].ctypes.data, host[1].ctypes.data, ny, 1, 0, 0, stream())
    small = torch.zeros(2 * nx, dtype=torch.float64, device="cuda:0")
    with pytest.raises(ValueError):  # strides that leave the allocation
        s.gradient_device(small.data_ptr(), small.data_ptr(), 1 << 40, 1, 0, 0, stream())
    ok = torch.zeros((nx, ny), dtype=torch.float64, device="cuda:0")
    with pytest.raises(ValueError):  # the second destination is checked as well
        s.gradient_device(ok.data_ptr(), host[1].ctypes.data, ny, 1, 0, 0, stream())
    with pytest.raises(ValueError):
        s.gradient_device(ok.data_ptr(), 0, ny, 1, 0, 0, stream())
    with pytest.raises(ValueError):
        s.gradient_device(ok.data_ptr(), ok.data_ptr(), -1, 1, 0, 0, stream())
    s.run_iterations(3, False)  # nothing was launched by a refused call: the state is intact
    s.synchronize()
    s.gradient(False)
    with pytest.raises(RuntimeError, match="reset"):  # the pass used an iteration plane as scratch
        s.run_iterations(3, False)
    s.reset()
    s.run_iterations(3, False)
    s.synchronize()
    assert s.state()["iter"] == 3


# ---- 4. virtual ranks ---------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "classic"])
@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_virtual_ranks(gpu, M, N, ranks, decomp, algo):
    """Every block's kernel writes its position; a missing halo shows at the seams."""
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    kw = dict(backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False, algo=algo, rhs=fc.rhs(M, N),
              w0=fc.w0(M, N))
    base = solve(prob, return_w=True, **kw)
    host = solve(prob, return_w=True, return_grad=True, **kw)
    dev = solve(prob, return_w="device", return_grad="device", rhs=cuda(fc.rhs(M, N)),
                **{k: v for k, v in kw.items() if k != "rhs"})
    stats = solve(prob, return_grad="stats", **kw)
    assert f"{host.Px}x{host.Py}" == decomp and host.iters == 9 and not host.converged
    for rep, how in ((host, "host"), (dev, "device")):
        gc.same_solve(f"{decomp} {algo} {how}", rep, base)
        gc.check_report(f"group {M}x{N} {decomp} {algo} {how}", prob, rep)
    assert isinstance(dev.grad, torch.Tensor) and dev.grad.is_cuda and tuple(dev.grad.shape) == (2, M - 1, N - 1)
    assert np.array_equal(dev.grad.cpu().numpy(), host.grad) and same_figures(dev, host)
    assert stats.grad is None and same_figures(stats, host)


# ---- 5. two processes on one GPU ----------------------------------------------------------------
def test_two_processes(gpu, tmp_path):
    """Row slabs of 37×50 over the host-staged transport (gradient_job.py):
    each rank returns its blocks on its device; the assembled gradient is the
    recompute on the assembled w, and both ranks report the job's figures."""
    from conftest import free_port

    M, N = 37, 50
    paths = [str(tmp_path / n) for n in ("f.npy", "g.npy")]
    for p, a in zip(paths, (fc.rhs(M, N), fc.w0(M, N))):
        np.save(p, a)
    env = dict(os.environ, PE_COMM="host", PE_HALO="exchange", PE_OVERLAP="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "gradient_job.py"),
           "hip", str(M), str(N), "9", *paths, str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    w = np.full((M - 1, N - 1), np.nan)
    g = np.full((2, M - 1, N - 1), np.nan)
    d = []
    for r in range(2):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d.append(json.load(fh))
        bw, bg = np.load(tmp_path / f"out.r{r}.w.npy"), np.load(tmp_path / f"out.r{r}.g.npy")
        i0, j0 = d[r]["w_origin"]
        w[i0 - 1:i0 - 1 + bw.shape[0], j0 - 1:j0 - 1 + bw.shape[1]] = bw
        g[:, i0 - 1:i0 - 1 + bw.shape[0], j0 - 1:j0 - 1 + bw.shape[1]] = bg
        assert d[r]["ranks"] == 2 and (d[r]["Px"], d[r]["Py"]) == (2, 1) and d[r]["iters"] >= 9
    assert np.isfinite(w).all() and np.isfinite(g).all() and not d[0]["converged"]
    for k in ("integral", "energy", "grad_max", "iters"):
        assert d[0][k] == d[1][k], k
    gc.check_values(f"two-process {d[0]['algo']}", EllipseProblem(M, N), w, g, d[0]["integral"], d[0]["energy"],
                    d[0]["grad_max"])


# ---- 6. session ---------------------------------------------------------------------------------
def test_session_sequence(gpu):
    """grad, no grad, stats, grad with a new rhs on one kept solver: each step a fresh solve()'s."""
    M = N = 40
    prob = EllipseProblem(M, N)
    f = fc.rhs(M, N)
    steps = [(f, True), (f, False), (f, "stats"), (2.0 * f, "device")]
    with DeviceSession(prob) as session:
        for n, (a, how) in enumerate(steps):
            rep = session.solve(rhs=cuda(a) if n % 2 else a, return_w=True, return_grad=how)
            ref = solve(prob, backend="hip", rhs=a, return_w=True, return_grad=how)
            assert rep.converged and (rep.timers["construct"] == 0) == (n > 0) and ref.timers["construct"] > 0
            assert np.array_equal(rep.w, ref.w) and rep.iters == ref.iters and same_figures(rep, ref), n
            if how is False:
                assert rep.grad is None and rep.integral == rep.energy == rep.grad_max == -1.0
            elif how == "stats":
                assert rep.grad is None
                gc.check_stats(f"session step {n}", prob, rep.w, rep.integral, rep.energy, rep.grad_max)
            else:
                assert np.array_equal(gc.host(rep.grad), gc.host(ref.grad)), n
                gc.check_report(f"session step {n}", prob, rep)
