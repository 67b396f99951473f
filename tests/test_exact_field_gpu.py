"""MI355X tests of the user exact solution on the device paths
(DeviceSolver.set_exact / set_exact_device, kErrorField, solve(exact=),
DeviceSession): the error pass reading w in every live layout (classic,
single-, two- and three-step planes, after a resident launch), the plane cut
from host arrays and from GPU tensors, the virtual-rank group driver, a kept
session, the tie to kError's analytic error and a two-process job.

Inputs: field_checks.rhs / w0 / exact (asymmetric in x and y).  The comparison
(exact_checks.check_error): l2_err to rel 1e-12 and max_err bit for bit against
fp64 numpy from the report's own w.  Shapes are the smallest at which the
plane, the pitch or the layout can go wrong (test_user_fields_gpu.py's edge
shapes); every test takes seconds.  Every test that passes `exact` fails
without the feature: l2_err stays −1."""

import json
import os
import subprocess
import sys

import exact_checks as xc
import field_checks as fc
import numpy as np
import pytest
import torch
from test_device_fields_gpu import cuda, stream, views

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- 1. every layout, far from convergence ------------------------------------------------------
@pytest.mark.parametrize("algo,M,N,variant,want", [
    ("three-step", 10, 50, 0, "three-step"),   # a second strip with one output column
    ("three-step", 66, 49, 0, "three-step"),   # a 17-row last item
    ("two-step", 10, 122, 0, "two-step"),
    ("fused", 10, 126, 0, "fused"),            # (the streaming single sweep: PE_RESIDENT=0)
    ("auto", 34, 250, 0, "resident"),
    ("classic", 10, 50, 0, "classic"),
    ("classic", 10, 50, 1, "classic")])
def test_every_layout_far_from_convergence(gpu, algo, M, N, variant, want, monkeypatch):
    """Nine iterations from w0: the error is still large, so w read with
    another layout's wpitch, or a plane read with the wrong row length, shows."""
    if algo == "fused":
        monkeypatch.setenv("PE_RESIDENT", "0")
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    kw = dict(backend="hip", algo=algo, variant=variant, rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    base = solve(prob, **kw)
    rep = solve(prob, exact=fc.exact(M, N), **kw)
    tag = f"{want} v{variant} {M}x{N}"
    assert rep.algo == want and rep.iters >= 9 and not rep.converged, (tag, rep.algo, rep.iters)
    assert base.l2_err == -1.0 and base.max_err == -1.0
    xc.same_solve(tag, rep, base)
    xc.check_error(tag, prob, rep, base=base)


# ---- 2. full solves -----------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "three-step", "two-step", "fused", "classic"])
@pytest.mark.parametrize("M,N", sorted(fc.COUNTS))
def test_full_solves_with_exact(gpu, M, N, algo):
    prob = EllipseProblem(M, N)
    f, g, u = fc.rhs(M, N), fc.w0(M, N), fc.exact(M, N)
    for warm in (False, True):
        base = solve(prob, backend="hip", algo=algo, rhs=f, w0=g if warm else None, return_w=True)
        rep = solve(prob, backend="hip", algo=algo, rhs=f, w0=g if warm else None, exact=u, return_w=True)
        tag = f"{M}x{N} {rep.algo} {'w0' if warm else 'zero'}"
        assert rep.converged and rep.iters == fc.COUNTS[(M, N)][warm], (tag, rep.iters)
        xc.same_solve(tag, rep, base)
        xc.check_error(tag, prob, rep, base=base)


# ---- 3. device tensors --------------------------------------------------------------------------
def test_exact_tensor_on_one_block(gpu, nat):
    """kSliceField<T, 0> into the exact plane for the four views, against the
    host array of the same values: the same plane, the same error bits."""
    M, N = 10, 50
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    blk = D.block(M, N, 1, 0)
    s = nat.DeviceSolver(prob.to_native(), blk, None, nat.SolveOptions())
    fc.set_fields(nat, s, M, N, fc.rhs(M, N), fc.w0(M, N))
    assert s.user_plane(2) is None and not s.user_exact
    for name, t, th in views(fc.exact(M, N)):
        want = nat.block_field(M, N, blk, th, 0)
        s.set_exact(want)
        host = s.solve()
        assert np.array_equal(s.user_plane(2), want)
        s.set_exact(None)
        assert s.user_plane(2) is None and not s.user_exact
        s.set_exact_device(t.data_ptr(), *t.stride(), t.dtype == torch.float32, stream())
        assert s.user_exact and np.array_equal(s.user_plane(2), want), name
        dev = s.solve()
        assert host.l2_err > 0 and (dev.l2_err, dev.max_err, dev.max_outside, dev.iters) == (
            host.l2_err, host.max_err, host.max_outside, host.iters), name
        l2, mx = xc.errors(prob, np.array(s.w()), th)
        assert dev.l2_err == pytest.approx(l2, rel=xc.L2_REL) and dev.max_err == mx, name
    s.set_exact_device(0, 0, 0, False, 0)  # a null pointer clears
    assert s.user_plane(2) is None and not s.user_exact and s.user_rhs and s.user_w0
    assert s.solve().l2_err == -1.0


@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_exact_tensor_on_every_block(gpu, nat, M, N, ranks, decomp):
    """The plane of every block for the four views against pe::block_field, and
    the group solve's error with the tensor against the host array's."""
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    uv = views(fc.exact(M, N))
    for r in range(ranks):
        blk = D.block(M, N, ranks, r, decomp)
        s = nat.DeviceSolver(prob.to_native(), blk, None, nat.SolveOptions())
        for name, t, th in uv:
            s.set_exact_device(t.data_ptr(), *t.stride(), t.dtype == torch.float32, stream())
            got = s.user_plane(2)
            assert got.shape == (blk.nx, blk.ny) and np.array_equal(got, nat.block_field(M, N, blk, th, 0)), (name, r)
            assert np.array_equal(got, th[blk.i0 - 1:blk.i0 - 1 + blk.nx, blk.j0 - 1:blk.j0 - 1 + blk.ny]), (name, r)
        s.set_exact_device(0, 0, 0, False, 0)
        assert s.user_plane(2) is None and s.user_plane(0) is None and s.user_plane(1) is None
    kw = dict(backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False, rhs=fc.rhs(M, N), w0=fc.w0(M, N))
    host = {}
    for name, t, th in uv:
        if name in ("contiguous", "float32"):  # (the two sets of values)
            host[name] = solve(prob, exact=th, **kw)
        want = host["float32" if name == "float32" else "contiguous"]
        dev = solve(prob, exact=t, **kw)
        assert want.l2_err > 0 and (dev.l2_err, dev.max_err, dev.max_outside, dev.iters) == (
            want.l2_err, want.max_err, want.max_outside, want.iters), name
    assert host["float32"].l2_err != host["contiguous"].l2_err  # (the narrowed values are other values)


# ---- 4. virtual ranks ---------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_virtual_ranks_with_exact(gpu, M, N, ranks, decomp):
    """Every block's kErrorField over its own plane, kGroupReduce over the
    blocks: the comparison on the gathered w, host and device exact alike."""
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    kw = dict(backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False, rhs=fc.rhs(M, N), w0=fc.w0(M, N))
    u = fc.exact(M, N)
    base = solve(prob, return_w=True, **kw)
    host = solve(prob, exact=u, return_w=True, **kw)
    dev = solve(prob, exact=cuda(u), return_w="device", **kw)
    assert f"{host.Px}x{host.Py}" == decomp and host.iters == 9 and not host.converged and base.l2_err == -1.0
    for rep, tag in ((host, "host"), (dev, "device")):
        xc.same_solve(f"{decomp} {tag}", rep, base)
        xc.check_error(f"group {M}x{N} {decomp} {tag}", prob, rep, base=base)
    assert (dev.l2_err, dev.max_err) == (host.l2_err, host.max_err)
    assert isinstance(dev.w, torch.Tensor) and dev.w.is_cuda


# ---- 5. session ---------------------------------------------------------------------------------
@pytest.mark.parametrize("flip", [0, 1])
def test_session_sets_replaces_and_clears_exact(gpu, flip):
    M = N = 40
    prob = EllipseProblem(M, N)
    f, u = fc.rhs(M, N), fc.exact(M, N)
    analytic = solve(prob, backend="hip")
    steps = [(f, u), (f, 2.0 * u), (f, None), (None, u), (None, None)]  # set, replace, clear; with and without rhs
    n_op = flip
    with DeviceSession(prob) as session:
        for n, (a, b) in enumerate(steps):
            ops = []
            for v in (a, b):  # operands alternate between the host and the device
                ops.append(v if v is None or n_op % 2 else cuda(v))
                n_op += v is not None
            rep = session.solve(rhs=ops[0], exact=ops[1], return_w=True)
            ref = solve(prob, backend="hip", rhs=a, exact=b, return_w=True)
            assert rep.converged and (rep.timers["construct"] == 0) == (n > 0) and ref.timers["construct"] > 0
            assert (rep.l2_err, rep.max_err) == (ref.l2_err, ref.max_err), n
            xc.same_solve(n, rep, ref)
            assert bool(session.solver.user_exact) == (b is not None)
            if b is not None:
                xc.check_error(f"session step {n}", prob, rep, u=b)
            elif a is not None:
                assert rep.l2_err == -1.0 and rep.max_err == -1.0
            else:
                assert (rep.l2_err, rep.max_err) == (analytic.l2_err, analytic.max_err) and rep.iters == 50
        assert session.solver.user_plane(2) is None


# ---- 6. the tie to the built-in path on the device ----------------------------------------------
def test_analytic_tensor_is_kerrors_error(gpu):
    """No rhs, exact = F (1 − x² − 4y²) / 10 as a GPU tensor: kErrorField over
    the plane against kError's expression — the solve bit for bit, l2_err to
    1e-12, max_err to 1e-15 absolute (|u| ≤ 0.1, ulp 1.4e-17)."""
    M, N = 10, 50
    prob = EllipseProblem(M, N)
    X, Y = fc._xy(prob)
    u = prob.F * (1.0 - X * X - 4.0 * Y * Y) / 10.0
    a = solve(prob, backend="hip", algo="three-step", return_w=True)
    b = solve(prob, backend="hip", algo="three-step", exact=cuda(u), return_w=True)
    print(f"exact-tie hip l2_rel={abs(a.l2_err - b.l2_err) / a.l2_err:.2e} max_diff={abs(a.max_err - b.max_err):.2e}")
    assert a.algo == b.algo == "three-step" and a.converged
    xc.same_solve("tie", b, a)
    assert b.l2_err == pytest.approx(a.l2_err, rel=1e-12)
    assert b.max_err == pytest.approx(a.max_err, rel=0, abs=1e-15)
    xc.check_error("tie hip", prob, b, u=u, base=a)


# ---- 7. two processes on one GPU ----------------------------------------------------------------
def test_two_processes_with_exact(gpu, tmp_path):
    """Row slabs of 37×50 over the host-staged transport (exact_field_job.py):
    every rank loads the three arrays onto its device and solves with
    return_w="device"; both report the job's error, which is the comparison's
    on the assembled w."""
    from conftest import free_port

    M, N = 37, 50
    paths = [str(tmp_path / n) for n in ("f.npy", "g.npy", "u.npy")]
    for p, a in zip(paths, (fc.rhs(M, N), fc.w0(M, N), fc.exact(M, N))):
        np.save(p, a)
    env = dict(os.environ, PE_COMM="host", PE_HALO="exchange", PE_OVERLAP="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(ROOT, "tests", "exact_field_job.py"),
           "hip", str(M), str(N), *paths, str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    w = np.full((M - 1, N - 1), np.nan)
    d = []
    for r in range(2):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d.append(json.load(fh))
        blk = np.load(tmp_path / f"out.r{r}.npy")
        i0, j0 = d[r]["w_origin"]
        w[i0 - 1:i0 - 1 + blk.shape[0], j0 - 1:j0 - 1 + blk.shape[1]] = blk
        assert d[r]["user_exact"] and d[r]["ranks"] == 2 and (d[r]["Px"], d[r]["Py"]) == (2, 1) and d[r]["converged"]
    assert np.isfinite(w).all()
    for k in ("l2_err", "max_err", "max_outside", "iters"):
        assert d[0][k] == d[1][k], k
    l2, mx = xc.errors(EllipseProblem(M, N), w)
    print(f"exact-dev two-process algo={d[0]['algo']} iters={d[0]['iters']} l2={d[0]['l2_err']:.6e} "
          f"l2_rel={abs(d[0]['l2_err'] - l2) / l2:.2e} max_diff={abs(d[0]['max_err'] - mx):.2e}")
    assert d[0]["l2_err"] == pytest.approx(l2, rel=xc.L2_REL) and d[0]["max_err"] == mx


# ---- 8. refusals --------------------------------------------------------------------------------
def test_exact_refusals(gpu, nat):
    M = N = 40
    prob = EllipseProblem(M, N)
    f, g, u = fc.rhs(M, N), fc.w0(M, N), fc.exact(M, N)
    nan = cuda(u).clone()
    nan[17, 23] = float("nan")
    bad = [torch.zeros(M - 1, N, dtype=torch.float64, device="cuda:0"),
           torch.zeros(M - 1, N - 1, dtype=torch.int64, device="cuda:0"),
           torch.zeros(M - 1, N - 1, dtype=torch.float16, device="cuda:0"),
           torch.zeros(M - 1, N - 1, dtype=torch.complex128, device="cuda:0"),
           nan]
    for t in bad:
        for backend, kw in (("hip", {}), ("hip-group", dict(ranks=4, decomp="2x2"))):
            with pytest.raises(ValueError, match="exact"):
                solve(prob, backend=backend, exact=t, **kw)
    with DeviceSession(prob) as session:
        session.solve(rhs=cuda(f), w0=g, exact=cuda(u))
        before = [session.solver.user_plane(k).copy() for k in range(3)]
        assert np.array_equal(before[2], u)
        for t in bad:
            with pytest.raises(ValueError, match="exact"):
                # (nothing is set before everything is checked)
                session.solve(rhs=cuda(2.0 * f), w0=cuda(2.0 * g), exact=t)
        # a host pointer handed to the solver directly never reaches a kernel
        a = np.ascontiguousarray(u)
        with pytest.raises(ValueError, match="device"):
            session.solver.set_exact_device(a.ctypes.data, N - 1, 1, False, stream())
        small = torch.zeros(M - 1, dtype=torch.float64, device="cuda:0")  # strides that leave the allocation
        with pytest.raises(ValueError):
            session.solver.set_exact_device(small.data_ptr(), 1 << 40, 1, False, stream())
        for k in range(3):
            assert np.array_equal(session.solver.user_plane(k), before[k]), k
