"""MI355X tests of the operator pass (kApplyField; DeviceSolver.apply_device /
residual_device, DeviceSession.apply / residual, pe.apply_operator /
pe.residual on hip and hip-group, multi-process jobs): the kernel reading the
caller's global array in place — tile edges, idle lanes, strides, float32,
every layout the solver can be in, block seams.

Inputs and bounds: operator_checks (field_checks.w0 / rhs; fields to
1e-13·max|ref| against the host definition, sums to the CPU tolerances).
Whether a field equals the host's bit for bit is printed, not asserted; device
runs of the same values must give identical bits to each other, asserted.
Every test takes seconds and fails without the feature (no such names)."""

import json
import math
import os
import subprocess
import sys

import field_checks as fc
import norm_checks
import numpy as np
import operator_checks as oc
import pytest
import torch
from test_device_fields_gpu import cuda, stream

import poisson_ellipse_openmp_mpi_cuda_amd as pe
from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(res):
    f = res.field
    return f.cpu().numpy() if isinstance(f, torch.Tensor) else f


# ---- 1. shapes: the smallest at which the kernel can go wrong (256 columns per tile, 4 rows per step) -----------
@pytest.mark.parametrize("M,N,kw", [
    (10, 10, None),
    (40, 40, None),
    (7, 257, None),      # six rows: not a multiple of the row batch; exactly one full column tile
    (9, 258, None),      # a second column tile with one live lane
    (257, 129, None),
    (18, 21, None),      # 17 rows at the launch's band height of 8: the last row band has a single row
] + oc.STRETCHED)
def test_shapes(gpu, M, N, kw):
    prob = oc.problem(M, N, kw)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    with DeviceSession(prob) as s:
        a = s.apply(v)
        oc.compare(f"{M}x{N}", prob, a.field, a.sum)
        r = s.residual(cuda(v), rhs=None)
        oc.compare(f"{M}x{N} F", prob, r.field, r.sum, True)
        ru = s.residual(v, rhs=f)
        oc.compare(f"{M}x{N} rhs", prob, ru.field, ru.sum, True, True)
        assert a.origin is None and isinstance(a.field, np.ndarray)


# ---- 2. out modes and input forms -------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", [(9, 258), (40, 40)])
def test_out_modes_and_input_forms(gpu, M, N):
    prob = EllipseProblem(M, N)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    v32 = oc.operand(M, N, f32=True)
    t = cuda(v)
    big = torch.full((N + 4, M + 2), -7.0, dtype=torch.float64, device="cuda:0")
    big[3:3 + N - 1, 1:M] = t.T
    forms = [("host", v, False), ("f64", t, False), ("transposed", big[3:3 + N - 1, 1:M].T, False),
             ("f32", cuda(v).to(torch.float32), True), ("f64 of f32", cuda(v32), True), ("host of f32", v32, True)]
    assert not forms[2][1].is_contiguous()
    with DeviceSession(prob) as s:
        for resid, user in ((False, False), (True, False), (True, True)):
            first = {}
            for name, x, f32 in forms:
                kw = dict(rhs=f if user else None) if resid else {}
                call = s.residual if resid else s.apply
                h, d, only = call(x, out="host", **kw), call(x, out="device", **kw), call(x, out="sum", **kw)
                oc.compare(f"{M}x{N} {name}", prob, h.field, h.sum, resid, user, f32)
                assert isinstance(d.field, torch.Tensor) and d.field.is_cuda and d.field.dtype == torch.float64
                assert tuple(d.field.shape) == (M - 1, N - 1) and d.origin is None and only.field is None
                assert np.array_equal(host(d), h.field) and d.sum == h.sum == only.sum, name
                ref = first.setdefault(f32, (h.field, h.sum))  # the same values: identical bits whatever the form
                assert np.array_equal(h.field, ref[0]) and h.sum == ref[1], name
        # an expanded (stride 0) tensor against its materialised copy, and against the host definition of the constant
        c = torch.full((1, 1), 0.375, dtype=torch.float64, device="cuda:0").expand(M - 1, N - 1)
        assert c.stride() == (0, 0)
        e, m = s.apply(c), s.apply(c.contiguous())
        assert np.array_equal(e.field, m.field) and e.sum == m.sum
        sc, fcst = gpu.apply_operator(prob.to_native(), np.full((M - 1, N - 1), 0.375))
        assert np.abs(e.field - fcst).max() <= 1e-13 * np.abs(fcst).max() and e.sum == pytest.approx(sc, rel=1e-12)


def test_residual_rhs_semantics(gpu):
    """F, a user rhs for the call, F again after clearing it; left out, the last one stays; solve(rhs=) sets it too."""
    M = N = 40
    prob = EllipseProblem(M, N)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    with DeviceSession(prob) as s:
        builtin = s.residual(v, rhs=None)
        user = s.residual(v, rhs=cuda(f))
        kept = s.residual(v)
        cleared = s.residual(v, rhs=None)
        oc.compare("F", prob, builtin.field, builtin.sum, True)
        oc.compare("rhs", prob, user.field, user.sum, True, True)
        assert np.array_equal(kept.field, user.field) and kept.sum == user.sum
        assert np.array_equal(cleared.field, builtin.field) and cleared.sum == builtin.sum
        s.solve(rhs=f)
        after = s.residual(v)
        assert np.array_equal(after.field, user.field)
    one = pe.residual(prob, v, rhs=f, backend="hip")
    assert np.array_equal(one.field, user.field) and one.sum == user.sum


# ---- 3. every layout, before a solve, after one, after a gradient pass ------------------------------------------
@pytest.mark.parametrize("algo,M,N,variant,want", [
    ("three-step", 10, 50, 0, "three-step"),
    ("three-step", 66, 49, 0, "three-step"),
    ("two-step", 10, 122, 0, "two-step"),
    ("fused", 10, 126, 0, "fused"),            # (the streaming single sweep: PE_RESIDENT=0)
    ("auto", 34, 250, 0, "resident"),
    ("classic", 10, 50, 0, "classic"),
    ("classic", 10, 50, 1, "classic")])
def test_every_layout(gpu, algo, M, N, variant, want, monkeypatch):
    if algo == "fused":
        monkeypatch.setenv("PE_RESIDENT", "0")
    prob = EllipseProblem(M, N)
    prob.max_iter = 9
    v, f = fc.w0(M, N), fc.rhs(M, N)
    vt = cuda(v)
    with DeviceSession(prob, algo=algo, variant=variant) as s:
        def both():
            a, r = s.apply(vt), s.residual(vt, rhs=f)
            return a.field, a.sum, r.field, r.sum

        before = both()
        rep = s.solve(rhs=f, w0=v)
        assert rep.algo == want and rep.iters >= 9 and not rep.converged, (rep.algo, rep.iters)
        after = both()
        s.solve(rhs=f, w0=v, return_grad="stats")
        after_grad = both()
    oc.compare(f"{want} v{variant} {M}x{N}", prob, before[0], before[1])
    oc.compare(f"{want} v{variant} {M}x{N}", prob, before[2], before[3], True, True)
    for other in (after, after_grad):
        assert np.array_equal(other[0], before[0]) and np.array_equal(other[2], before[2])
        assert other[1] == before[1] and other[3] == before[3]


# ---- 4. the pass disturbs nothing -------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "three-step", "classic"])
def test_pass_disturbs_nothing(gpu, algo):
    M = N = 40
    prob = EllipseProblem(M, N)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    same = ("iters", "converged", "last_diff", "l2_err", "max_err", "max_outside", "res_true", "res_rec", "b_norm")
    with DeviceSession(prob, algo=algo) as s:
        s.solve(rhs=f, return_w=True)
        s.apply(v)
        s.residual(cuda(v), out="device")
        second = s.solve(rhs=f, w0=v, return_w=True)
    with DeviceSession(prob, algo=algo) as s:
        s.solve(rhs=f, return_w=True)
        ref = s.solve(rhs=f, w0=v, return_w=True)
    assert np.array_equal(second.w, ref.w)
    for k in same:
        assert getattr(second, k) == getattr(ref, k), k


# ---- 5. the tie to the solver -----------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "three-step", "two-step", "fused", "classic"])
def test_tie_to_the_solver(gpu, algo, nat):
    """‖B − A w‖_E of a converged solve's w through kApplyField (exact coefficients)
    against the solve's own res_true (kResid, division-free coefficients) — where
    the layout has none (classic: −1) against fp64 numpy — and (w, A w)."""
    M = N = 40
    prob = EllipseProblem(M, N)
    with DeviceSession(prob, algo=algo) as s:
        rep = s.solve(return_w=True)
        assert rep.converged
        r = s.residual(rep.w, rhs=None, out="sum")
        a = s.apply(rep.w, out="sum")
    ref = rep.res_true if rep.res_true >= 0 else norm_checks.fp64_norms(prob, rep.w)["res_true"]
    print(f"operator-tie {rep.algo} resid={math.sqrt(r.sum):.12e} res_true={ref:.12e}")
    assert r.field is None and math.sqrt(r.sum) == pytest.approx(ref, rel=norm_checks.resid_tol(prob))
    Aw = nat.apply_operator(prob.to_native(), rep.w)[1]
    hh = prob.h1 * prob.h2
    assert abs(a.sum - hh * float((rep.w * Aw).sum())) <= 1e-12 * hh * float(np.abs(rep.w * Aw).sum())


# ---- 6. seams ---------------------------------------------------------------------------------------------------
def single_rank(prob, M, N):
    with DeviceSession(prob) as s:
        a, r = s.apply(cuda(fc.w0(M, N)), out="device"), s.residual(cuda(fc.w0(M, N)), rhs=fc.rhs(M, N), out="device")
    return host(a), a.sum, host(r), r.sum


@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (37, 50, 3, "3x1")])
def test_virtual_ranks(gpu, M, N, ranks, decomp):
    prob = EllipseProblem(M, N)
    v, f = fc.w0(M, N), fc.rhs(M, N)
    af, asum, rf, rsum = single_rank(prob, M, N)
    kw = dict(backend="hip-group", ranks=ranks, decomp=decomp)
    for x, out in ((v, "host"), (cuda(v), "device"), (cuda(v), "host"), (v, "device")):
        a = pe.apply_operator(prob, x, out=out, **kw)
        r = pe.residual(prob, x, rhs=cuda(f) if out == "device" else f, out=out, **kw)
        if out == "device":  # the global tensor, every block's kernel having written its position
            assert isinstance(a.field, torch.Tensor) and a.field.is_cuda and tuple(a.field.shape) == (M - 1, N - 1)
            assert a.origin is None
        assert np.array_equal(host(a), af) and np.array_equal(host(r), rf), (decomp, out)
        oc.compare(f"group {decomp}", prob, host(a), a.sum)
        oc.compare(f"group {decomp}", prob, host(r), r.sum, True, True)
    only = pe.apply_operator(prob, v, out="sum", **kw)
    assert only.field is None and only.sum == a.sum


@pytest.mark.parametrize("M,N,world,decomp,grid", [(37, 50, 3, "rows", (3, 1)), (26, 27, 4, "2x2", (2, 2))])
def test_processes_on_one_gpu(gpu, tmp_path, M, N, world, decomp, grid):
    """Row slabs and a 2 × 2 grid of processes over the host-staged transport
    (operator_job.py): every rank reads the global tensor on its device and
    returns its block; reassembled, the fields are the single-rank device
    fields bit for bit, and every rank reports the job's sums."""
    from conftest import free_port

    prob = EllipseProblem(M, N)
    paths = [str(tmp_path / n) for n in ("v.npy", "f.npy")]
    for p, a in zip(paths, (fc.w0(M, N), fc.rhs(M, N))):
        np.save(p, a)
    env = dict(os.environ, PE_COMM="host", PE_HALO="exchange", PE_OVERLAP="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "operator_job.py"), "hip", str(M), str(N), *paths, str(tmp_path / "out"), decomp]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    A = np.full((M - 1, N - 1), np.nan)
    R = np.full((M - 1, N - 1), np.nan)
    d = []
    for r in range(world):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d.append(json.load(fh))
        ba, br = np.load(tmp_path / f"out.r{r}.a.npy"), np.load(tmp_path / f"out.r{r}.r.npy")
        i0, j0 = d[r]["origin"]
        A[i0 - 1:i0 - 1 + ba.shape[0], j0 - 1:j0 - 1 + ba.shape[1]] = ba
        R[i0 - 1:i0 - 1 + br.shape[0], j0 - 1:j0 - 1 + br.shape[1]] = br
    assert len({tuple(x["origin"]) for x in d}) == world == grid[0] * grid[1]
    af, asum, rf, rsum = single_rank(prob, M, N)
    assert np.array_equal(A, af) and np.array_equal(R, rf)
    for x in d:
        assert x["apply_sum"] == d[0]["apply_sum"] and x["resid_sum"] == d[0]["resid_sum"]
    oc.compare(f"{world} processes {decomp}", prob, A, d[0]["apply_sum"])
    oc.compare(f"{world} processes {decomp}", prob, R, d[0]["resid_sum"], True, True)


# ---- 7. refusals ------------------------------------------------------------------------------------------------
def test_refusals(gpu):
    M = N = 40
    prob = EllipseProblem(M, N)
    v = fc.w0(M, N)
    with DeviceSession(prob) as s:
        good = s.apply(cuda(v))
        hostv = np.ascontiguousarray(v)
        dst = torch.zeros((M - 1, N - 1), dtype=torch.float64, device="cuda:0")
        with pytest.raises(ValueError, match="device"):  # a host pointer never reaches a kernel
            s.solver.apply_device(hostv.ctypes.data, N - 1, 1, False, False, dst.data_ptr(), N - 1, 1, 0, 0, stream())
        with pytest.raises(ValueError, match="device"):  # nor a host destination
            s.solver.apply_device(cuda(v).data_ptr(), N - 1, 1, False, True, hostv.ctypes.data, N - 1, 1, 0, 0, stream())
        with pytest.raises(ValueError):  # strides that leave the allocation
            s.solver.apply_device(dst.data_ptr(), 1 << 40, 1, False, False, 0, 0, 0, 0, 0, stream())
        with pytest.raises(ValueError, match="shape"):
            s.apply(cuda(v)[:-1])
        with pytest.raises(ValueError, match="dtype"):
            s.apply(cuda(v).to(torch.float16))
        with pytest.raises(ValueError, match="out"):
            s.apply(v, out="gpu")
        if torch.cuda.device_count() > 1:  # a tensor of another device
            with pytest.raises(ValueError, match="cuda"):
                s.apply(torch.from_numpy(np.array(v)).to("cuda:1"))
        assert (dst == 0).all()
        again = s.apply(cuda(v))  # nothing was launched by a refused call: the session is usable
        assert np.array_equal(again.field, good.field) and again.sum == good.sum
        assert s.solve().converged
    with pytest.raises(ValueError, match="device"):
        pe.apply_operator(prob, v, backend="torch", out="device")
