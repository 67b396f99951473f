"""MI355X tests of the reaction field c of −Δu + c(x, y)·u = f: the FIELD
instantiations of the classic two-kernel path (csrc/hip/kernels.hip kInitField,
kF, kG) node for node against the fp64 reference loop after a fixed number of
iterations, the one-node ring of the device plane on virtual ranks and across
processes, the constant field against the constant shift, converged solves on
every device backend, the session's field replaced between solves, the
refusals.  Inputs, shapes, references and bounds: reaction_checks.py (the
references are gated on the CPU by test_reaction.py).  Every case takes
seconds; the first test fails without the feature (`reaction` is an unknown
keyword there)."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import reaction_checks as rc
import shift_checks as sc
import torch
from test_device_fields_gpu import cuda

import poisson_ellipse_openmp_mpi_cuda_amd as pe
from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _free(monkeypatch):
    monkeypatch.delenv("PE_TI", raising=False)
    monkeypatch.delenv("PE_ORDER", raising=False)


# ---- 1. converged solves (the public interface first) ---------------------------------------------------------------
@pytest.mark.parametrize("M,N", rc.SOLVES, ids=lambda v: str(v))
def test_converged_solves(gpu, M, N):
    """hip, hip-group 2x2 and a DeviceSession with the field as a GPU tensor — float64, float32 and strided: the
    classic path, serial's iteration count, w within 1e-10; and the same under the residual stop rule."""
    c, kw = rc.field(M, N), rc.fields(M, N)
    ref = rc.stop_margin(M, N)
    rep = solve(EllipseProblem(M, N), backend="hip", reaction=c, return_w=True, **kw)
    grp = solve(EllipseProblem(M, N), backend="hip-group", ranks=4, decomp="2x2", reaction=cuda(c), return_w=True, **kw)
    big = torch.full((N + 4, M + 2), -7.0, dtype=torch.float64, device="cuda:0")
    big[3:3 + N - 1, 1:M] = cuda(c).T
    strided = big[3:3 + N - 1, 1:M].T
    assert not strided.is_contiguous()
    with DeviceSession(EllipseProblem(M, N), reaction=strided) as s:
        ses = s.solve(return_w="device", rhs=cuda(kw["rhs"]), w0=cuda(kw["w0"]))
        ref32 = rc.stop_margin(M, N, f32=True)
        s32 = s.solve(return_w=True, reaction=cuda(c).to(torch.float32), **kw)
    for tag, r, want in (("hip", rep, ref), ("hip-group", grp, ref), ("session", ses, ref), ("session-f32", s32, ref32)):
        dw = float(np.abs(host(r.w) - want.w).max())
        print(f"reaction-solve {tag} {M}x{N} iters={r.iters}/{want.iters} dw={dw:.2e} algo={r.algo}")
        assert r.algo == "classic" and r.converged and r.iters == want.iters and dw <= 1e-10
        assert r.l2_err == -1.0 and r.max_err == -1.0 and r.to_dict()["reaction"] is True
    # the residual rule: the classic path carries it
    tol = 1e-6
    res = rc.serial(M, N, tol, "residual")
    for t in (tol * (1 - 1e-3), tol * (1 + 1e-3)):  # (no coin toss: the count holds 1e-3 either side of tol)
        assert torch_ref.pcg(EllipseProblem(M, N, tol=t, stop="residual"), reaction=c, **kw).iters == res.iters
    prob = EllipseProblem(M, N, tol=tol, stop="residual")
    for tag, r in (("hip", solve(prob, backend="hip", reaction=cuda(c), return_w=True, **kw)),
                   ("hip-group", solve(prob, backend="hip-group", ranks=4, decomp="2x2", reaction=c, return_w=True, **kw))):
        dw = float(np.abs(r.w - res.w).max())
        print(f"reaction-solve residual {tag} {M}x{N} iters={r.iters}/{res.iters} dw={dw:.2e}")
        assert r.algo == "classic" and r.converged and r.iters == res.iters and dw <= 1e-10


# ---- 2. node for node, one rank ------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("M,N,K,member", rc.EDGES + rc.FAMILY,
                         ids=[f"{m or 'ref'}-{M}x{N}" for M, N, _, m in rc.EDGES + rc.FAMILY])
def test_node_for_node(gpu, nat, M, N, K, member, variant, monkeypatch):
    """The lane pair of the reaction plane at strip and item edges; uniform rows only (cover) and band rows at the
    box edge (cut_xy)."""
    _free(monkeypatch)
    rc.check_single(nat, M, N, K, variant, member, ti=8)


@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("ti", rc.FORCED_TI)
def test_forced_item_heights(gpu, nat, ti, variant, monkeypatch):
    """130 rows as one-row items, items of 60 + 1 rows and one item of three segments."""
    _free(monkeypatch)
    monkeypatch.setenv("PE_TI", ti)
    M, N, K, _ = rc.FORCED_GRID
    rc.check_single(nat, M, N, K, variant, ti=int(ti))


# ---- 3. the ring ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ranks,decomp", rc.VIRTUAL, ids=[f"{M}x{N}-{d}" for M, N, _, d in rc.VIRTUAL])
def test_ring_on_virtual_ranks(gpu, M, N, ranks, decomp, monkeypatch):
    """The UP neighbour's halo column of c in lane 0 of a one-column strip, in hR, in c1 of lane 63; one-row slabs;
    a 2x2 seam: the gathered w after K iterations against the whole-grid loop."""
    _free(monkeypatch)
    rows, cols = rc.cc.BLOCKS[(M, N, ranks, decomp)]
    for name, c in (("host", rc.field(M, N)), ("device", cuda(rc.field(M, N)))):
        rep = solve(EllipseProblem(M, N, max_iter=rc.K), backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False,
                    return_w=True, reaction=c, **rc.fields(M, N))
        assert rep.algo == "classic" and rep.Px == len(rows) and rep.Py == len(cols) and rep.iters == rc.K
        rc.check_w(f"{M}x{N} {ranks}-{decomp}-virtual field={name}", rep.w, M, N)


def test_ring_across_processes(gpu, tmp_path):
    """Three processes on the one GPU, row slabs, the host-staged transport (reaction_job.py)."""
    from conftest import free_port

    M, N, world, decomp = rc.PROCESSES
    paths = [str(tmp_path / n) for n in ("f.npy", "g.npy", "c.npy")]
    for p, a in zip(paths, (fc.rhs(M, N), fc.w0(M, N), rc.field(M, N))):
        np.save(p, a)
    env = dict({k: v for k, v in os.environ.items() if k not in ("PE_TI", "PE_ORDER")}, PE_COMM="host",
               PE_HALO="exchange", PE_OVERLAP="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "reaction_job.py"), str(M), str(N), str(rc.K), *paths, str(tmp_path / "out"), decomp]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    W = np.full((M - 1, N - 1), np.nan)
    for r in range(world):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d = json.load(fh)
        blk = np.load(tmp_path / f"out.r{r}.npy")
        i0, j0 = d["origin"]
        W[i0 - 1:i0 - 1 + blk.shape[0], j0 - 1:j0 - 1 + blk.shape[1]] = blk
        assert d["algo"] == "classic" and d["iters"] == rc.K and not d["converged"] and d["reaction"] is True
        assert d["Px"] == world and d["Py"] == 1
    rc.check_w(f"{M}x{N} {world}-{decomp}-processes", W, M, N)


# ---- 4. the constant field against the shift -----------------------------------------------------------------------
@pytest.mark.parametrize("variant", (0, 1))
@pytest.mark.parametrize("sigma", rc.SIGMAS)
def test_constant_field_against_the_shift(gpu, sigma, variant):
    """Equal iterations and w within 1e-12·max|w| (not bitwise: the persistent grid, and with it the sum order, may
    differ between instantiations); the operator pass's field is per node — array_equal — its sum at the operator
    tests' bound."""
    M, N = 70, 129
    c, kw = np.full((M - 1, N - 1), sigma), rc.fields(M, N)
    shifted = sc.problem(M, N, None, sigma)
    sc.stop_margin(shifted)
    a = solve(shifted, backend="hip", return_w=True, variant=variant, **kw)
    b = solve(EllipseProblem(M, N), backend="hip", return_w=True, variant=variant, reaction=c, **kw)
    dw = float(np.abs(a.w - b.w).max() / np.abs(a.w).max())
    print(f"reaction-constant {M}x{N} sigma={sigma} v{variant} iters={b.iters}/{a.iters} dw={dw:.2e} "
          f"bitwise={np.array_equal(a.w, b.w)}")
    assert a.algo == b.algo == "classic" and a.converged and b.converged and a.iters == b.iters and dw <= 1e-12
    v, f = fc.w0(M, N), fc.rhs(M, N)
    for out in ("host", "device"):
        x = pe.apply_operator(shifted, cuda(v), backend="hip", out=out, variant=variant)
        y = pe.apply_operator(EllipseProblem(M, N), cuda(v), backend="hip", out=out, variant=variant, reaction=cuda(c))
        assert np.array_equal(host(x.field), host(y.field))
        sc.compare(f"constant field {out}", shifted, host(y.field), y.sum)
        x = pe.residual(shifted, v, rhs=f, backend="hip", out=out, variant=variant)
        y = pe.residual(EllipseProblem(M, N), v, rhs=f, backend="hip", out=out, variant=variant, reaction=c)
        assert np.array_equal(host(x.field), host(y.field))
        sc.compare(f"constant field {out}", shifted, host(y.field), y.sum, True, True)
    g = pe.apply_operator(EllipseProblem(M, N), v, backend="hip-group", ranks=4, decomp="2x2", reaction=cuda(c))
    sc.compare("constant field group", shifted, g.field, g.sum)


def test_operator_pass_with_the_field(gpu):
    """The non-constant field: the device pass against the host definition, 1e-13·max|ref| and the sum rel 1e-12."""
    M, N = 70, 129
    prob, c, v, f = EllipseProblem(M, N), rc.field(M, N), fc.w0(M, N), fc.rhs(M, N)
    want = pe.residual(prob, v, rhs=f, backend="serial", reaction=c)
    for tag, got in (("hip", pe.residual(prob, cuda(v), rhs=f, backend="hip", reaction=cuda(c))),
                     ("group", pe.residual(prob, v, rhs=cuda(f), backend="hip-group", ranks=2, decomp="1x2", reaction=c))):
        dev = float(np.abs(got.field - want.field).max() / np.abs(want.field).max())
        print(f"reaction-operator {tag} field={dev:.2e} sum={got.sum!r}/{want.sum!r}")
        assert dev <= 1e-13 and got.sum == pytest.approx(want.sum, rel=1e-12)


# ---- 5. a session's field replaced between solves -----------------------------------------------------------------
def test_session_replaces_the_field(gpu):
    """Two solves of one session with two fields — the Newton loop — give what two fresh solves give; left out, the
    last field stays."""
    M, N = 40, 40
    c1, kw = rc.field(M, N), rc.fields(M, N)
    c2 = np.ascontiguousarray(c1[::-1, :]) * 0.5 + 1.0
    fresh = [solve(EllipseProblem(M, N), backend="hip", reaction=c, return_w=True, **kw) for c in (c1, c2)]
    with DeviceSession(EllipseProblem(M, N), reaction=c1) as s:
        first = s.solve(return_w=True, **kw)
        second = s.solve(return_w=True, reaction=cuda(c2), **kw)
        kept = s.solve(return_w=True, **kw)
        again = s.solve(return_w=True, reaction=c1, **kw)
    assert not np.array_equal(fresh[0].w, fresh[1].w)
    for got, want in ((first, fresh[0]), (second, fresh[1]), (kept, fresh[1]), (again, fresh[0])):
        assert got.iters == want.iters and got.converged and np.array_equal(got.w, want.w)


# ---- 6. refusals ---------------------------------------------------------------------------------------------------
def test_device_side_refusals(gpu):
    """ValueError before any launch; a refused call leaves a session as it was."""
    from poisson_ellipse_openmp_mpi_cuda_amd.solver import _options

    M, N = 40, 40
    prob, c, kw = EllipseProblem(M, N), rc.field(M, N), rc.fields(M, N)
    neg, nan = cuda(c), cuda(c)
    neg[5, 7], nan[5, 7] = -1e-300, float("nan")
    for bad, msg in ((neg, "reaction: negative"), (nan, "reaction: non-finite"), (cuda(c)[:-1], "reaction: expected"),
                     (cuda(c).to(torch.float16), "reaction: dtype")):
        for call in (lambda: solve(prob, backend="hip", reaction=bad), lambda: DeviceSession(prob, reaction=bad),
                     lambda: solve(prob, backend="hip-group", ranks=2, reaction=bad),
                     lambda: pe.apply_operator(prob, fc.w0(M, N), backend="hip", reaction=bad)):
            with pytest.raises(ValueError, match=msg):
                call()
    with DeviceSession(prob) as s:  # constructed without a field
        with pytest.raises(ValueError, match="constructed without a reaction field"):
            s.solve(reaction=c)
        assert s.solve(reaction=None).iters == 50
    with DeviceSession(prob, reaction=c) as s:
        before = s.solve(return_w=True, **kw)
        with pytest.raises(ValueError, match="None on a session constructed with a reaction field"):
            s.solve(reaction=None, **kw)
        with pytest.raises(ValueError, match="reaction: negative"):
            s.solve(reaction=neg, **kw)
        after = s.solve(return_w=True, **kw)
        assert np.array_equal(before.w, after.w) and before.iters == after.iters
    # the native layer on its own
    blk = D.block(M, N, 1, 0)
    plain = gpu.DeviceSolver(prob.to_native(), blk, None, _options())
    with pytest.raises(ValueError, match="constructed without Problem::reaction"):
        plain.set_reaction(gpu.block_field(M, N, blk, c, 1))
    flagged = gpu.DeviceSolver(EllipseProblem(M, N, reaction=True).to_native(), blk, None, _options())
    assert not flagged.fused
    with pytest.raises(ValueError, match="none is set"):
        flagged.reset()
    with pytest.raises(ValueError, match="null field"):
        flagged.set_reaction(None)
    with pytest.raises(ValueError, match="reaction"):
        flagged.set_reaction_device(c.ctypes.data, N - 1, 1, False, 0)  # (host memory)
    for algo in ("fused", "two-step", "three-step"):
        with pytest.raises(ValueError, match="reaction"):
            gpu.DeviceSolver(EllipseProblem(M, N, reaction=True).to_native(), blk, None, _options(algo=algo))
