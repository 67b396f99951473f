"""MI355X tests of the user right-hand side and initial guess on the device
paths (DeviceSolver.set_rhs / set_w0, solve(rhs=, w0=)): kInitField into
every live layout (classic, single-, two- and three-step planes, the resident
kernel's start), kResidField for the end-of-solve check and the three-step
restart, the virtual-rank group driver and the per-rank slicing of a
multi-process job.  Inputs, references and comparisons: field_checks.py
(asymmetric in x and y; sweep_checks.KINDS bounds unchanged).

Shapes are the smallest at which indexing, pitch or strip handling can go
wrong (sweep_checks' edge shapes); every test takes seconds."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALGO = {name: sweep_checks.KINDS[name][0] for name in sweep_checks.KINDS}


# ---- 1. fixed iterations, far from convergence, both fields -----------------------------
@pytest.mark.parametrize("kind,M,N,count", [
    ("three", 10, 50, 8),    # a second strip with one output column
    ("three", 66, 49, 8),    # a 17-row last item
    ("two", 10, 122, 6),
    ("single", 10, 126, 20)])
def test_sweeps_with_fields(gpu, nat, kind, M, N, count, monkeypatch):
    if kind == "single":
        monkeypatch.setenv("PE_RESIDENT", "0")
    s = fc.solver(nat, M, N, ALGO[kind])
    assert not s.resident
    fc.check_sweeps(s, M, N, kind, count)


def test_resident_with_fields(gpu, nat):
    """The resident kernel starts from the streaming layout kInitField and
    S_0 left: 34×250 on the default algorithm, 20 iterations."""
    s = fc.solver(nat, 34, 250, 0)
    assert s.resident
    fc.check_sweeps(s, 34, 250, "single", 20)


@pytest.mark.parametrize("variant", [0, 1])
def test_classic_with_fields(gpu, nat, variant):
    """kInitField<EXACT> into the classic layout (pitch = wpitch, r's own
    allocation), kF / kG from there: 20 iterations against the plain loop."""
    M, N, K = 10, 50, 20
    s = fc.solver(nat, M, N, 1, variant)
    assert not s.fused
    s.reset()
    s.run_iterations(K, False)
    s.synchronize()
    st = s.state()
    assert st["iter"] == K and st["status"] == 0
    ref = torch_ref.pcg(EllipseProblem(M, N), rhs=fc.rhs(M, N), w0=fc.w0(M, N), max_iter=K)
    want = ref.w[1:M, 1:N].numpy()
    dev = float(np.abs(s.w() - want).max() / np.abs(want).max())
    print(f"field-sweep-dev classic variant={variant} {M}x{N} count={K} w={dev:.2e}")
    assert dev <= sweep_checks.KINDS["single"][6]


# ---- 2. the tie to today's path ---------------------------------------------------------------
@pytest.mark.parametrize("kind,M,N,K", [("three", 10, 50, 9), ("single", 10, 126, 20)])
def test_constant_fields_are_the_builtin_path(gpu, nat, kind, M, N, K, monkeypatch):
    """rhs ≡ F and w0 ≡ 0 through kInitField / kResidField against no fields
    through kInit / kResid: the same bits after K iterations and after a solve."""
    if kind == "single":
        monkeypatch.setenv("PE_RESIDENT", "0")
    prob = EllipseProblem(M, N)
    F, Z = np.full((M - 1, N - 1), prob.F), np.zeros((M - 1, N - 1))
    plain = fc.solver(nat, M, N, ALGO[kind], fields=False)
    user = fc.solver(nat, M, N, ALGO[kind], fields=False)
    fc.set_fields(nat, user, M, N, F, Z)
    assert user.user_rhs and user.user_w0 and not plain.user_rhs and not plain.user_w0
    for s in (plain, user):
        s.reset()
        s.run_iterations(K, False)
        s.synchronize()
        assert s.state()["iter"] == K
    for which in (0, 4, 2, 3):
        assert np.array_equal(plain.field(which), user.field(which)), which
    assert np.array_equal(plain.w(), user.w())
    algo = {"three": "three-step", "single": "fused"}[kind]
    a = solve(prob, backend="hip", algo=algo, return_w=True)
    b = solve(prob, backend="hip", algo=algo, return_w=True, rhs=F, w0=Z)
    assert a.algo == b.algo == algo and a.converged
    assert (a.iters, a.res_true, a.b_norm) == (b.iters, b.res_true, b.b_norm)
    assert np.array_equal(a.w, b.w)


# ---- 3. full solves ------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["auto", "three-step", "two-step", "fused", "classic"])
@pytest.mark.parametrize("M,N", sorted(fc.COUNTS))
def test_full_solves(gpu, M, N, algo):
    prob = EllipseProblem(M, N)
    f = fc.rhs(M, N)
    for warm in (False, True):
        rep = solve(prob, backend="hip", algo=algo, rhs=f, w0=fc.w0(M, N) if warm else None, return_w=True)
        tag = f"{M}x{N} {rep.algo} {'w0' if warm else 'zero'}"
        assert rep.converged and rep.iters == fc.COUNTS[(M, N)][warm], (tag, rep.iters)
        assert rep.init == ("field" if warm else "zero")
        want = fc.torch_solve(M, N, warm).w[1:-1, 1:-1].numpy()
        print(f"field-solve {tag} iters={rep.iters} w_dev={np.abs(rep.w - want).max() / np.abs(want).max():.2e}")
        np.testing.assert_allclose(rep.w, want, rtol=0, atol=1e-9)
        if algo == "classic":  # no single-sweep layout: no residual check
            assert rep.algo == "classic" and rep.res_true == -1.0 and rep.b_norm == -1.0
            assert rep.l2_err == -1.0 and rep.max_err == -1.0
            assert rep.max_outside == pytest.approx(fc.fp64_norms(prob, rep.w, f)["max_outside"], rel=1e-12)
        else:
            fc.check_norms(tag, prob, rep, f, rep.algo == "three-step")


# ---- 4. the restart restarts the user's problem -----------------------------------------------
def test_drift_restart_with_user_rhs(gpu, monkeypatch):
    """drift@iter:30 pokes w behind the three-step recurrence; the residual
    replacement must go on from r = B − A w with the USER's B.  The bound is
    not a measurement: the F = 1 solution lies 0.45·max|w| away, two converged
    solves of one problem differ by ≤ 3.2e-4·max|w| — 1e-2 separates them by
    more than an order of magnitude on either side."""
    prob = EllipseProblem(40, 40)
    f = fc.rhs(40, 40)
    clean = solve(prob, backend="hip", algo="three-step", rhs=f, return_w=True)
    monkeypatch.setenv("PE_FAULT_INJECT", "drift@iter:30,amp:1e-3")
    hit = solve(prob, backend="hip", algo="three-step", rhs=f, return_w=True)
    dev = float(np.abs(hit.w - clean.w).max() / np.abs(clean.w).max())
    print(f"field-restart restarts={hit.restarts} iters={hit.iters} (clean {clean.iters}) w_dev={dev:.2e} "
          f"res_gap={hit.res_gap:.2e}")
    assert clean.restarts == 0 and clean.iters == 69
    assert hit.algo == "three-step" and hit.restarts >= 1 and hit.converged
    assert dev <= 1e-2


# ---- 5. one solver, several fields ------------------------------------------------------------
def test_one_solver_several_fields(gpu, nat):
    """set_rhs / set_w0 / clearing on a constructed solver: each solve equals
    the same solve on a fresh solver bit for bit; the construction is paid once."""
    M = N = 40
    prob = EllipseProblem(M, N)
    blk = D.block(M, N, 1, 0)
    f, g = fc.rhs(M, N), fc.w0(M, N)
    steps = [(f, None), (2.0 * f, g), (None, None)]

    def run(s, a, b):
        fa, fb = nat.block_fields(M, N, blk, a, b)
        s.set_rhs(fa)
        s.set_w0(fb)
        res = s.solve()
        return res, np.array(s.w())

    one = nat.DeviceSolver(prob.to_native(), blk, None, nat.SolveOptions())
    for n, (a, b) in enumerate(steps):
        res, w = run(one, a, b)
        ref, wref = run(nat.DeviceSolver(prob.to_native(), blk, None, nat.SolveOptions()), a, b)
        assert res.converged and (res.iters, res.last_diff, res.res_true, res.b_norm) == (
            ref.iters, ref.last_diff, ref.res_true, ref.b_norm), n
        assert np.array_equal(w, wref), n
        assert (res.timers["construct"] == 0) == (n > 0) and ref.timers["construct"] > 0
        assert (res.l2_err == -1.0) == (a is not None)
    assert res.iters == 50 and not one.user_rhs and not one.user_w0


# ---- 6. blocks -------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ranks,decomp", [(26, 27, 4, "2x2"), (26, 40, 6, "2x3")])
def test_virtual_ranks_with_fields(gpu, M, N, ranks, decomp):
    """12-13-row blocks on kS3, 9 iterations, both fields sliced per block by
    the group driver; the gathered w against the whole-grid recurrence at
    halo_checks' bound."""
    K = 9
    prob = EllipseProblem(M, N)
    prob.max_iter = K
    rep = solve(prob, backend="hip-group", ranks=ranks, decomp=decomp, check_tol=False, return_w=True,
                rhs=fc.rhs(M, N), w0=fc.w0(M, N))
    assert f"{rep.Px}x{rep.Py}" == decomp and rep.algo == "three-step" and rep.iters == K and not rep.converged
    want = fc.reference("single", M, N, K).w[1:M, 1:N].numpy()
    dev = float(np.abs(rep.w - want).max() / np.abs(want).max())
    print(f"field-halo-dev {M}x{N}-{ranks}-{decomp}-K{K}-virtual w_rel={dev:.2e}")
    assert dev <= sweep_checks.KINDS["three"][6]


def test_two_processes_with_fields(gpu, tmp_path, monkeypatch):
    """Two processes on the one GPU (host-staged transport), row slabs of
    37×50: every rank loads the same global arrays and solve() cuts its slice.
    Same count as the single-rank solve, w within 1e-10·max|w| of it."""
    from conftest import free_port

    M, N = 37, 50
    f, g, outp = str(tmp_path / "f.npy"), str(tmp_path / "g.npy"), str(tmp_path / "w.npy")
    np.save(f, fc.rhs(M, N))
    np.save(g, fc.w0(M, N))
    env = dict(os.environ, PE_COMM="host")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "-m", "poisson_ellipse_openmp_mpi_cuda_amd", "--json",
           "--quiet", "--decomp", "rows", "--rhs", f, "--w0", g, "--dump", outp, str(M), str(N)]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["ranks"] == 2 and d["Px"] == 2 and d["Py"] == 1 and d["converged"] and d["init"] == "field", d
    assert d["l2_err"] == -1.0
    monkeypatch.setenv("PE_RESIDENT", "0")  # (the single-rank solve on the job's streaming sweep)
    one = solve(EllipseProblem(M, N), backend="hip", algo=d["algo"], rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    w = np.load(outp)
    dev = float(np.abs(w - one.w).max() / np.abs(one.w).max())
    print(f"field-two-process algo={d['algo']} iters={d['iters']} (one rank {one.iters}) w_rel={dev:.2e}")
    assert one.algo == d["algo"] and d["iters"] == one.iters
    assert dev <= 1e-10
