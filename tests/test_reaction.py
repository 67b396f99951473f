"""CPU tests of the reaction field c of −Δu + c(x, y)·u = f (solve(...,
reaction=c); csrc/include/pe/fields.hpp): the constant field against the
constant shift bit for bit, the serial backend against the torch recurrence,
the references of test_reaction_gpu.py before a device sees them, the operator
pass, the refusals, the report, the plan.  Inputs, shapes and bounds:
reaction_checks.  The first test fails without the feature (`reaction` is an
unknown keyword there)."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import reaction_checks as rc

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, apply_operator, residual, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU_BACKENDS = [("serial", {}), ("omp", dict(threads=3)), ("ranks", dict(ranks=4, decomp="2x2"))]


# ---- 1. the constant field is the shift -------------------------------------------------------------------------
@pytest.mark.parametrize("sigma", rc.SIGMAS)
@pytest.mark.parametrize("backend,kw", CPU_BACKENDS, ids=[b for b, _ in CPU_BACKENDS])
def test_constant_field_is_the_shift_bit_for_bit(backend, kw, sigma):
    """reaction = full(σ) and shift = σ share one expression tree: the same w, iterations and last step, no tolerance."""
    M, N = 37, 50
    c = np.full((M - 1, N - 1), sigma)
    a = solve(EllipseProblem(M, N, shift=sigma), backend=backend, return_w=True, **rc.fields(M, N), **kw)
    b = solve(EllipseProblem(M, N), backend=backend, return_w=True, reaction=c, **rc.fields(M, N), **kw)
    assert a.converged and b.converged and a.iters == b.iters and a.last_diff == b.last_diff
    assert np.array_equal(a.w, b.w)
    assert b.l2_err == -1.0 and b.max_err == -1.0
    v, f = fc.w0(M, N), fc.rhs(M, N)
    x, y = apply_operator(EllipseProblem(M, N, shift=sigma), v, backend=backend, **kw), apply_operator(
        EllipseProblem(M, N), v, backend=backend, reaction=c, **kw)
    assert np.array_equal(x.field, y.field) and x.sum == y.sum
    x, y = residual(EllipseProblem(M, N, shift=sigma), v, rhs=f, backend=backend, **kw), residual(
        EllipseProblem(M, N), v, rhs=f, backend=backend, reaction=c, **kw)
    assert np.array_equal(x.field, y.field) and x.sum == y.sum


# ---- 2. the non-constant field ----------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N", rc.SOLVES + [(9, 130)], ids=lambda v: str(v))
def test_serial_against_the_torch_recurrence(M, N):
    c = rc.field(M, N)
    assert c.min() == 0.0 and c.max() > 39.0 and not rc.problem(M, N).reaction
    assert (c[~fc.inside(EllipseProblem(M, N))] > 0).any()  # (non-zero outside the ellipse)
    ref = rc.stop_margin(M, N)
    t = torch_ref.pcg(EllipseProblem(M, N), reaction=c, **rc.fields(M, N))
    print(f"reaction-serial {M}x{N} iters={ref.iters} torch={t.iters} "
          f"dw={np.abs(t.w[1:-1, 1:-1].numpy() - ref.w).max():.2e} last={ref.history[-2:]}")
    assert t.converged and t.iters == ref.iters
    np.testing.assert_allclose(t.w[1:-1, 1:-1].numpy(), ref.w, rtol=0, atol=1e-9)
    assert ref.l2_err == -1.0 and ref.max_err == -1.0 and t.l2_err == -1.0
    # the field is in the system: the iterate is closer to solving (A + diag(c)) w = B than A w = B
    assert (residual(EllipseProblem(M, N), ref.w, rhs=fc.rhs(M, N), backend="serial", reaction=c).sum
            < residual(EllipseProblem(M, N), ref.w, rhs=fc.rhs(M, N), backend="serial").sum)
    for backend, kw in CPU_BACKENDS[1:]:
        rep = solve(EllipseProblem(M, N), backend=backend, return_w=True, reaction=c, **rc.fields(M, N), **kw)
        assert rep.converged and rep.iters == ref.iters
        np.testing.assert_allclose(rep.w, ref.w, rtol=0, atol=1e-9)
    # with an exact field the error is numpy's from the returned w; the solve is the same solve
    u = fc.exact(M, N)
    with_u = solve(EllipseProblem(M, N), backend="serial", return_w=True, reaction=c, exact=u, **rc.fields(M, N))
    e = np.where(fc.inside(EllipseProblem(M, N)), with_u.w - u, 0.0)
    assert np.array_equal(with_u.w, ref.w)
    assert with_u.max_err == pytest.approx(float(np.abs(e).max()), rel=1e-12)


@pytest.mark.parametrize("case", rc.REFERENCES, ids=lambda c: f"{c[0]}x{c[1]}-K{c[2]}-{c[3] or 'ref'}")
def test_classic_references_agree(case):
    """test_classic_oracle.py's gate with the field: torch_ref.classic against
    the capped reference loop and the serial backend within 1e-13·max|w|, both
    ending at K unconverged — the device comparison rests on a checked reference."""
    M, N, k, member = case
    prob = rc.problem(M, N, member)
    c = rc.field(M, N)
    ref = rc.reference(M, N, k, member)
    assert ref.iters == k == len(ref.alpha) == len(ref.beta) == len(ref.sums)
    wmax = float(ref.w.abs().max())
    loop = torch_ref.pcg(prob, max_iter=k, reaction=c, **rc.fields(M, N))
    assert loop.iters == k and not loop.converged
    assert float((ref.w - loop.w).abs().max()) <= 1e-13 * wmax
    prob.max_iter = k
    ser = solve(prob, backend="serial", return_w=True, reaction=c, **rc.fields(M, N))
    assert ser.iters == k and not ser.converged
    assert abs(ser.w - ref.w[1:M, 1:N].numpy()).max() <= 1e-13 * wmax
    inner = lambda u, v: float((u[1:-1, 1:-1] * v[1:-1, 1:-1]).sum())  # noqa: E731
    assert ref.sums[-1][1] == inner(ref.p, ref.p)
    assert ref.alpha[-1] == pytest.approx(ref.sums[-2][2] / ref.sums[-1][0], rel=1e-13)


@pytest.mark.parametrize("M,N", [(40, 40), (9, 130), (70, 129)], ids=lambda v: str(v))
def test_operator_pass_against_the_torch_oracle(nat, M, N):
    """pe.residual / apply_operator with the field against torch_ref at the operator tests' bound, and the definition
    written out: A_c v = (A v) + c·v with no contraction, the bits of numpy."""
    prob, c, v, f = EllipseProblem(M, N), rc.field(M, N), fc.w0(M, N), fc.rhs(M, N)
    want = torch_ref.residual(prob, v, f, reaction=c)[1:-1, 1:-1].numpy()
    for backend, kw in CPU_BACKENDS[:2] + [("torch", dict(device="cpu"))]:
        got = residual(prob, v, rhs=f, backend=backend, reaction=c, **kw)
        assert np.abs(got.field - want).max() <= 1e-13 * np.abs(want).max()
        assert got.sum == pytest.approx(prob.h1 * prob.h2 * float((want * want).sum()), rel=1e-12)
    base = apply_operator(prob, v, backend="serial").field
    got = apply_operator(prob, v, backend="serial", reaction=c)
    assert np.array_equal(got.field, base + c * v)
    assert got.sum == pytest.approx(prob.h1 * prob.h2 * float((v * got.field).sum()), rel=1e-12)
    P = rc.problem(M, N, reaction=True).to_native()
    for threads in (1, 3):
        s, a = nat.apply_operator(P, v, True, threads, c)
        assert np.array_equal(np.asarray(a), got.field) and s == pytest.approx(got.sum, rel=1e-12)


# ---- 3. refusals, each by message --------------------------------------------------------------------------------
def test_refusals(nat):
    M, N = 40, 40
    prob, c, v = EllipseProblem(M, N), rc.field(M, N), fc.w0(M, N)
    neg, nan, inf = c.copy(), c.copy(), c.copy()
    neg[5, 7], nan[5, 7], inf[5, 7] = -1e-300, np.nan, np.inf
    every = CPU_BACKENDS + [("torch", dict(device="cpu")), ("dist-cpu", {}), ("hip", {}), ("hip-group", dict(ranks=2))]
    for backend, kw in every:
        for bad, msg in ((neg, "reaction: negative"), (nan, "reaction: non-finite"), (inf, "reaction: non-finite"),
                         (c[:-1], r"reaction: expected the global interior, shape \(39, 39\)"),
                         (c.astype(np.complex128), "reaction: dtype complex128")):
            with pytest.raises(ValueError, match=msg):
                solve(prob, backend=backend, reaction=bad, **kw)
            with pytest.raises(ValueError, match=msg):
                apply_operator(prob, v, backend=backend, reaction=bad, **kw)
            with pytest.raises(ValueError, match=msg):
                residual(prob, v, backend=backend, reaction=bad, **kw)
        with pytest.raises(ValueError, match="reaction together with shift != 0 .*add the constant to the field"):
            solve(EllipseProblem(M, N, shift=2.0), backend=backend, reaction=c, **kw)
        with pytest.raises(ValueError, match="reaction=True but no field"):
            solve(EllipseProblem(M, N, reaction=True), backend=backend, **kw)
    for algo in ("fused", "two-step", "three-step"):
        for backend, kw in (("hip", {}), ("hip-group", dict(ranks=2))):
            with pytest.raises(ValueError, match=f'algo "{algo}".*reaction'):
                solve(prob, backend=backend, reaction=c, algo=algo, **kw)
        with pytest.raises(ValueError, match=f'algo "{algo}".*reaction'):
            DeviceSession(prob, reaction=c, algo=algo)
    with pytest.raises(ValueError, match="reaction together with shift"):
        torch_ref.pcg(EllipseProblem(M, N, shift=1.0), reaction=c)
    with pytest.raises(ValueError, match="reaction must be finite and >= 0"):
        torch_ref.classic(prob, 3, reaction=neg)
    # the native layer refuses on its own (a Problem filled in by hand)
    from poisson_ellipse_openmp_mpi_cuda_amd.solver import _options

    P, Q = EllipseProblem(M, N, reaction=True).to_native(), prob.to_native()
    for bad in (neg, nan, inf):
        with pytest.raises(ValueError, match="reaction must be finite and >= 0 at every node"):
            nat.apply_operator(P, v, True, 1, bad)
        with pytest.raises(ValueError, match="reaction must be finite and >= 0 at every node"):
            nat.cpu_solve_grid(P, D.grid(4, M, N, "2x2"), _options(), False, None, None, None, bad)
    with pytest.raises(ValueError, match="go together"):
        nat.residual_field(Q, v, None, True, 1, c)
    with pytest.raises(ValueError, match="go together"):
        nat.cpu_solve_grid(P, D.grid(1, M, N, "reference"), _options(), False)
    P.shift = 3.0
    with pytest.raises(ValueError, match="add the constant to the field"):
        nat.apply_operator(P, v, True, 1, c)


# ---- 4. the report, the default, the plan --------------------------------------------------------------------------
def test_report_and_problem_carry_the_flag():
    M, N = 26, 27
    c = rc.field(M, N)
    rep = solve(EllipseProblem(M, N), backend="serial", reaction=c)
    assert rep.to_dict()["reaction"] is True and rep.reaction
    plain = solve(EllipseProblem(M, N), backend="serial")
    assert "reaction" not in plain.to_dict() and not plain.reaction
    p = EllipseProblem(M, N, reaction=True)
    assert not EllipseProblem().reaction and p.with_grid(40, 40).reaction
    assert p.to_native().reaction is True and EllipseProblem().to_native().reaction is False


@pytest.mark.parametrize("backend,kw", CPU_BACKENDS + [("torch", dict(device="cpu"))], ids=lambda v: str(v))
def test_none_is_the_existing_solve(backend, kw):
    M = N = 40
    a = solve(EllipseProblem(M, N), backend=backend, return_w=True, **rc.fields(M, N), **kw)
    b = solve(EllipseProblem(M, N), backend=backend, return_w=True, reaction=None, **rc.fields(M, N), **kw)
    assert a.iters == b.iters == fc.COUNTS[(M, N)][1] and np.array_equal(a.w, b.w) and a.last_diff == b.last_diff
    d = solve(EllipseProblem(M, N), backend=backend, reaction=None, **kw)
    assert d.iters == 50 and d.l2_err > 0 and "reaction" not in d.to_dict()
    x, y = apply_operator(EllipseProblem(M, N), fc.w0(M, N), backend=backend, **kw), apply_operator(
        EllipseProblem(M, N), fc.w0(M, N), backend=backend, reaction=None, **kw)
    assert np.array_equal(x.field, y.field) and x.sum == y.sum


def test_plan(nat):
    """Planned as a shift is: classic on every decomposition and never the resident kernel for auto; algo 2-4 refused."""
    opt = nat.SolveOptions()
    for M, N, P, spec, comm in ((40, 40, 1, "1x1", 1), (800, 1200, 1, "1x1", 1), (2048, 2048, 1, "1x1", 1),
                                (2048, 2048, 4, "rows", 4), (2048, 2048, 4, "2x2", 1)):
        blk = nat.decompose(M, N, D.grid(P, M, N, spec), 0)
        for algo in (0, 1):
            opt.algo = algo
            pl = nat.solver_plan(EllipseProblem(M, N, reaction=True).to_native(), blk, comm, opt)
            sh = nat.solver_plan(EllipseProblem(M, N, shift=40.0).to_native(), blk, comm, opt)
            assert not pl["fused"] and pl["steps"] == 1 and not pl["tune_ti"], (M, N, spec, pl)
            assert pl["algo"] == "classic" and not pl["resident"], (M, N, spec, pl)
            assert {k: pl[k] for k in ("fused", "steps", "ti", "order", "tune_ti")} == {
                k: sh[k] for k in ("fused", "steps", "ti", "order", "tune_ti")}
        opt.algo = 0
        assert nat.solver_plan(EllipseProblem(M, N).to_native(), blk, comm, opt)["fused"]  # (the default is unchanged)
        for algo in (2, 3, 4):
            opt.algo = algo
            with pytest.raises(ValueError, match="reaction"):
                nat.solver_plan(EllipseProblem(M, N, reaction=True).to_native(), blk, comm, opt)
    P = EllipseProblem(40, 40, reaction=True).to_native()
    P.shift = 1.0
    opt.algo = 0
    with pytest.raises(ValueError, match="reaction together with shift"):
        nat.solver_plan(P, nat.decompose(40, 40, D.grid(1, 40, 40, "1x1"), 0), 1, opt)


# ---- 5. the command line ---------------------------------------------------------------------------------------------
def test_cli_reaction(tmp_path):
    M, N = 40, 40
    np.save(tmp_path / "c.npy", rc.field(M, N))
    np.save(tmp_path / "f.npy", fc.rhs(M, N))
    np.save(tmp_path / "g.npy", fc.w0(M, N))
    np.save(tmp_path / "neg.npy", -rc.field(M, N))
    py = [sys.executable, "-m", "poisson_ellipse_openmp_mpi_cuda_amd.cli", "--backend", "serial"]
    run = lambda cmd: subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)  # noqa: E731
    out = run(py + ["--reaction", str(tmp_path / "c.npy"), "--rhs", str(tmp_path / "f.npy"), "--w0", str(tmp_path / "g.npy"),
                    "--json", "--dump", str(tmp_path / "w.npy"), str(M), str(N)])
    assert out.returncode == 0, out.stderr
    ref = rc.serial(M, N)
    d = json.loads(out.stdout.strip().splitlines()[-1])
    assert d["reaction"] is True and d["iters"] == ref.iters and d["l2_err"] == -1.0 and "n/a" in out.stdout
    assert np.array_equal(np.load(tmp_path / "w.npy"), ref.w)
    out = run(py + ["--json", str(M), str(N)])
    assert out.returncode == 0 and "reaction" not in out.stdout
    out = run(py + ["--reaction", str(tmp_path / "neg.npy"), str(M), str(N)])
    assert out.returncode == 2 and "reaction" in out.stderr and out.stdout == ""
    out = run(py + ["--reaction", str(tmp_path / "c.npy"), "--shift", "1", str(M), str(N)])
    assert out.returncode == 2 and "add the constant to the field" in out.stderr
