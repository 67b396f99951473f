"""CPU tests of the residual stop rule, EllipseProblem(stop="residual"): the
gate, the serial / omp / ranks / dist-cpu / torch loops, the k = 0 and cap
cases, the default's bits, validation, the device plan, the CLI.  Cases, gate
and bounds: stop_checks.  No device is needed; every test takes seconds and
fails without the feature (EllipseProblem has no `stop`)."""

import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import stop_checks as sc

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the gate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(sc.CASES))
def test_gate(name):
    """Every case passes the margin at every tested iterate; the table's K are the recurrence's."""
    K, thr, nat = sc.gate(name)
    assert len(nat) == K + 1 and nat[K] <= thr < min(nat[:K])
    ups = sum(1 for a, b in zip(nat, nat[1:]) if b > a)
    print(f"stop-gate {name} upticks={ups}")


# ---- serial -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sc.TABLE + [n for n in sc.CASES if n not in sc.TABLE])
def test_serial(name):
    """iters = K, converged, res_nat = sqrt(h1 h2 zr_K) and w = the recurrence's w_K.

    40x40-F is the case whose threshold (2.202e-8) lies below sqrt(1e-15): it
    passes because the rule's breakdown test is relative to g (cg_breakdown);
    under the absolute |(Ap, p)·h1h2| < 1e-15 the solve ended in iteration 75,
    "breakdown", with sqrt(g_74) = 3.633e-8 still above the threshold."""
    c = sc.CASES[name]
    K, thr, nat = sc.gate(name)
    rep = sc.serial(name)
    ref = sc.torch_state(name)
    hh = c.problem().h1 * c.problem().h2
    want = float(np.sqrt(ref.sums[K - 1][2] * hh))
    dw = float(np.abs(rep.w - ref.w[1:-1, 1:-1].numpy()).max())
    print(f"stop-serial {name} iters={rep.iters}/{K} converged={rep.converged} breakdown={rep.breakdown} "
          f"res_nat={rep.res_nat!r}/{want!r} dw={dw:.2e}")
    assert rep.converged and not rep.breakdown and rep.iters == K
    assert rep.res_nat == pytest.approx(want, rel=1e-9) and rep.res_nat0 == pytest.approx(nat[0], rel=1e-9)
    assert rep.stop_thr == pytest.approx(thr, rel=1e-12) and rep.res_nat <= rep.stop_thr
    assert dw <= 1e-9
    d = rep.to_dict()
    assert d["stop"] == "residual" and d["atol"] == 0.0 and d["res_nat"] == rep.res_nat and d["stop_thr"] == rep.stop_thr


# ---- the other CPU backends against serial --------------------------------------------------------------------------
BACKENDS = [("omp", dict(threads=3)), ("ranks", dict(ranks=4, decomp="4x1")), ("ranks", dict(ranks=4, decomp="2x2")),
            ("torch", dict(device="cpu"))]


@pytest.mark.parametrize("backend,kw", BACKENDS, ids=["omp", "ranks-4x1", "ranks-2x2", "torch"])
@pytest.mark.parametrize("name", ["40x40-F", "40x40-s40", "70x129", "9x130-s40", "cut_y-66x49"])
def test_backends_against_serial(name, backend, kw):
    c = sc.CASES[name]
    rep = solve(c.problem(), backend=backend, return_w=True, **kw, **c.inputs())
    sc.check_against_serial(f"{backend}{kw.get('decomp', '')}", name, rep, 1e-9)


def test_dist_cpu_through_the_cli(tmp_path):
    """Three processes over gloo, row slabs, started through the CLI with --stop residual --atol: the JSON report
    and the dumped w against serial — the CLI round trip of every new key."""
    from conftest import free_port

    name = "40x40-s40"
    c = sc.CASES[name]
    ref = sc.serial(name)
    f, g, outp = str(tmp_path / "f.npy"), str(tmp_path / "g.npy"), str(tmp_path / "w.npy")
    np.save(f, fc.rhs(c.M, c.N))
    np.save(g, fc.w0(c.M, c.N))
    atol = 1e-9  # (below tol·sqrt(g_0) = 3.2e-6: the threshold and K stay the gated ones)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "3", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), "-m", "poisson_ellipse_openmp_mpi_cuda_amd", "--backend",
           "dist-cpu", "--decomp", "3x1", "--json", "--quiet", "--stop", "residual", "--atol", repr(atol), "--shift",
           repr(c.sigma), "--rhs", f, "--w0", g, "--dump", outp, str(c.M), str(c.N)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert d["ranks"] == 3 and d["converged"] and d["iters"] == ref.iters
    assert d["stop"] == "residual" and d["atol"] == atol and d["shift"] == c.sigma
    for key in ("res_nat", "res_nat0", "stop_thr"):
        assert d[key] == pytest.approx(getattr(ref, key), rel=1e-9), key
    assert np.abs(np.load(outp) - ref.w).max() <= 1e-9


def test_cli_default_output_has_no_stop_keys(tmp_path):
    base = [sys.executable, "-m", "poisson_ellipse_openmp_mpi_cuda_amd", "--backend", "serial", "--json", "--quiet"]
    out = subprocess.run(base + ["40", "40"], cwd=ROOT, capture_output=True, text=True, check=True).stdout
    d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][0])
    assert d["iters"] == 50 and not {"stop", "atol", "res_nat", "res_nat0", "stop_thr"} & set(d)
    bad = subprocess.run(base + ["--atol", "1e-3", "40", "40"], cwd=ROOT, capture_output=True, text=True)
    assert bad.returncode == 2 and "atol" in bad.stderr
    bad = subprocess.run(base + ["--stop", "residual", "--atol", "-1", "40", "40"], cwd=ROOT, capture_output=True,
                         text=True)
    assert bad.returncode == 2 and "atol" in bad.stderr


@pytest.mark.parametrize("tool", ["pe_cpu"])
def test_native_program(tool):
    """bin/pe_cpu --stop residual --atol X: the built-in problem at 40×40 with σ = 40 and τ = 1e-4 (gated) against solve()."""
    exe = os.path.join(ROOT, "bin", tool)
    assert os.path.exists(exe), f"{tool} is not built"
    prob = EllipseProblem(40, 40, shift=40.0, stop="residual", tol=1e-4, atol=1e-12)
    sc.gate_sums(prob)
    ref = solve(prob, backend="serial")
    out = subprocess.run([exe, "--stop", "residual", "--tol", "1e-4", "--atol", "1e-12", "--shift", "40", "--json", "40", "40"],
                         capture_output=True, text=True, check=True).stdout
    d = json.loads(out.strip().splitlines()[-1])
    assert d["iters"] == ref.iters and d["converged"] and d["stop"] == "residual" and d["atol"] == 1e-12
    assert d["res_nat"] == ref.res_nat and d["res_nat0"] == ref.res_nat0 and d["stop_thr"] == ref.stop_thr
    plain = subprocess.run([exe, "--json", "40", "40"], capture_output=True, text=True, check=True).stdout
    assert "stop" not in plain and "atol" not in plain
    bad = subprocess.run([exe, "--atol", "1e-3", "40", "40"], capture_output=True, text=True)
    assert bad.returncode == 2 and "atol" in bad.stderr
    bad = subprocess.run([exe, "--stop", "sometimes", "40", "40"], capture_output=True, text=True)
    assert bad.returncode == 2 and "stop" in bad.stderr


# ---- k = 0 and the cap ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,kw", [("serial", {})] + BACKENDS, ids=["serial", "omp", "ranks-4x1", "ranks-2x2", "torch"])
@pytest.mark.parametrize("sigma", [0.0, 40.0])
def test_zero_iterations(sigma, backend, kw):
    """A w0 that already meets the rule: 0 iterations, converged, w0 back bit for bit."""
    prob, inputs = sc.zero_iteration_problem(40, 40, sigma)
    rep = solve(prob, backend=backend, return_w=True, **kw, **inputs)
    assert rep.iters == 0 and rep.converged and np.array_equal(rep.w, inputs["w0"])
    assert rep.stop_thr == 1e-3 and rep.res_nat == rep.res_nat0 and 0 < rep.res_nat <= 1e-3


@pytest.mark.parametrize("backend,kw", [("serial", {}), ("ranks", dict(ranks=4, decomp="2x2")), ("torch", dict(device="cpu"))],
                         ids=["serial", "ranks-2x2", "torch"])
def test_the_cap_wins(backend, kw):
    """max_iter = K: K iterations, not converged (the capped iterate is not tested); K + 1: K iterations, converged."""
    name = "40x40-s40"
    c, K = sc.CASES[name], sc.gate(name)[0]
    capped = solve(c.problem(max_iter=K), backend=backend, return_w=True, **kw, **c.inputs())
    assert capped.iters == K and not capped.converged and capped.res_nat == -1.0 and capped.res_nat0 > 0
    one_more = solve(c.problem(max_iter=K + 1), backend=backend, return_w=True, **kw, **c.inputs())
    sc.check_against_serial(f"{backend} cap+1", name, one_more, 1e-9)
    assert np.abs(capped.w - one_more.w).max() <= 1e-9  # (the same iterate K)


# ---- the default ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend,kw", [("serial", {})] + BACKENDS, ids=["serial", "omp", "ranks-4x1", "ranks-2x2", "torch"])
def test_explicit_step_rule_is_the_default(backend, kw):
    M, N = 40, 40
    args = dict(backend=backend, rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True, keep_history=True, **kw)
    a, b = solve(EllipseProblem(M, N), **args), solve(EllipseProblem(M, N, stop="step", atol=0.0), **args)
    assert a.converged and a.iters == b.iters and np.array_equal(a.w, b.w) and a.last_diff == b.last_diff
    assert a.history == b.history
    d = b.to_dict()
    assert not {"stop", "atol", "res_nat", "res_nat0", "stop_thr"} & set(d)
    assert (b.res_nat, b.res_nat0, b.stop_thr, b.stop) == (-1.0, -1.0, -1.0, "step")


def test_history_and_last_diff_hold_step_sizes():
    name = "40x40-s40"
    c = sc.CASES[name]
    a = solve(c.problem(), backend="serial", keep_history=True, **c.inputs())
    b = solve(c.problem(stop="step", tol=1e-300), backend="serial", keep_history=True, **c.inputs(), )
    assert len(a.history) == a.iters == sc.gate(name)[0] and a.history == b.history[:a.iters]
    assert a.last_diff == a.history[-1]
    assert EllipseProblem(40, 40, stop="residual", atol=1e-3).with_grid(20, 30).atol == 1e-3


# ---- validation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backend", ["serial", "omp", "ranks", "torch", "dist-cpu", "hip", "hip-group"])
@pytest.mark.parametrize("kw", [dict(stop="sometimes"), dict(stop="residual", atol=-1e-3),
                                dict(stop="residual", atol=float("nan")), dict(stop="residual", atol=float("inf")),
                                dict(atol=1e-3), dict(stop="step", atol=1e-3)],
                         ids=["rule", "negative", "nan", "inf", "atol-default-rule", "atol-step-rule"])
def test_validation(backend, kw):
    """ValueError before any work: no device, process group or solver is touched."""
    with pytest.raises(ValueError, match="stop|atol"):
        solve(EllipseProblem(40, 40, **kw), backend=backend, ranks=2 if backend in ("ranks", "hip-group") else 1)


@pytest.mark.parametrize("atol", [-1.0, float("nan"), float("inf")])
def test_native_validation(nat, atol):
    from poisson_ellipse_openmp_mpi_cuda_amd.solver import _options

    P = EllipseProblem(40, 40, stop="residual").to_native()
    P.atol = atol  # (a native Problem filled in by hand)
    with pytest.raises(ValueError, match="atol"):
        nat.cpu_solve_grid(P, D.grid(1, 40, 40, "reference"), _options(), False, None, None, None)
    with pytest.raises(ValueError, match="atol"):
        nat.solver_plan(P, nat.decompose(40, 40, D.grid(1, 40, 40, "1x1"), 0))
    Q = EllipseProblem(40, 40).to_native()
    Q.atol = 1e-3
    with pytest.raises(ValueError, match="atol"):
        nat.cpu_solve_grid(Q, D.grid(2, 40, 40, "2x1"), _options(), False, None, None, None)


# ---- the device plan ------------------------------------------------------------------------------------------------
def _plan(nat, M, N, P, spec, rank, comm_size, stop, algo=0, shift=0.0, **knobs):
    prob = EllipseProblem(M, N, stop=stop, shift=shift).to_native()
    opt = nat.SolveOptions()
    opt.algo = algo
    return nat.solver_plan(prob, nat.decompose(M, N, D.grid(P, M, N, spec), rank), comm_size, opt, **knobs)


PLAN_BLOCKS = [("single-2048", 2048, 2048, 1, "1x1", 1), ("slab-12rows", 25, 200, 2, "2x1", 2),
               ("2x2-of-25", 51, 51, 4, "2x2", 4), ("vgroup-2x2-of-25", 51, 51, 4, "2x2", 1)]


@pytest.mark.parametrize("tag,M,N,P,spec,comm", PLAN_BLOCKS, ids=[b[0] for b in PLAN_BLOCKS])
def test_plan_takes_one_iteration_per_launch(nat, tag, M, N, P, spec, comm):
    for rank in range(P):
        step = _plan(nat, M, N, P, spec, rank, comm, "step")
        res = _plan(nat, M, N, P, spec, rank, comm, "residual")
        one = _plan(nat, M, N, P, spec, rank, comm, "step", pe_steps=1)
        assert step["steps"] == 3 and step["algo"] == "three-step", (tag, step["steps"])
        assert res["steps"] == 1 and res["fused"] and res["algo"] == "fused"
        # the plan of PE_STEPS=1, field for field; a PE_STEPS of 2 or 3 is ignored
        assert res == one
        for s in (2, 3):
            assert _plan(nat, M, N, P, spec, rank, comm, "residual", pe_steps=s) == one


def test_plan_keeps_classic_and_resident(nat):
    for stop in ("step", "residual"):
        assert _plan(nat, 70, 129, 1, "1x1", 0, 1, stop, shift=40.0)["algo"] == "classic"
        assert _plan(nat, 70, 129, 1, "1x1", 0, 1, stop, algo=1)["algo"] == "classic"
        assert _plan(nat, 800, 1200, 1, "1x1", 0, 1, stop)["algo"] == "resident"
        assert _plan(nat, 800, 1200, 1, "1x1", 0, 1, stop, algo=2, pe_resident=0)["algo"] == "fused"
    assert _plan(nat, 800, 1200, 1, "1x1", 0, 1, "residual") == _plan(nat, 800, 1200, 1, "1x1", 0, 1, "step")


@pytest.mark.parametrize("algo,name", [(3, "two-step"), (4, "three-step")])
def test_plan_refuses_the_multi_step_sweeps(nat, algo, name):
    assert _plan(nat, 2048, 2048, 1, "1x1", 0, 1, "step", algo=algo)["algo"] == name
    with pytest.raises(ValueError, match="stop"):
        _plan(nat, 2048, 2048, 1, "1x1", 0, 1, "residual", algo=algo)
    # after the existing refusals: their texts come first
    with pytest.raises(ValueError, match="shift"):
        _plan(nat, 2048, 2048, 1, "1x1", 0, 1, "residual", algo=algo, shift=0.75)
    with pytest.raises(ValueError, match="-step sweep: single-rank blocks"):
        _plan(nat, 6, 6, 1, "1x1", 0, 1, "residual", algo=algo)


# ---- breakdown ------------------------------------------------------------------------------------------------------
def test_breakdown_is_relative_under_the_rule_and_absolute_without_it():
    """The step-size rule keeps the reference's |den| < 1e-15: F = 1 at 40×40 with tol = 1e-12 ends "breakdown" in
    iteration 75, as before.  Under the residual rule the same recurrence runs through that point (40x40-F, K = 76),
    and a tolerance of 1e-30 still ends in a status with finite scalars (here r reaches 0 exactly: converged)."""
    a = solve(EllipseProblem(40, 40, tol=1e-12), backend="serial")
    assert a.breakdown and not a.converged and a.iters == 75
    b = sc.serial("40x40-F")
    assert b.converged and not b.breakdown and b.iters == 76
    c = solve(EllipseProblem(40, 40, stop="residual", tol=1e-30, max_iter=400), backend="serial")
    assert not c.nonfinite and np.isfinite(c.last_diff) and (c.converged or c.breakdown or c.iters == 400)
