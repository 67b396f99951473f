"""MI355X tests of the residual stop rule, EllipseProblem(stop="residual"): the
terminal paths of the three one-iteration kernel families — classic (kF's
entry test), the single sweep (kS / kRed through sweep_term, listed and
dynamic-queue walks) and the resident kernel (the loop top) — against the
serial backend; k = 0 and the cap on each; virtual ranks and processes; a
DeviceSession's time steps; checkpoint and resume; the refusals.  Cases, gate
and bounds: stop_checks.  Every test takes seconds and fails without the
feature (EllipseProblem has no `stop`).

Not asserted: that a session keeps its captured graphs from one step to the
next.  DeviceSolver::set_rhs / set_w0 drop the cached graphs on every call (as
before this rule), so there is nothing to observe; the threshold itself is
device state and would not force a rebuild."""

import dataclasses
import json
import os
import subprocess
import sys

import field_checks as fc
import numpy as np
import pytest
import stop_checks as sc
import torch
from test_device_fields_gpu import cuda

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def hip(name, **kw):
    c = sc.CASES[name]
    return solve(c.problem(**kw.pop("prob", {})), backend="hip", return_w=True, **kw, **c.inputs())


# ---- classic: kF --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", sc.UNSHIFTED + sc.SHIFTED40 + ["70x129-s0.75"])
def test_classic(gpu, name, variant):
    rep = hip(name, algo="classic", variant=variant)
    sc.check_against_serial(f"classic v{variant}", name, rep, 1e-10, algo="classic")
    assert rep.to_dict()["stop"] == "residual"


@pytest.mark.parametrize("name", sc.SHIFTED40)
def test_auto_with_a_shift_is_classic(gpu, name):
    sc.check_against_serial("auto", name, hip(name), 1e-10, algo="classic")


# ---- the single sweep: kS, kRed -------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["0", "3"])
@pytest.mark.parametrize("name", sc.SWEEP)
def test_single_sweep(gpu, name, order, monkeypatch):
    """algo="fused" with the resident kernel off: the listed static walk (kS's own terminal write) and PE_ORDER=3, the
    dynamic queue whose terminal state kRed writes."""
    monkeypatch.setenv("PE_RESIDENT", "0")
    monkeypatch.setenv("PE_ORDER", order)
    rep = hip(name, algo="fused")
    sc.check_against_serial(f"kS order {order}", name, rep, 1e-9, algo="fused")


@pytest.mark.parametrize("name,parity", [("70x129", 1), ("65x258", 0)])
def test_single_sweep_stops_in_either_sweep(gpu, name, parity, monkeypatch):
    """K odd / K even: the test at the top of iteration K + 1 runs in an applying / in a deferring sweep — with and
    without a pending α p term to flush."""
    assert sc.gate(name)[0] % 2 == parity
    monkeypatch.setenv("PE_RESIDENT", "0")
    rep = hip(name, algo="fused")
    assert rep.iters % 2 == parity
    sc.check_against_serial(f"kS parity {parity}", name, rep, 1e-9, algo="fused")


# ---- the resident kernel --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [0, 8])
@pytest.mark.parametrize("name", sc.UNSHIFTED)
def test_resident(gpu, name, chunk, monkeypatch):
    """auto with PE_RESIDENT=1: one launch for the whole solve (the test fires mid-launch), and launches of 8
    iterations (the test fires at iteration K mod 8 of a launch; 9×130's K = 263 ends a launch's 7th)."""
    monkeypatch.setenv("PE_RESIDENT", "1")
    rep = hip(name, chunk=chunk)
    sc.check_against_serial(f"resident chunk {chunk}", name, rep, 1e-9, algo="resident")


# ---- k = 0 and the cap on each family -------------------------------------------------------------------------------
FAMILIES = [("classic", dict(algo="classic"), "0", 0.0, 1e-10), ("classic", dict(algo="classic", variant=1), "0", 40.0, 1e-10),
            ("fused", dict(algo="fused"), "0", 0.0, 1e-9), ("resident", dict(), "1", 0.0, 1e-9)]
FAMILY_IDS = ["classic", "classic-v1-s40", "kS", "resident"]


@pytest.mark.parametrize("algo,kw,resident,sigma,tol", FAMILIES, ids=FAMILY_IDS)
def test_zero_iterations(gpu, algo, kw, resident, sigma, tol, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", resident)
    prob, inputs = sc.zero_iteration_problem(40, 40, sigma)
    ref = solve(prob, backend="serial", **inputs)
    rep = solve(prob, backend="hip", return_w=True, **kw, **inputs)
    print(f"stop-zero {algo} iters={rep.iters} res_nat={rep.res_nat!r}/{ref.res_nat!r} bitwise={np.array_equal(rep.w, inputs['w0'])}")
    assert rep.algo == algo and rep.iters == 0 and rep.converged and np.array_equal(rep.w, inputs["w0"])
    assert rep.stop_thr == 1e-3 and rep.res_nat == rep.res_nat0 == pytest.approx(ref.res_nat0, rel=1e-9)


@pytest.mark.parametrize("algo,kw,resident,sigma,tol", FAMILIES, ids=FAMILY_IDS)
def test_the_cap_wins(gpu, algo, kw, resident, sigma, tol, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", resident)
    name = "40x40-s40" if sigma else "40x40"
    K = sc.gate(name)[0]
    capped = hip(name, prob=dict(max_iter=K), **kw)
    assert capped.algo == algo and capped.iters == K and not capped.converged and capped.res_nat == -1.0
    one_more = hip(name, prob=dict(max_iter=K + 1), **kw)
    sc.check_against_serial(f"{algo} cap+1", name, one_more, tol, algo=algo)
    assert np.abs(capped.w - one_more.w).max() <= tol  # (the same iterate K)


@pytest.mark.parametrize("algo,kw,resident,sigma,tol", FAMILIES, ids=FAMILY_IDS)
def test_explicit_step_rule_is_the_default(gpu, algo, kw, resident, sigma, tol, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", resident)
    M, N = 40, 40
    args = dict(backend="hip", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True, **kw)
    a, b = solve(EllipseProblem(M, N, shift=sigma), **args), solve(EllipseProblem(M, N, shift=sigma, stop="step"), **args)
    assert a.algo == b.algo == algo and a.converged and a.iters == b.iters and np.array_equal(a.w, b.w)
    assert a.last_diff == b.last_diff and "stop" not in b.to_dict() and b.res_nat == b.res_nat0 == b.stop_thr == -1.0


# ---- several ranks ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,ranks,decomp", [("26x27", 4, "2x2"), ("37x50", 3, "3x1"), ("26x27-s40", 4, "2x2"),
                                               ("37x50-s40", 3, "3x1")])
def test_virtual_ranks(gpu, name, ranks, decomp):
    """hip-group against one rank: equal iterations (a gated case), w within 1e-9; the group driver writes the
    threshold into every block's state."""
    c = sc.CASES[name]
    one = hip(name)
    rep = solve(c.problem(), backend="hip-group", ranks=ranks, decomp=decomp, return_w=True, **c.inputs())
    assert rep.algo == ("classic" if c.sigma else "fused") and one.algo in ("classic", "fused", "resident")
    sc.check_against_serial(f"one rank ({one.algo})", name, one, 1e-9)
    sc.check_against_serial(f"group {decomp} ({rep.algo})", name, rep, 1e-9)
    assert rep.iters == one.iters and np.abs(rep.w - one.w).max() <= 1e-9


@pytest.mark.parametrize("name", ["37x50", "37x50-s40"])
def test_processes_on_one_gpu(gpu, name, tmp_path):
    """Three processes, row slabs, the host-staged transport, on one GPU (stop_job.py) against serial: every rank
    reads the same reduced g_0 and sets the same threshold."""
    from conftest import free_port

    c, world = sc.CASES[name], 3
    ref = sc.serial(name)
    paths = [str(tmp_path / n) for n in ("f.npy", "g.npy")]
    for p, a in zip(paths, (fc.rhs(c.M, c.N), fc.w0(c.M, c.N))):
        np.save(p, a)
    env = dict(os.environ, PE_COMM="host", PE_HALO="exchange", PE_OVERLAP="0")
    cmd = ["timeout", "-k", "10", "240", sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node",
           str(world), "--master-addr", "127.0.0.1", "--master-port", str(free_port()),
           os.path.join(ROOT, "tests", "stop_job.py"), str(c.M), str(c.N), repr(c.sigma), repr(c.tol), repr(c.atol), *paths,
           str(tmp_path / "out"), "rows"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    W = np.full((c.M - 1, c.N - 1), np.nan)
    for r in range(world):
        with open(tmp_path / f"out.r{r}.json") as fh:
            d = json.load(fh)
        blk = np.load(tmp_path / f"out.r{r}.npy")
        i0, j0 = d["origin"]
        W[i0 - 1:i0 - 1 + blk.shape[0], j0 - 1:j0 - 1 + blk.shape[1]] = blk
        assert d["algo"] == ("classic" if c.sigma else "fused") and d["converged"] and d["iters"] == ref.iters
        assert d["Px"] == world and d["Py"] == 1 and d["stop"] == "residual"
        for key in ("res_nat", "res_nat0", "stop_thr"):
            assert d[key] == pytest.approx(getattr(ref, key), rel=1e-9), (r, key)
    print(f"stop-processes {name} dw={np.abs(W - ref.w).max():.2e}")
    assert np.abs(W - ref.w).max() <= 1e-9


# ---- a session's time steps -------------------------------------------------------------------------------------------
def test_implicit_euler_steps_in_a_session(gpu):
    """Three steps of u' = Δu + f, (A + I/dt) u⁺ = u/dt + f, in one session: the first step's res_nat0 fixes
    atol = τ·res_nat0 for the warm-started ones.  Every step is gated and equal to serial."""
    M, N, dt = 40, 40, 1.0 / 40.0
    prob = EllipseProblem(M, N, shift=1.0 / dt, stop="residual", tol=1e-6)
    f = fc.rhs(M, N)
    u_host = fc.w0(M, N)
    u, ft = cuda(u_host), cuda(f)
    atol = None
    with DeviceSession(prob) as s:
        for step in range(3):
            p = dataclasses.replace(prob, atol=atol or 0.0)
            K = sc.gate_sums(p, rhs=u_host / dt + f, w0=u_host)[0]
            ref = solve(p, backend="serial", rhs=u_host / dt + f, w0=u_host, return_w=True)
            rep = s.solve(rhs=u / dt + ft, w0=u, return_w="device", atol=atol)
            dev = float(np.abs(host(rep.w) - ref.w).max())
            print(f"stop-heat step {step} iters={rep.iters}/{ref.iters}/{K} thr={rep.stop_thr!r}/{ref.stop_thr!r} dw={dev:.2e}")
            assert rep.algo == "classic" and rep.converged and rep.iters == ref.iters == K and dev <= 1e-10
            assert rep.stop_thr == pytest.approx(ref.stop_thr, rel=1e-9) and rep.atol == (atol or 0.0)
            assert rep.res_nat == pytest.approx(ref.res_nat, rel=1e-9)
            if step == 0:
                atol = prob.tol * ref.res_nat0
            else:  # (the warm start's own tol·sqrt(g_0) lies far below the floor)
                assert rep.stop_thr == atol > prob.tol * rep.res_nat0
            u, u_host = rep.w, ref.w
        with pytest.raises(ValueError, match="atol"):
            s.solve(rhs=ft, atol=-1.0)
    with DeviceSession(EllipseProblem(M, N)) as s:
        with pytest.raises(ValueError, match="atol"):
            s.solve(atol=1e-3)


# ---- checkpoint and resume --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo,resident", [("classic", "0"), ("fused", "0"), ("auto", "1")])
def test_checkpoint_resume_bitwise(gpu, algo, resident, tmp_path, monkeypatch):
    """70×129 checkpointed mid-solve and resumed: the threshold travels in the file's state; the same iterations, the
    same bits."""
    monkeypatch.setenv("PE_RESIDENT", resident)
    name = "70x129"
    ck = str(tmp_path / "ck")
    full = hip(name, algo=algo, checkpoint=ck, checkpoint_every=100, chunk=8)
    sc.check_against_serial(f"checkpointed {algo}", name, full, 1e-9)
    assert os.path.exists(ck + ".r0")
    res = hip(name, algo=algo, resume=ck, chunk=8)
    assert res.algo == full.algo and res.converged and res.iters == full.iters and np.array_equal(res.w, full.w)
    assert (res.res_nat, res.res_nat0, res.stop_thr) == (full.res_nat, full.res_nat0, full.stop_thr)


# ---- refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algo", ["two-step", "three-step"])
def test_multi_step_sweeps_refuse(gpu, algo):
    prob = EllipseProblem(40, 40, stop="residual")
    with pytest.raises(ValueError, match="stop"):
        DeviceSession(prob, algo=algo)
    with pytest.raises(ValueError, match="stop"):
        solve(prob, backend="hip", algo=algo)
    with pytest.raises(ValueError, match="stop"):
        solve(EllipseProblem(51, 51, stop="residual"), backend="hip-group", ranks=4, decomp="2x2", algo="three-step")
    with DeviceSession(EllipseProblem(40, 40), algo=algo) as s:  # (the step-size rule: the layout exists as ever)
        assert s.solve().converged


def test_auto_beyond_the_resident_kernel_is_the_single_sweep(gpu, monkeypatch):
    """Where auto takes the three-step sweep today, the rule takes kS — PE_STEPS ignored."""
    monkeypatch.setenv("PE_RESIDENT", "0")
    monkeypatch.setenv("PE_STEPS", "3")
    assert solve(EllipseProblem(70, 129, max_iter=6), backend="hip").algo == "three-step"
    sc.check_against_serial("auto", "70x129", hip("70x129"), 1e-9, algo="fused")


def test_native_program(gpu):
    """bin/pe_hip --stop residual --atol X: the built-in problem at 40×40 with σ = 40 and τ = 1e-4 (gated) against serial."""
    exe = os.path.join(ROOT, "bin", "pe_hip")
    assert os.path.exists(exe), "pe_hip is not built"
    prob = EllipseProblem(40, 40, shift=40.0, stop="residual", tol=1e-4, atol=1e-12)
    K = sc.gate_sums(prob)[0]
    ref = solve(prob, backend="serial")
    out = subprocess.run(["timeout", "-k", "10", "120", exe, "--stop", "residual", "--tol", "1e-4", "--atol", "1e-12",
                          "--shift", "40", "--json", "--quiet", "40", "40"], capture_output=True, text=True, check=True).stdout
    d = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
    assert d["iters"] == ref.iters == K and d["converged"] and d["algo"] == "classic"
    assert d["stop"] == "residual" and d["atol"] == 1e-12
    for key in ("res_nat", "res_nat0", "stop_thr"):
        assert d[key] == pytest.approx(getattr(ref, key), rel=1e-9), key
    plain = subprocess.run(["timeout", "-k", "10", "120", exe, "--json", "--quiet", "40", "40"], capture_output=True,
                           text=True, check=True).stdout
    assert '"stop"' not in plain and '"atol"' not in plain
    bad = subprocess.run([exe, "--atol", "1e-3", "40", "40"], capture_output=True, text=True)
    assert bad.returncode == 2 and "atol" in bad.stderr


@pytest.mark.parametrize("K", [20, 21])
def test_forced_breakdown_under_the_rule(gpu, K, monkeypatch):
    """The rule's breakdown test is |den| ≤ 1e-15·|g| (cg_breakdown): den = 0 (PE_FAULT_INJECT=zero@iter:K zeroes the
    (p, A p) sums of sweep K) still stops the solve at iteration K + 1 before its update, in a deferring and in an
    applying sweep, with w that of a run capped at K — test_gpu.test_forced_breakdown_terminal_path under the rule."""
    c = sc.CASES["70x129"]
    monkeypatch.setenv("PE_RESIDENT", "0")
    monkeypatch.setenv("PE_FAULT_INJECT", f"zero@iter:{K}")
    brk = hip("70x129", algo="fused")
    assert brk.breakdown and not brk.converged and brk.iters == K + 1 and brk.res_nat == -1.0
    monkeypatch.delenv("PE_FAULT_INJECT")
    ref = hip("70x129", algo="fused", prob=dict(max_iter=K))
    assert ref.iters == K and np.abs(brk.w - ref.w).max() <= 1e-15 * np.abs(ref.w).max()
