"""The cases, the gate and the references of test_stop_rule.py /
test_stop_rule_gpu.py: the residual stop rule, EllipseProblem(stop="residual",
tol=τ, atol=a) — iterate k is tested at the top of iteration k + 1,
sqrt(g_k) ≤ thr = max(τ·sqrt(g_0), a) with g_k = h1·h2·Σ z_k·r_k.

The gate.  (r, z) is not monotone, and a backend's g differs from another's in
the last bits, so a stop decision is only compared where it is no coin toss:
gate() takes the sums of the fp64 reference recurrence (torch_ref.classic, with
the case's shift, rhs and w0), finds K = the first k with sqrt(g_k) ≤ thr and
asserts |sqrt(g_k) − thr| > 1e-3·thr for EVERY k ≤ K — shift_checks.stop_margin's
margin applied to every iterate the rule tests.  Every test uses gated cases only.

Bounds (none taken from the code under test):
  serial vs the torch recurrence after K iterations: |w − w_ref| ≤ 1e-9
      (test_oracle.py's serial-vs-torch bound), res_nat to rel 1e-9;
  omp / ranks / dist-cpu / torch vs serial: equal iterations, |w − w_ref| ≤ 1e-9;
  hip vs serial: equal iterations, |w − w_ref| ≤ 1e-10 classic, 1e-9 the sweeps
      (test_sweep_family.py's), res_nat / res_nat0 to rel 1e-9;
  hip-group / processes vs one rank or serial: equal iterations (gated), 1e-9."""

import dataclasses
import functools
import math

import field_checks as fc
import numpy as np
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    sigma: float = 0.0
    tol: float = 1e-6
    fields: bool = True          # field_checks' rhs and w0 (False: F and the zero start)
    member: str = ""             # a sweep_checks.FAMILY member ("" the reference ellipse)
    atol: float = 0.0
    K: int = -1                  # the stopping iterate where the cases' table pins it (-1: the gate's)

    def problem(self, **more):
        kw = dict(sweep_checks.FAMILY[self.member]) if self.member else {}
        kw.update(shift=self.sigma, tol=self.tol, stop="residual", atol=self.atol)
        kw.update(more)
        return EllipseProblem(self.M, self.N, **kw)

    def inputs(self):
        return dict(rhs=fc.rhs(self.M, self.N), w0=fc.w0(self.M, self.N)) if self.fields else {}


# K: the fp64 recurrence's, checked with the gate's own loop (worst margins 1.1e-2 .. 7.2e-2 of thr)
CASES = {c.name: c for c in [
    # 40x40-F: thr = 2.2e-8 lies below sqrt(1e-15) — g_74 = 1.3e-15, and (Ap, p) of iteration 75 is under the
    # step-size rule's absolute breakdown bound 1e-15.  The residual rule's breakdown test is relative to g
    # (pe/fields.hpp cg_breakdown), so the solve goes on to K = 76; with the absolute test it ended "breakdown"
    # with iters = 75.
    Case("40x40-F", 40, 40, fields=False, K=76),
    Case("40x40-s40", 40, 40, sigma=40.0, K=64),
    Case("70x129", 70, 129, K=251),
    Case("70x129-s0.75", 70, 129, sigma=0.75, K=250),
    Case("9x130-s40", 9, 130, sigma=40.0, K=181),
    Case("65x258", 65, 258, tol=1e-4, K=282),
    # further cases through the same gate: the unshifted 40×40 and 9×130 with field_checks' fields (the
    # single-sweep kernels refuse a shift), σ = 40 at the two larger shapes
    Case("40x40", 40, 40),
    Case("9x130", 9, 130),
    Case("70x129-s40", 70, 129, sigma=40.0),
    Case("65x258-s40", 65, 258, sigma=40.0, tol=1e-4),
    # the multi-rank shapes of test_shift_gpu.py (2×2 of 26×27, three row slabs of 37×50)
    Case("26x27", 26, 27),
    Case("26x27-s40", 26, 27, sigma=40.0),
    Case("37x50", 37, 50),
    Case("37x50-s40", 37, 50, sigma=40.0),
    # two family members at 66×49 through the same gate (both pass the margin at tol = 1e-6: no move)
    Case("cover-66x49", 66, 49, member="cover"),
    Case("cut_y-66x49", 66, 49, member="cut_y"),
]}
TABLE = ["40x40-F", "40x40-s40", "70x129", "70x129-s0.75", "9x130-s40", "65x258"]  # the issue's table
UNSHIFTED = ["40x40-F", "40x40", "9x130", "70x129", "65x258"]            # σ = 0 at the four shapes
SHIFTED40 = ["40x40-s40", "9x130-s40", "70x129-s40", "65x258-s40"]       # σ = 40 at the four shapes
SWEEP = UNSHIFTED + ["cover-66x49", "cut_y-66x49"]


def g0(prob, rhs=None, w0=None):
    """g_0 = h1·h2·Σ z⁰·r⁰ in fp64, with torch_ref.classic's own start."""
    a, b, B = torch_ref.assemble(prob, "cpu", rhs=rhs)
    h1, h2 = prob.h1, prob.h2
    D = torch_ref.diag(a, b, h1, h2, prob.shift)
    w = torch_ref.embed(prob, w0, "cpu") if w0 is not None else B * 0.0
    r = B - torch_ref.apply_A(w, a, b, h1, h2, prob.shift)
    r[0, :] = r[-1, :] = 0
    r[:, 0] = r[:, -1] = 0
    z = torch_ref.apply_Dinv(r, D)
    return float((z[1:-1, 1:-1] * r[1:-1, 1:-1]).sum()) * h1 * h2


def gate_sums(prob, rhs=None, w0=None, limit=1200):
    """(K, thr, [sqrt(g_0) .. sqrt(g_K)]) of the fp64 recurrence, the margin
    asserted at every tested iterate.  The recurrence is run in growing
    stretches (it has no stop test of its own)."""
    nat = [math.sqrt(g0(prob, rhs, w0))]
    thr = max(prob.tol * nat[0], prob.atol)
    n = 0
    while not any(v <= thr for v in nat):
        n = 100 if n == 0 else 2 * n
        assert n <= limit, (prob.M, prob.N, "the fp64 recurrence does not meet the rule")
        st = torch_ref.classic(prob, n, rhs=rhs, w0=w0)
        hh = prob.h1 * prob.h2
        nat = nat[:1] + [math.sqrt(s[2] * hh) for s in st.sums]
    K = next(k for k, v in enumerate(nat) if v <= thr)
    for k in range(K + 1):
        assert abs(nat[k] - thr) > 1e-3 * thr, (prob.M, prob.N, prob.shift, k, nat[k], thr)
    return K, thr, nat[:K + 1]


@functools.lru_cache(maxsize=None)
def gate(name):
    """The gate of a named case: (K, thr, sqrt(g_0..K)); computed once."""
    c = CASES[name]
    K, thr, nat = gate_sums(c.problem(), **c.inputs())
    worst = min(abs(v - thr) / thr for v in nat)
    print(f"stop-gate {name} K={K} thr={thr:.6e} worst-margin={worst:.2e}")
    assert c.K < 0 or K == c.K, (name, K, c.K)
    return K, thr, tuple(nat)


@functools.lru_cache(maxsize=None)
def torch_state(name):
    """torch_ref.classic after the gate's K iterations (the w the rule returns)."""
    c = CASES[name]
    return torch_ref.classic(c.problem(), gate(name)[0], **c.inputs())


@functools.lru_cache(maxsize=None)
def serial(name):
    """The serial solve of a gated case under the rule; computed once, read-only."""
    c = CASES[name]
    gate(name)
    rep = solve(c.problem(), backend="serial", return_w=True, **c.inputs())
    rep.w.setflags(write=False)
    return rep


def check_against_serial(tag, name, rep, w_tol, algo=None):
    """A backend's report of a gated case against the serial one: converged, equal
    iterations, w within w_tol, res_nat / res_nat0 / stop_thr to rel 1e-9.
    Prints the deviations, then asserts."""
    ref = serial(name)
    w = rep.w.cpu().numpy() if hasattr(rep.w, "cpu") else np.asarray(rep.w)
    dw = float(np.abs(w - ref.w).max())
    print(f"stop-dev {tag} {name} iters={rep.iters}/{ref.iters} dw={dw:.2e} res_nat={rep.res_nat!r}/{ref.res_nat!r} "
          f"res_nat0={rep.res_nat0!r}/{ref.res_nat0!r} algo={rep.algo}")
    if algo is not None:
        assert rep.algo == algo, (tag, rep.algo)
    assert rep.converged and rep.iters == ref.iters == gate(name)[0], (tag, rep.iters, ref.iters)
    assert dw <= w_tol, (tag, dw)
    for key in ("res_nat", "res_nat0", "stop_thr"):
        got, want = getattr(rep, key), getattr(ref, key)
        assert want > 0 and abs(got - want) <= 1e-9 * want, (tag, key, got, want)


@functools.lru_cache(maxsize=None)
def tight_w(M, N, sigma):
    """A w0 that already meets a loose rule: the serial solve of field_checks' problem to τ = 1e-7 (a tighter one runs into the absolute breakdown test |(Ap, p)| < 1e-15 first)."""
    prob = EllipseProblem(M, N, shift=sigma, stop="residual", tol=1e-7)
    rep = solve(prob, backend="serial", rhs=fc.rhs(M, N), w0=fc.w0(M, N), return_w=True)
    assert rep.converged
    rep.w.setflags(write=False)
    return rep.w


def zero_iteration_problem(M, N, sigma):
    """(prob, inputs) of the k = 0 case: w0 = tight_w, atol = 1e-3 — gated: K = 0 with the margin."""
    prob = EllipseProblem(M, N, shift=sigma, stop="residual", tol=1e-6, atol=1e-3)
    inputs = dict(rhs=fc.rhs(M, N), w0=tight_w(M, N, sigma))
    K, thr, nat = gate_sums(prob, **inputs)
    assert K == 0 and thr == 1e-3, (K, thr, nat)
    return prob, inputs
