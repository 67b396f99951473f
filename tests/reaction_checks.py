"""The inputs, references and comparisons of test_reaction.py /
test_reaction_gpu.py: the reaction field c of −Δu + c(x, y)·u = f,
(A + diag(c)) w = B with the preconditioner D + c (csrc/include/pe/fields.hpp).

The test field is deterministic, c_ij = 40·(0.5 + 0.5·sin(1.3 i + 0.7 j)) at
node (i, j): non-constant in both directions, not symmetric under i ↔ j or a
reflection, non-zero outside the ellipse, up to ≈ 40, with two patches of exact
zeros — rows 2-3 × columns 3-5, and rows 1-2 × columns 129-130 where the grid
has them (the seam of 129 / 128 column blocks: an owned zero next to a ring
zero).  Right-hand side and initial guess are field_checks.rhs / w0.

Grids are M×N, the interior nx×ny = (M−1)×(N−1).  The classic walk: strips of
128 columns, 2 per lane (lane l owns c0 = j0 + 2l and c1 = c0 + 1), items of 8
rows, segments of 60 rows.

Bounds (none taken from the code under test):
  constant field vs shift on the CPU: the same bits (one expression tree);
  serial vs torch_ref.pcg: equal iterations, |w − w_ref| ≤ 1e-9 (test_shift.py's);
  torch_ref.classic vs the capped loop and serial: 1e-13·max|w| (test_classic_oracle.py's);
  residual / operator fields 1e-13·max|ref|, sums rel 1e-12 (operator_checks');
  device planes after K iterations: sweep_checks.KINDS["single"] — 1e-12 of the
  plane's maximum, sums rel 1e-10 / abs 1e-13·scale, α and β rel 1e-12;
  gathered w of several ranks 1e-12·max|w_ref|; converged device solves: equal
  iterations, |w − w_serial| ≤ 1e-10 (test_shift_gpu.py's).
A stop decision is compared only where it is no coin toss: stop_margin()."""

import functools

import classic_checks as cc
import field_checks as fc
import numpy as np
import pytest
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem, solve
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

SIGMAS = (0.75, 40.0)
K = cc.K
_, _, _, S_REL, S_ABS, AB_REL, F_TOL = sweep_checks.KINDS["single"]

# One rank, node for node: (M, N, K, member).  9×9 the smallest grid; 130×9 seventeen items down one strip; M = 10 with
# 126 .. 257 interior columns: the last lane owning both columns, c0 only (127), a full strip (128), a one-column
# second strip (129), two strips and hL / hR from owned columns (256, 257); cover: uniform rows only; cut_xy: band
# rows at the box edge.
EDGES = [(9, 9, 4, None), (130, 9, K, None)] + [(10, n, K, None) for n in (127, 128, 129, 130, 257, 258)]
FAMILY = [(10, 130, K, "cover"), (66, 130, K, "cut_xy")]
FORCED_GRID = (131, 130, K, None)  # 130 rows
FORCED_TI = ("1", "61", "130")
VIRTUAL = cc.VIRTUAL
PROCESSES = (37, 130, 3, "rows")
# converged solves: (M, N) — stop_margin() holds for each
SOLVES = [(40, 40), (37, 130)]


@functools.lru_cache(maxsize=None)
def field(M, N):
    """The test field of an M×N grid, read-only."""
    i = np.arange(1, M, dtype=np.float64)[:, None]
    j = np.arange(1, N, dtype=np.float64)[None, :]
    c = 40.0 * (0.5 + 0.5 * np.sin(1.3 * i + 0.7 * j))
    c[1:3, 2:5] = 0.0
    if N - 1 >= 130:
        c[0:2, 128:130] = 0.0
    c.setflags(write=False)
    return c


def problem(M, N, member=None, **more):
    return EllipseProblem(M, N, **(sweep_checks.FAMILY[member] if member else {}), **more)


def fields(M, N, on=True):
    return dict(rhs=fc.rhs(M, N), w0=fc.w0(M, N)) if on else {}


@functools.lru_cache(maxsize=None)
def reference(M, N, k, member=None):
    """torch_ref.classic with the test field after k iterations; computed once, never modified."""
    return torch_ref.classic(problem(M, N, member), k, reaction=field(M, N), **fields(M, N))


def _references():
    out = set(EDGES) | set(FAMILY) | {FORCED_GRID}
    out |= {(M, N, K, None) for M, N, _, _ in VIRTUAL}
    out.add(PROCESSES[:2] + (K, None))
    return sorted(out, key=lambda c: (c[3] or "",) + c[:3])


REFERENCES = _references()


@functools.lru_cache(maxsize=None)
def _serial(M, N, tol, stop, f32):
    c = field(M, N).astype(np.float32).astype(np.float64) if f32 else field(M, N)
    rep = solve(EllipseProblem(M, N, tol=tol, stop=stop), backend="serial", return_w=True, keep_history=True,
                reaction=c, **fields(M, N))
    rep.w.setflags(write=False)
    return rep


def serial(M, N, tol=1e-6, stop="step", f32=False):
    """The serial solve with the test field (f32: rounded to float32 first); computed once, read-only."""
    return _serial(M, N, tol, stop, bool(f32))


def stop_margin(M, N, tol=1e-6, f32=False):
    """Asserts on the CPU, with the reference loop alone, that the step-size
    stop test of this case is no coin toss — the last two step sizes further
    than 1e-3·tol from tol — and returns the serial solve."""
    c = field(M, N).astype(np.float32).astype(np.float64) if f32 else field(M, N)
    t = torch_ref.pcg(EllipseProblem(M, N, tol=tol), keep_history=True, reaction=c, **fields(M, N))
    assert t.converged and len(t.history) == t.iters >= 2
    for d in t.history[-2:]:
        assert abs(d - tol) > 1e-3 * tol, (M, N, t.history[-2:])
    assert t.history[-1] < tol <= t.history[-2]
    ref = serial(M, N, tol, "step", f32)
    assert ref.converged and ref.iters == t.iters
    return ref


def solver(nat, M, N, variant=0, member=None, c=None):
    """A single-rank classic solver of the reaction problem (convergence test off) with rhs, w0 and the field set."""
    opt = nat.SolveOptions()
    opt.algo = 0
    opt.variant = variant
    opt.check_tol = False
    blk = D.block(M, N, 1, 0)
    s = nat.DeviceSolver(problem(M, N, member, reaction=True).to_native(), blk, None, opt)
    fc.set_fields(nat, s, M, N, fc.rhs(M, N), fc.w0(M, N))
    s.set_reaction(nat.block_field(M, N, blk, field(M, N) if c is None else c, 1))
    return s


def check_single(nat, M, N, k, variant, member=None, ti=None):
    """classic_checks.check_single with the field: k iterations of the FIELD
    kF + kG on one rank against the reference loop — r, p_k, w, the three sums,
    α, β.  Prints the deviations ("reaction-dev"), then asserts."""
    s = solver(nat, M, N, variant, member)
    assert not s.fused and s.user_rhs and s.user_w0
    if ti is not None:
        assert s.ti == ti, (s.ti, ti)
    s.reset()
    s.run_iterations(k, False)
    s.synchronize()
    st = s.state()
    ref = reference(M, N, k, member)
    par = (k - 1) & 1
    got = {"r": s.field(0)[1:M, 1:N], "p": s.field(2 + par)[1:M, 1:N], "w": s.w()}
    want = {name: getattr(ref, name)[1:M, 1:N].numpy() for name in got}
    dev = {name: float(np.abs(got[name] - want[name]).max() / np.abs(want[name]).max()) for name in got}
    sums_got = list(st["red_F"]) + [st["red_G"]]
    sums_want = ref.sums[-1]
    scale = max(abs(x) for x in sums_want)
    dev["sums"] = max(abs(g - x) / max(abs(x), S_ABS / S_REL * scale) for g, x in zip(sums_got, sums_want))
    dev["alpha"] = abs(st["alpha"] - ref.alpha[-1]) / abs(ref.alpha[-1])
    dev["beta"] = abs(st["beta"] - ref.beta[-1]) / abs(ref.beta[-1])
    print(f"reaction-dev {M}x{N}{' ' + member if member else ''} K={k} v{variant} ti={s.ti} "
          + " ".join(f"{n}={v:.2e}" for n, v in dev.items()))
    assert st["iter"] == k and st["status"] == 0, (st["iter"], st["status"])
    for n, (g, x) in enumerate(zip(sums_got, sums_want)):
        assert g == pytest.approx(x, rel=S_REL, abs=S_ABS * scale), n
    assert st["alpha"] == pytest.approx(ref.alpha[-1], rel=AB_REL)
    assert st["beta"] == pytest.approx(ref.beta[-1], rel=AB_REL)
    for name in got:
        np.testing.assert_allclose(got[name], want[name], rtol=0, atol=F_TOL * np.abs(want[name]).max(), err_msg=name)
    return dev


def check_w(tag, w, M, N):
    """A gathered w after K iterations against the whole-grid loop at 1e-12·max|w_ref|."""
    want = reference(M, N, K).w[1:M, 1:N].numpy()
    assert w.shape == want.shape, (tag, w.shape)
    dev = float(np.abs(w - want).max() / np.abs(want).max())
    print(f"reaction-dev {tag} w={dev:.2e}")
    assert dev <= F_TOL, (tag, dev)
    return dev
