"""MI355X tests of the four marching sweeps — kS3, kS2, kS and kResident — and
of the end-of-solve kernels on members of the ellipse family that cut, cover
or sit off-centre in the box (sweep_checks.FAMILY), against the PyTorch fp64
recurrence.  On the reference problem, the circle and the wide ellipse the
ellipse meets the box in a point at the most, so a node with interior
coefficients (face 1, 1/D = dinv_in) never sits next to a box-boundary column,
a padding column past ny or a halo row outside the global interior, and every
three-step item of the edge shapes is a band item.  Here they do: the uniform
march of kS3 on edge strips (its per-lane mask of z, the row scalars of rows
outside the interior), the band-free rows' select between 1 and 1/ε in kS2, kS
and kResident at the first and last columns and rows, and the same through
block seams on virtual ranks.

The shapes, counts, comparison and tolerances are those of test_sweep_edges.py
(sweep_checks.check_sweeps, KINDS); test_oracle.py holds every reference used
here to the others ten times tighter without a device, and
test_item_layout.py pins, from the host planner, the item kinds the three-step
cases are there for — asserted here again from the live solver's list.

One converged solve per member, grid and sweep then checks kResid / kError
against fp64 from the returned w (norm_checks.check_norms), the iteration
count against the serial backend's and w against its w."""

import functools

import halo_checks
import norm_checks
import numpy as np
import pytest
import sweep_checks
from sweep_checks import FAMILY, SHORT_GRID, SHORT_MEMBERS

from poisson_ellipse_openmp_mpi_cuda_amd import solve

pytestmark = pytest.mark.gpu
THREE = "three-step"


def _cases(shapes):
    return [(m,) + c for m in FAMILY for c in (shapes(m) if callable(shapes) else shapes)]


@pytest.mark.parametrize("member,M,N,J", _cases(sweep_checks.family_three))
def test_three_step_family(gpu, nat, member, M, N, J):
    s = sweep_checks.solver(nat, M, N, "three", member)
    kinds = sweep_checks.check_item_kinds(s.layout_entries, M, N, member)
    print(f"item-kinds {member} {M}x{N} ti={s.ti} {s.layout_name} {sorted(kinds)}")
    sweep_checks.check_sweeps(s, M, N, "three", J, member)


@pytest.mark.parametrize("layout", sweep_checks.SHORT_THREE[2])
@pytest.mark.parametrize("ti", sweep_checks.SHORT_THREE[1])
@pytest.mark.parametrize("member", SHORT_MEMBERS)
def test_three_step_family_short_items(gpu, nat, member, ti, layout, monkeypatch):
    """Uniform items of 4, 7 and 13 rows on edge strips: all fill and drain
    (4, 7) and one steady group between them (13)."""
    M, N = SHORT_GRID
    monkeypatch.setenv("PE_TI", str(ti))
    monkeypatch.setenv("PE_LAYOUT", layout)
    s = sweep_checks.solver(nat, M, N, "three", member)
    assert s.ti == ti and s.layout_name == layout
    sweep_checks.check_item_kinds(s.layout_entries, M, N, member)
    sweep_checks.check_sweeps(s, M, N, "three", sweep_checks.SHORT_THREE[0], member)


@pytest.mark.parametrize("member,M,N,J", _cases(sweep_checks.TWO_EDGES))
def test_two_step_family(gpu, nat, member, M, N, J):
    s = sweep_checks.solver(nat, M, N, "two", member)
    assert s.two_step
    sweep_checks.check_sweeps(s, M, N, "two", J, member)


@pytest.mark.parametrize("ti", sweep_checks.SHORT_TWO[1])
@pytest.mark.parametrize("member", SHORT_MEMBERS)
def test_two_step_family_short_items(gpu, nat, member, ti, monkeypatch):
    M, N = SHORT_GRID
    monkeypatch.setenv("PE_TI", str(ti))
    s = sweep_checks.solver(nat, M, N, "two", member)
    assert s.two_step and s.ti == ti
    sweep_checks.check_sweeps(s, M, N, "two", sweep_checks.SHORT_TWO[0], member)


@pytest.mark.parametrize("member,M,N,K", _cases(sweep_checks.SINGLE_EDGES))
def test_single_sweep_family(gpu, nat, member, M, N, K, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", "0")
    s = sweep_checks.solver(nat, M, N, "single", member)
    assert not s.resident
    sweep_checks.check_sweeps(s, M, N, "single", K, member)


@pytest.mark.parametrize("ti", sweep_checks.SHORT_SINGLE[1])
@pytest.mark.parametrize("member", SHORT_MEMBERS)
def test_single_sweep_family_short_items(gpu, nat, member, ti, monkeypatch):
    M, N = SHORT_GRID
    monkeypatch.setenv("PE_TI", str(ti))
    monkeypatch.setenv("PE_RESIDENT", "0")
    s = sweep_checks.solver(nat, M, N, "single", member)
    assert not s.resident and s.ti == ti
    sweep_checks.check_sweeps(s, M, N, "single", sweep_checks.SHORT_SINGLE[0], member)


@pytest.mark.parametrize("member,M,N,K", _cases(sweep_checks.SINGLE_EDGES))
def test_resident_family(gpu, nat, member, M, N, K, monkeypatch):
    monkeypatch.setenv("PE_RESIDENT", "1")
    s = sweep_checks.solver(nat, M, N, "single", member)
    assert s.resident
    sweep_checks.check_sweeps(s, M, N, "single", K, member)


@pytest.mark.parametrize("M,N,ranks,decomp,K,expect,member", halo_checks.FAMILY_VIRTUAL,
                         ids=[f"{v[6]}-{v[0]}x{v[1]}-{v[3]}-K{v[4]}" for v in halo_checks.FAMILY_VIRTUAL])
def test_virtual_ranks_family(gpu, M, N, ranks, decomp, K, expect, member):
    """2x2 virtual ranks: 12×12 blocks and 13/12 rows × 49 columns (a
    one-column last strip in front of an UP neighbour) on the three-step sweep,
    11×11 blocks on the single sweep — seams through interior-coefficient
    nodes that reach the box edge."""
    halo_checks.check_virtual(M, N, ranks, decomp, K, expect, member)


# ---- converged solves: kResid, kError, the stop iteration and w -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def _serial(member, M, N):
    rep = solve(sweep_checks.problem(M, N, member), backend="serial", return_w=True, keep_history=True)
    assert rep.converged and len(rep.history) == rep.iters >= 2
    rep.w.setflags(write=False)
    return rep


def _stop_is_decided(prob, ref):
    """shift_checks.stop_margin's rule: ‖Δw‖ is not within 1e-3·δ of δ at the serial solve's last two iterations."""
    return all(abs(d - prob.tol) > 1e-3 * prob.tol for d in ref.history[-2:])


@pytest.mark.parametrize("algo", ["fused", "two-step", THREE, "classic"])
@pytest.mark.parametrize("M,N", [(66, 49), SHORT_GRID])
@pytest.mark.parametrize("member", list(FAMILY))
def test_end_of_solve_family(gpu, member, M, N, algo, monkeypatch):
    """A converged solve (19 to 154 iterations) per member and sweep: the
    report's residual and error figures against fp64 from its own w, at
    check_norms' bounds (the classic path reports no residual: its error
    figures at the same 1e-12); the iteration count equal to the serial
    backend's where its stop test is decided by more than 1e-3·δ, else within
    one; w within 1e-9 of the serial w (classic: 1e-10, its bound in
    test_shift_gpu.py).  On the cut members u_exact is not the solution; the
    error figures are still the same expression of the same w on both sides."""
    if algo == "fused":
        monkeypatch.setenv("PE_RESIDENT", "0")
    prob = sweep_checks.problem(M, N, member)
    ref = _serial(member, M, N)
    rep = solve(prob, backend="hip", algo=algo, return_w=True)
    assert rep.algo == algo and rep.converged
    slack = 0 if _stop_is_decided(prob, ref) else 1
    dw = float(np.abs(rep.w - ref.w).max())
    print(f"family-solve {member} {M}x{N} {algo} iters={rep.iters} serial={ref.iters} slack={slack} dw={dw:.2e}")
    got = {k: getattr(rep, k) for k in ("res_true", "b_norm", "l2_err", "max_err", "max_outside", "res_rec", "res_gap")}
    if algo == "classic":
        want = norm_checks.fp64_norms(prob, rep.w)
        print(f"norm-dev {member} {M}x{N} classic l2_err={abs(got['l2_err'] - want['l2_err']) / want['l2_err']:.2e} "
              f"max_err={abs(got['max_err'] - want['max_err']) / want['max_err']:.2e}")
        assert got["res_true"] == -1.0
        assert got["l2_err"] == pytest.approx(want["l2_err"], rel=1e-12)
        assert got["max_err"] == pytest.approx(want["max_err"], rel=1e-12)
    else:
        norm_checks.check_norms(f"{member} {M}x{N} {algo}", prob, got, rep.w, algo == THREE)
    assert abs(rep.iters - ref.iters) <= slack, (rep.iters, ref.iters)
    assert dw <= (1e-10 if algo == "classic" else 1e-9), dw
