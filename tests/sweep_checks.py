"""The comparison of a marching sweep kernel with the PyTorch fp64 recurrence
(ops/torch_ref.py), shared by the MI355X tests of the sweeps (test_gpu.py,
test_two_step.py, test_three_step.py, test_sweep_edges.py,
test_sweep_family.py), the edge shapes of test_sweep_edges.py and the family
members of test_sweep_family.py, which the CPU test of the references
(test_oracle.py) walks too.

Grids are M×N, the interior (M−1)×(N−1).  A case is (M, N, count): count
sweeps of the multi-step kernels, count iterations of the single sweep.  The
counts keep the iterate far from convergence (the moment forms' own rounding
would otherwise decide the comparison): 9×9 converges in 12 iterations, hence
its short counts."""

import functools

import numpy as np
import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

# kind -> (SolveOptions.algo, iterations per sweep, reduced sums, sums rel / abs·scale, α β rel, fields and w)
KINDS = {
    "three": (4, 3, 19, 1e-9, 1e-12, 1e-11, 1e-11),
    "two": (3, 2, 20, 1e-9, 1e-12, 1e-11, 1e-11),
    "single": (2, 1, 7, 1e-10, 1e-13, 1e-12, 1e-12),
}

# Strips: 48 output columns (kS3), 120 (kS2), 124 (kS, kResident); default rows per item of a small block 48 / 24 / 10.
THREE_EDGES = [
    (15, 48, 8),    # 47 columns: one strip, one column short
    (9, 49, 8),     # 48 columns: exactly one full strip, 8 rows
    (10, 50, 8),    # 49 columns: a second strip with one output column
    (9, 97, 8),     # 96 columns: two full strips
    (14, 98, 8),    # 97 columns
    (66, 49, 8),    # 65 rows at 48 rows per item: a 17-row last item
    (700, 9, 8),    # tall, 8 columns
    (9, 1000, 8),   # 8 rows, 21 strips
    (9, 9, 2),      # the 8×8 minimum the constructor accepts
]
TWO_EDGES = [
    (9, 121, 6),    # 120 columns: exactly one full strip
    (10, 122, 6),   # 121 columns
    (9, 49, 6),
    (700, 9, 6),
    (9, 1000, 6),
    (9, 9, 3),
]
SINGLE_EDGES = [
    (9, 125, 20),   # 124 columns: exactly one full strip
    (10, 126, 20),  # 125 columns
    (34, 250, 20),  # 249 = 2·124 + 1 columns
    (700, 9, 20),
    (9, 1000, 20),
    (9, 9, 6),
]

# Short items: 129 rows × 96 columns at forced rows per item (PE_TI).  4 is the
# constructor's lower clamp for the multi-step sweeps, 2 relayout's; 7 and 13
# straddle kS3's pipeline depth and its six-step unrolled group.
SHORT_GRID = (130, 97)
SHORT_THREE = (8, [4, 7, 13], ["equal", "lpt", "fill"])
SHORT_TWO = (6, [4, 5, 9])
SHORT_SINGLE = (20, [2, 5])

# every (kind, M, N, count) whose reference a MI355X test compares a kernel with
REFERENCE_CASES = ([("three",) + c for c in THREE_EDGES] + [("two",) + c for c in TWO_EDGES]
                   + [("single",) + c for c in SINGLE_EDGES]
                   + [("three",) + SHORT_GRID + (SHORT_THREE[0],), ("two",) + SHORT_GRID + (SHORT_TWO[0],),
                      ("single",) + SHORT_GRID + (SHORT_SINGLE[0],)])


# Members of the family beyond the reference one (None): name -> EllipseProblem keyword arguments.  On the
# reference member, the circle and the wide ellipse the ellipse meets the box in a point at the most; on these,
# nodes with interior coefficients sit at the box edge, next to padding columns and next to halo rows.
FAMILY = {
    "cover": dict(cx=0.25, cy=0.5),                   # the ellipse contains the box: no band, every item uniform
    "cut_y": dict(cy=1.0),                            # the unit circle in |y| ≤ 0.6: cut by the first and last columns
    "cut_xy": dict(cx=0.5, cy=1.5),                   # only the box corners outside (M ≤ 10: the same nodes as cover)
    "offc": dict(A1=-0.4, B1=1.6, A2=-0.3, B2=0.9),   # the reference ellipse off-centre: cut by row 1 and column 1
    "tiny": dict(cx=30.0, cy=30.0),                   # almost all exterior, isolated inside nodes
}
SHORT_MEMBERS = ["cover", "cut_y", "offc"]  # (tiny converges at 130×97 in 19 iterations: under the short grid's counts)


def problem(M, N, member=None):
    return EllipseProblem(M, N, **(FAMILY[member] if member else {}))


def family_three(member):
    """The member's three-step cases: the edge shapes (cut_xy from M > 10) and five strips of 40 rows."""
    return [c for c in THREE_EDGES if member != "cut_xy" or c[0] > 10] + [(40, 200, 8)]


# every (kind, M, N, count, member) of the family that test_sweep_family.py compares a kernel with
FAMILY_REFERENCE_CASES = (
    [("three",) + c + (m,) for m in FAMILY for c in family_three(m)]
    + [("two",) + c + (m,) for m in FAMILY for c in TWO_EDGES]
    + [("single",) + c + (m,) for m in FAMILY for c in SINGLE_EDGES]
    + [(kind,) + SHORT_GRID + (short[0], m) for m in SHORT_MEMBERS
       for kind, short in (("three", SHORT_THREE), ("two", SHORT_TWO), ("single", SHORT_SINGLE))])


BAND_BIT, UNI_BIT = 1 << 30, 1 << 29  # item_layout.hpp kBandBit, kUniBit


def item_kinds(entries, N):
    """The kinds of a single-rank three-step item list, (first row, rows, strip,
    flags) per position: "band" / "uni" / "mixed" + "-edge" where the strip's
    64-column window (from column 48·strip − 7) holds a box-boundary or padding
    column — there the uniform march masks z per lane — else "-inner"."""
    kinds = set()
    for _, rows, strip, flags in entries:
        if rows:
            J = 48 * strip - 7
            kinds.add(("band" if flags & BAND_BIT else "uni" if flags & UNI_BIT else "mixed")
                      + ("-inner" if J >= 1 and J + 63 <= N - 1 else "-edge"))
    return kinds


def check_item_kinds(entries, M, N, member):
    """What a three-step family case is there for, from its item list: cover at
    66×49 and on the short-item grid is uniform items only (both strips are
    edge strips); the cut and off-centre members mix band and uniform items on
    the short grid's edge strips; 40×200 (five strips) has uniform items on an
    inner strip and on an edge strip for every member.  Returns the kinds."""
    kinds = item_kinds(entries, N)
    if member == "cover" and (M, N) in ((66, 49), SHORT_GRID):
        assert kinds == {"uni-edge"}, kinds
    elif member in ("cut_y", "cut_xy", "offc") and (M, N) == SHORT_GRID:
        assert {"band-edge", "uni-edge"} <= kinds, kinds
    elif (M, N) == (40, 200):
        assert {"uni-inner", "uni-edge"} <= kinds, kinds
    return kinds


@functools.lru_cache(maxsize=None)
def reference(kind, M, N, count, member=None):
    """The fp64 recurrence after `count` sweeps; computed once, never modified."""
    fn = {"three": torch_ref.three_step, "two": torch_ref.two_step, "single": torch_ref.single_sweep}[kind]
    return fn(problem(M, N, member), count)


def solver(nat, M, N, kind, member=None):
    """A single-rank solver of the kind's kernel, convergence test off."""
    opt = nat.SolveOptions()
    opt.algo = KINDS[kind][0]
    opt.check_tol = False
    return nat.DeviceSolver(problem(M, N, member).to_native(), D.block(M, N, 1, 0), None, opt)


def check_sweeps(s, M, N, kind, count, member=None):
    """S_0 + `count` sweeps on solver s: the reduced sums, the last α and β,
    the r / p planes and w against the recurrence.  Prints the worst relative
    deviations of the planes, then asserts; returns them."""
    _, steps, nsums, s_rel, s_abs, ab_rel, f_tol = KINDS[kind]
    assert s.sweep_steps == steps
    s.reset()
    s.run_iterations(steps * count, False)
    s.synchronize()
    st = s.state()
    assert st["iter"] == steps * count and st["status"] == 0, (st["iter"], st["status"])
    ref = reference(kind, M, N, count, member)
    par = (count - 1) & 1
    got, want = st["fs" if steps == 1 else "fs2"][par], ref.sums[count]
    last = (lambda v: v[-1]) if steps == 1 else (lambda v: v[-1][steps - 1])
    fields = {"r": s.field(0 if par == 0 else 4)[2:M + 1, 2:N + 1], "p": s.field(2 if par == 0 else 3)[2:M + 1, 2:N + 1],
              "w": s.w()}
    dev = {}
    for name, f in fields.items():
        want_f = getattr(ref, name)[1:M, 1:N].numpy()
        dev[name] = float(np.abs(f - want_f).max() / np.abs(want_f).max())
    scale = max(abs(x) for x in want)
    # (the sums' worst deviation in units in which the bound below is s_rel)
    dev["sums"] = max(abs(got[n] - want[n]) / max(abs(want[n]), s_abs / s_rel * scale) for n in range(nsums))
    print(f"sweep-dev {kind} {M}x{N}{' ' + member if member else ''} count={count} ti={s.ti} resident={int(s.resident)} "
          + " ".join(f"{k}={v:.2e}" for k, v in dev.items()))
    for n in range(nsums):
        assert got[n] == pytest.approx(want[n], rel=s_rel, abs=s_abs * scale), n
    assert st["alpha"] == pytest.approx(last(ref.alpha), rel=ab_rel)
    assert st["beta"] == pytest.approx(last(ref.beta), rel=ab_rel)
    for name, f in fields.items():
        want_f = getattr(ref, name)[1:M, 1:N].numpy()
        np.testing.assert_allclose(f, want_f, rtol=0, atol=f_tol * np.abs(want_f).max(), err_msg=name)
    return dev
