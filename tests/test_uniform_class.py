"""CPU tests of the invariant the three-step sweep's uniform march relies on:
a uniform item is of ONE class.  kS3 takes the row coefficients of a uniform
item — the face coefficient over h1², over h2², and 1/D — once, from the first
row of its window (rows ib−6 .. ie+6 in the strip's 64 loaded columns), so
every row of that window must be wholly interior or every row wholly
non-interior.  The planner requires it (rows_uniform, item_layout.cpp); here
it is checked from outside, on the lists native.item_layout returns and the
row classes it planned them from (native.planner_row_classes), for the
reference problem and every member of sweep_checks.FAMILY under each static
layout.

Why no list changed when the requirement was added (test_item_layout.py's
pinned lists and hashes): an interior node has its four faces at exactly 1, an
exterior one at exactly 1/ε, and vertical neighbours share a face — so between
a wholly interior and a wholly exterior row of a strip lies a band row, which
no uniform window holds.  test_adjacent_uniform_rows_share_a_class checks that
directly on the row classes."""

import numpy as np
import pytest
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

UNI_BIT = sweep_checks.UNI_BIT
H, FSW, HL, WIN = 6, 48, 8, 64  # halo rows of an item's window; output columns, left halo and loaded columns of a strip
MEMBERS = [None] + list(sweep_checks.FAMILY)
GRIDS = [(66, 49), (130, 97), (40, 200), (2048, 2048)]
HEIGHTS = [8, 32, 112]
LAYOUTS = ["lpt", "fill", "equal"]


def _row_kinds(rc, J):
    """Per table row: 1 wholly interior in columns J .. J+63, 0 no interior column there, -1 some of each."""
    lo, hi = np.maximum(rc[:, 0], J), np.minimum(rc[:, 1], J + WIN - 1)
    inner = (rc[:, 0] <= J) & (rc[:, 1] >= J + WIN - 1)
    return np.where(inner, 1, np.where(lo > hi, 0, -1))


def _band(rc, J):
    """Per table row: a boundary-band node in the strip's columns (the planner's row_gen_x, the kernel's has_gen)."""
    lo, hi = np.maximum(rc[:, 2], J), np.minimum(rc[:, 3], J + WIN - 1)
    return (lo <= hi) & ((rc[:, 0] > rc[:, 1]) | (lo < rc[:, 0]) | (hi > rc[:, 1]))


def _check_lists(nat, member, M, N, P=1, spec="device", ranks=(0,), overlaps=(False,), heights=HEIGHTS):
    prob = sweep_checks.problem(M, N, member).to_native()
    seen = 0
    for rank in ranks:
        blk = nat.decompose(M, N, D.grid(P, M, N, spec), rank)
        rc, tab_lo = nat.planner_row_classes(prob, blk, 3)
        rc = np.asarray(rc)
        kinds = {}
        for ov in overlaps:
            for ti in heights:
                for layout in LAYOUTS:
                    lay = nat.item_layout(prob, blk, 3, ti, overlap=ov, layout=layout, force_layout=layout)
                    assert lay["name"] == layout
                    for ib, rows, strip, flags in lay["entries"]:
                        if rows == 0 or not flags & UNI_BIT:
                            continue
                        J = -(HL - 1) + FSW * strip
                        if strip not in kinds:
                            kinds[strip] = _row_kinds(rc, J)
                        ie = min(ib + rows - 1, blk.nx)
                        win = kinds[strip][ib - H - tab_lo:ie + H - tab_lo + 1]
                        assert len(win) == ie - ib + 1 + 2 * H
                        assert (win == win[0]).all() and win[0] >= 0, (member, M, N, rank, ov, ti, layout, ib, rows, strip)
                        seen += 1
    return seen


@pytest.mark.parametrize("M,N", GRIDS)
@pytest.mark.parametrize("member", MEMBERS)
def test_uniform_items_are_single_class(nat, member, M, N):
    seen = _check_lists(nat, member, M, N)
    print(f"uniform-class {member} {M}x{N}: {seen} uniform entries")
    if member == "cover" or (M, N) in ((40, 200), (2048, 2048)):  # (the shapes that hold uniform items for every member)
        assert seen > 0


@pytest.mark.parametrize("member", MEMBERS)
def test_uniform_items_are_single_class_2x2(nat, member):
    """A 2×2 split of 2048² (1024-row blocks with neighbours on two sides), with and without the overlap's
    boundary-first lists; 130×97 splits into 65/64 × 48 blocks."""
    seen = _check_lists(nat, member, 2048, 2048, 4, "2x2", range(4), (False, True), heights=[32])
    seen += _check_lists(nat, member, 130, 97, 4, "2x2", range(4), (False, True), heights=[8, 32])
    print(f"uniform-class {member} 2x2: {seen} uniform entries")
    assert seen > 0


@pytest.mark.parametrize("M,N", GRIDS + [(1600, 2400)])
@pytest.mark.parametrize("member", MEMBERS)
def test_adjacent_uniform_rows_share_a_class(nat, member, M, N):
    """In every strip, two vertically adjacent rows that are both uniform (no band node, one class over the strip's
    columns) are of the same class."""
    blk = nat.decompose(M, N, D.grid(1, M, N, "device"), 0)
    rc, tab_lo = nat.planner_row_classes(sweep_checks.problem(M, N, member).to_native(), blk, 3)
    rc = np.asarray(rc)
    q = np.arange(len(rc)) + tab_lo
    rows = (q >= 1 - H) & (q <= blk.nx + H)  # the rows of every item's window
    strips = nat.sweep_geometry(blk.nx, blk.ny, 3)["strips"]
    pairs = 0
    for s in range(strips):
        J = -(HL - 1) + FSW * s
        k = _row_kinds(rc, J)
        uni = rows & (k >= 0) & ~_band(rc, J)
        both = uni[:-1] & uni[1:]
        assert (k[:-1][both] == k[1:][both]).all(), (member, M, N, s)
        pairs += int(both.sum())
    assert pairs > 0 or member is None
