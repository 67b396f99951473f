"""Invariants of an item list, shared by the MI355X tests of live solvers
(test_layout.py) and the CPU tests of the host planner (test_item_layout.py).
Entries are (first row, rows, strip, flags) per list position; rows 0 is an
empty position."""

import hashlib
import struct

import numpy as np

# per iterations-per-sweep: output columns per strip, a strip's left halo columns
FSW = {1: 124, 2: 120, 3: 48}
HL = {1: 2, 2: 4, 3: 8}


def coverage(entries, nstrips, nx, ny, steps=3):
    """Every owned row of every strip is marched exactly once."""
    ent = [e for e in entries if e[1] > 0]
    assert nstrips == (ny + FSW[steps] - 1) // FSW[steps]  # (three-step: 48 output columns per strip, fused3.hip)
    cov = np.zeros((nstrips, nx + 1), dtype=np.int32)
    for ib, rows, strip, _flags in ent:
        assert 0 <= strip < nstrips and ib >= 1 and ib + rows - 1 <= nx
        cov[strip, ib:ib + rows] += 1
    assert (cov[:, 1:] == 1).all(), "a row of a strip is marched twice or never"
    return ent


def boundary_first(entries, nbr, nx, ny, lbase, lnb, steps=3):
    """Overlap: the kernel's kSignal variant counts the first lnb[x] positions
    of shard x (a static list is one shard: positions 0 .. nb-1) as the boundary
    items (outputs a neighbour needs: the 2·steps owned rows / columns next to
    it) and starts the exchange when they are stored — so those positions hold
    exactly the boundary items."""
    assert sum(lnb) > 0
    H, fsw, hl = 2 * steps, FSW[steps], HL[steps]
    has = [nbr[i] >= 0 for i in range(4)]  # LEFT, RIGHT, DOWN, UP

    def bnd(ib, rows, strip):
        j0 = -(hl - 1) + fsw * strip
        jlo, jhi = max(1, j0 + hl), min(ny, j0 + fsw + hl - 1)
        return ((has[0] and ib <= H) or (has[1] and ib + rows - 1 >= nx - H + 1) or (has[2] and jlo <= H)
                or (has[3] and jhi >= ny - H + 1))

    for x in range(len(lnb)):
        for pos in range(lbase[x], lbase[x + 1]):
            ib, rows, strip, _flags = entries[pos]
            if rows == 0:
                continue
            assert bnd(ib, rows, strip) == (pos - lbase[x] < lnb[x]), (x, pos, lnb[x], ib, rows, strip)


def equal_balance(entries, load, waves):
    """Equal-cost layout: exactly k pieces per wave, estimated loads within a
    few percent."""
    mx, mean, per = load
    assert mx <= 1.10 * mean, (mx, mean)  # (8192² at 112 rows: 7 pieces per wave, 1.09)
    ent = [e for e in entries if e[1] > 0]
    assert (per - 1) * waves < len(ent) <= per * waves


def digest(entries):
    """SHA-256 over the entries as little-endian int32 quadruples."""
    h = hashlib.sha256()
    for e in entries:
        h.update(struct.pack("<4i", *e))
    return h.hexdigest()
