"""CPU tests of the host-only item-layout planner (csrc/core/item_layout.cpp,
native.item_layout / sweep_geometry / ti_candidates): the invariants of
test_layout.py — every owned row of every strip marched exactly once, the
overlap's boundary items first (per shard for dynamic lists), the equal-cost
layout's balance — over that test's matrix at 8192² and over small shapes
where the cutting paths run; the lists, candidate heights and geometry pinned
entry for entry against tests/golden/layouts.json, recorded from live solvers
on an MI355X before the planner was split from the solver; and the planner
under ASan + UBSan as a stand-alone program (make asan, bin/pe_layout_asan).
No device is needed: layouts are milliseconds of host arithmetic."""

import json
import os
import shutil
import subprocess

import pytest

import layout_checks
import sweep_checks

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "layouts.json")) as _f:
    GOLD = json.load(_f)
CASES = {c["name"]: c for c in GOLD["cases"]}


def _default_name(steps, nx, ny):
    """The construction's three-step layout by block size (device_solver.cpp)."""
    npts = nx * ny
    return "lpt" if steps < 3 or npts >= 5e7 else "fill" if npts >= 2.5e7 else "equal"


def _layout(nat, M, N, P=1, spec="device", rank=0, steps=3, ti=None, order=0, overlap=False, force="", member=None, **kw):
    blk = nat.decompose(M, N, D.grid(P, M, N, spec), rank)
    if ti is None:  # the construction's untuned heights (three-step)
        npts = blk.nx * blk.ny
        ti = 448 if npts > 1 << 26 else 112 if npts >= 1 << 25 else 80 if npts >= 1 << 24 else 48
    lay = nat.item_layout(sweep_checks.problem(M, N, member).to_native(), blk, steps, ti, order=order, overlap=overlap,
                          layout=_default_name(steps, blk.nx, blk.ny), force_layout=force, **kw)
    return blk, lay


def _check(nat, blk, lay, steps, overlap):
    ent = layout_checks.coverage(lay["entries"], nat.sweep_geometry(blk.nx, blk.ny, steps)["strips"], blk.nx, blk.ny, steps)
    if overlap:
        n = lay["shards"]
        layout_checks.boundary_first(lay["entries"], blk.nbr, blk.nx, blk.ny, lay["lbase"][:n + 1], lay["lnb"][:n], steps)
        if lay["waves"]:  # a static list: one shard
            assert n == 1 and lay["boundary"] == lay["lnb"][0]
    else:
        assert lay["boundary"] == 0
    return ent


@pytest.mark.parametrize("P,spec,env", [(1, "device", {}), (1, "device", {"PE_LAYOUT": "equal"}),
                                        (1, "device", {"PE_LAYOUT": "fill"}), (8, "device", {}),
                                        (2, "device", {}), (4, "device", {"PE_LAYOUT": "equal"}),
                                        (8, "4x2", {"PE_OVERLAP": "1"}), (6, "2x3", {"PE_OVERLAP": "1"}),
                                        (4, "2x2", {"PE_OVERLAP": "1", "PE_LAYOUT": "lpt"}),
                                        (8, "device", {"PE_YOUNG": "1.25"}), (1, "device", {"PE_YOUNG": "1.25"})])
def test_layout_covers_every_row_once(nat, P, spec, env):
    """test_layout.py's matrix at 8192² (rank P // 2; untuned heights)."""
    ov = env.get("PE_OVERLAP") == "1"
    blk, lay = _layout(nat, 8192, 8192, P, spec, P // 2, overlap=ov, force=env.get("PE_LAYOUT", ""),
                       young=float(env.get("PE_YOUNG", 1.0)))
    _check(nat, blk, lay, 3, ov)
    if lay["name"] == "equal" and not ov:
        layout_checks.equal_balance(lay["entries"], lay["load"], lay["waves"])


SMALL = ([(500, 700, 1, "device", 0, 3, 48, 0, False, lay) for lay in ("equal", "fill", "lpt")]
         + [(40, 40, 1, "device", 0, 3, 48, 0, False, lay) for lay in ("equal", "fill", "lpt")]
         + [(2048, 2048, 8, "rows", r, 3, 48, 0, ov, lay) for r in (0, 4, 7) for ov in (False, True)
            for lay in ("equal", "fill", "lpt")]
         + [(1000, 1000, P, spec, r, 3, 48, 0, True, lay) for P, spec in ((6, "2x3"), (8, "4x2")) for r in range(P)
            for lay in ("lpt", "fill", "equal")]
         + [(2048, 2048, 1, "device", 0, 2, 24, 0, False, ""), (2048, 2048, 1, "device", 0, 1, 10, 0, False, ""),
            (2048, 2048, 1, "device", 0, 1, 18, 3, False, "")]
         + [(2048, 2048, 4, "2x2", r, 1, ti, o, ov, "") for o, ti in ((0, 10), (3, 18)) for r in (0, 2)
            for ov in (False, True)])


@pytest.mark.parametrize("M,N,P,spec,rank,steps,ti,order,ov,lay", SMALL)
def test_small_shapes(nat, M, N, P, spec, rank, steps, ti, order, ov, lay):
    """Fewer items than waves (the cutting paths), one short item per strip,
    one- and two-sided neighbours, 2-D splits under the overlap, the two-step
    and single sweeps (static and dynamic lists).  Every shape passed these
    invariants on live solvers before the planner was split off."""
    blk, l = _layout(nat, M, N, P, spec, rank, steps, ti, order, ov, lay)
    ent = _check(nat, blk, l, steps, ov)
    assert (l["waves"] == 0) == (order == 3) and l["name"] == (lay or "lpt")
    if order == 3:
        assert len(ent) == len(l["entries"]) == l["nslots"] and l["lbase"][l["shards"]] == len(ent)
    if l["name"] == "equal" and not ov:
        # exactly k pieces per wave; the balance bound max <= 1.10 mean where
        # the list met it before the split: 40×40 (1.01).  The other shapes
        # have one piece per wave, of 8 rows at least, so a band piece weighs
        # several uniform ones and the bound cannot hold — max / mean 2.39 at
        # 500×700 (73 row steps against 30.5), 2.42-2.68 on the slab blocks of
        # 2048², the same lists on live solvers.
        per = l["load"][2]
        assert (per - 1) * l["waves"] < len(ent) <= per * l["waves"]
        if (M, N) == (40, 40):
            layout_checks.equal_balance(l["entries"], l["load"], l["waves"])


# the three-step cases of test_sweep_family.py whose item kinds sweep_checks.check_item_kinds pins: (member, M, N, ti, layout)
FAMILY_KINDS = ([("cover", 66, 49, 48, "")] + [(m, 40, 200, 48, "") for m in sweep_checks.FAMILY]
                + [(m,) + sweep_checks.SHORT_GRID + (48, "") for m in ("cover", "cut_y", "cut_xy", "offc")]
                + [(m,) + sweep_checks.SHORT_GRID + (ti, lay) for m in sweep_checks.SHORT_MEMBERS
                   for ti in sweep_checks.SHORT_THREE[1] for lay in sweep_checks.SHORT_THREE[2]])


@pytest.mark.parametrize("member,M,N,ti,lay", FAMILY_KINDS)
def test_family_cases_hold_their_item_kinds(nat, member, M, N, ti, lay):
    """The family members' three-step cases are there for uniform items on
    edge strips (the reference problem's lists at these shapes are band items
    only): the covering ellipse is nothing else, the cut and off-centre ones
    mix them with band items, 40×200 adds an inner strip.  Were the planner to
    stop flagging them, the MI355X test would compare kernels it no longer
    runs; it asserts the same from the live solver's list."""
    blk, l = _layout(nat, M, N, ti=ti, force=lay, member=member)
    _check(nat, blk, l, 3, False)
    assert l["name"] == (lay or "equal")
    sweep_checks.check_item_kinds(l["entries"], M, N, member)


def _rebuild(nat, c):
    blk = nat.decompose(c["M"], c["N"], D.grid(c["P"], c["M"], c["N"], c["spec"]), c["rank"])
    q = c["request"]
    return nat.item_layout(EllipseProblem(c["M"], c["N"]).to_native(), blk, c["steps"], c["ti"], order=c["order"],
                           overlap=c["overlap"], layout=q["layout"], wave_caps=tuple(q["wave_caps"]), cus=q["cus"],
                           ov_reserve=q["ov_reserve"], young=q["young"], wperm=q["wperm"], ov_debug=q["ov_debug"],
                           force_layout=q["force_layout"])


@pytest.mark.parametrize("name", sorted(CASES))
def test_golden_layouts(nat, name):
    """Entry for entry the list the solver laid out before the split."""
    c = CASES[name]
    lay = _rebuild(nat, c)
    if "entries" in c:  # (three small cases in full, so a mismatch can be read)
        assert [tuple(e) for e in lay["entries"]] == [tuple(e) for e in c["entries"]]
    assert (lay["name"], lay["waves"], lay["boundary"], lay["cuts"], lay["nblocks"], len(lay["entries"])) == \
        (c["layout_name"], c["layout_waves"], c["layout_boundary"], c["layout_cuts"], c["blocks"], c["n_entries"])
    assert layout_checks.digest(lay["entries"]) == c["sha256"]


def test_candidate_heights_and_geometry(nat):
    for c in GOLD["candidates"]:
        blk = nat.decompose(c["M"], c["N"], D.grid(c["P"], c["M"], c["N"], c["spec"]), c["rank"])
        assert nat.ti_candidates(blk.nx, blk.ny, c["steps"], c["wave_cap"]) == c["leading"], c["name"]
    assert sorted(g["steps"] for g in GOLD["geometry"]) == [1, 2, 3]
    for g in GOLD["geometry"]:
        geo = nat.sweep_geometry(g["nx"], g["ny"], g["steps"])
        # (a solver's fields: rows -1 .. nx+2 of the plane's columns)
        assert (g["nx"] + 4, geo["plane"], geo["strips"]) == (g["field_rows"], g["field_cols"], g["strips"]), g["name"]


@pytest.fixture(scope="module")
def layout_asan():
    if shutil.which("make") is None or shutil.which("g++") is None:
        pytest.skip("no host toolchain")
    r = subprocess.run(["make", "-s", "bin/pe_layout_asan"], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return os.path.join(ROOT, "bin", "pe_layout_asan")


@pytest.mark.parametrize("name", ["500x700-equal-48", "2048-fill-64", "8192-lpt-112", "4x2-r4-default-ov1",
                                  "slab8-r4-equal-64-ov1", "2048-2x2-r2-single-18-o3-ov1"])
def test_planner_asan_ubsan_clean(layout_asan, name):
    """The planner indexes prefix arrays with computed offsets: the
    stand-alone program, built with ASan + UBSan from the host sources alone,
    lays the case out cleanly and prints the golden digest."""
    c, q = CASES[name], CASES[name]["request"]
    cmd = [layout_asan] + [str(v) for v in (c["M"], c["N"], c["P"], c["spec"], c["rank"], c["steps"], c["ti"], c["order"],
                                            int(c["overlap"]), q["layout"], q["wave_caps"][0], q["wave_caps"][1], q["cus"],
                                            q["young"], q["wperm"], q["force_layout"])]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1"))
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-3000:]
    assert "AddressSanitizer" not in out and "runtime error" not in out
    assert out.split()[-1] == c["sha256"] and f"entries {c['n_entries']} " in out
