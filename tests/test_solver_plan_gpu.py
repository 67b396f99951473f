"""The live constructor against its host-only plan (MI355X): for small blocks
on each side of the plan's thresholds, native.solver_plan(**s.plan_request)
rebuilds what the solver set up, and native.halo_candidates(**s.halo_request)
the paths its halo-path choice timed.  Construction only: nothing is iterated."""

import re

import pytest

from poisson_ellipse_openmp_mpi_cuda_amd import EllipseProblem
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D

pytestmark = pytest.mark.gpu

# name: (M, N, P, spec, rank, delay comm, variant, shift, env, (fused, steps) expected)
CASES = {
    "8x8": (8, 8, 1, "device", 0, False, 0, 0.0, {}, (True, 1)),
    "9x9": (9, 9, 1, "device", 0, False, 0, 0.0, {}, (True, 1)),
    "9x9-nores": (9, 9, 1, "device", 0, False, 0, 0.0, {"PE_RESIDENT": "0"}, (True, 3)),
    "25x25-virtual": (25, 25, 4, "2x2", 2, False, 0, 0.0, {}, (True, 3)),
    "24x24-virtual": (24, 24, 4, "2x2", 2, False, 0, 0.0, {}, (True, 1)),
    "slab4-31": (32, 40, 4, "rows", 1, True, 0, 0.0, {}, (True, 1)),
    "slab4-32": (33, 40, 4, "rows", 1, True, 0, 0.0, {}, (True, 2)),
    "slab4-45": (46, 40, 4, "rows", 1, True, 0, 0.0, {}, (True, 2)),
    "slab4-48": (49, 40, 4, "rows", 1, True, 0, 0.0, {}, (True, 3)),
    "variant1": (40, 40, 1, "device", 0, False, 1, 0.0, {}, (False, 1)),
    "shift40": (40, 40, 1, "device", 0, False, 0, 40.0, {}, (False, 1)),
    "1025x1026": (1025, 1026, 1, "device", 0, False, 0, 0.0, {"PE_TI_TUNE": "0"}, (True, 1)),
}
PLAN_KNOBS = ("PE_RESIDENT", "PE_STEPS", "PE_TI", "PE_ORDER", "PE_TI_TUNE", "PE_LAYOUT", "PE_HALO", "PE_OVERLAP", "PE_HALO_TUNE")


def _leading(rows):
    out = []
    for r in rows:
        if r <= 0 or (out and r <= out[-1]):
            break
        out.append(r)
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_live_solver_follows_its_plan(gpu, monkeypatch, name):
    nat = gpu
    M, N, P, spec, rank, comm, variant, shift, env, want = CASES[name]
    for k in PLAN_KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    opt = nat.SolveOptions()
    opt.variant, opt.check_tol = variant, False
    blk = nat.decompose(M, N, D.grid(P, M, N, spec), rank)
    c = nat.make_delay_comm(P, 0.0, 0.0) if comm else None
    s = nat.DeviceSolver(EllipseProblem(M, N, shift=shift).to_native(), blk, c, opt)
    rq = s.plan_request
    assert (rq["comm_size"], rq["resident"], rq["pe_resident"], rq["pe_ti_tune"]) == \
        (P if comm else 1, s.resident, int(env["PE_RESIDENT"]) if "PE_RESIDENT" in env else None,
         int(env["PE_TI_TUNE"]) if "PE_TI_TUNE" in env else None)
    pl = nat.solver_plan(**rq)
    assert (s.fused, s.sweep_steps) == want
    # (under the halo/interior overlap the list in use is the overlap's boundary-first one, whatever it was asked
    # with: layout_name is then that list's, and the plan's name is the request's)
    assert (pl["fused"], pl["steps"], pl["ti"], pl["order"], pl["chunk"], pl["strips"], pl["layout"]) == \
        (s.fused, s.sweep_steps, s.ti, s.order, s.chunk, s.strips, s.layout_request["layout"] if s.overlap else s.layout_name)
    rows = list(s.ti_tuning_rows)
    assert (len(rows) > 0) == (pl["tune_ti"] and not s.resident)
    if rows:
        assert _leading(rows) == pl["candidates"]
    assert not s.resident or pl["resident_likely"]
    if s.fused:
        assert s.layout_request["layout"] == pl["layout"]
        assert tuple(s.layout_request["wave_caps"]) == tuple(pl["wave_caps"]) and s.layout_request["cus"] == rq["cus"]
    if not comm:
        assert s.halo_candidates == []
        return
    cands, late = nat.halo_candidates(**s.halo_request)
    names = [p + ("+overlap" if o else "") for p, o, _ in cands] + (["put+overlap"] if late else [])
    timed = [re.sub(r" @\d+$", "", n) for n, _ in s.halo_candidates if not n.endswith("(again)")]
    if len(names) == 1:  # (nothing to choose: not timed)
        assert timed == [] and s.halo_path == names[0] + " (only candidate)"
    else:
        assert timed == names and s.halo_path in names
