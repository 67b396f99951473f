#!/usr/bin/env python3
"""Record the fixtures of tests/test_solver_plan.py (tests/golden/solver_plans.json).

Run on an MI355X from a checkout whose DeviceSolver constructor is the one to
pin — the file in the repository was recorded on the commit before the
algorithm choice moved into the host-only plan (csrc/core/solver_plan.cpp).
Only properties that commit already had are read: what the live solver decided
for each block, next to the inputs it decided from.

Multi-rank blocks are constructed on the delay transport in one process
(make_delay_comm(P, 0, 0), as tests/test_layout.py does); virtual-rank blocks
are a split Block without a comm.  A block whose rows per item are tuned is
recorded twice: with PE_TI_TUNE=0 (the untuned height and layout), and tuned,
keeping only that the tuning ran and its candidate heights (the chosen height
and layout depend on the timings).

usage: tools/record_solver_plans.py [OUT [COMMIT]]   (default: tests/golden/solver_plans.json, git's HEAD)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import poisson_ellipse_openmp_mpi_cuda_amd as pe  # noqa: E402
from poisson_ellipse_openmp_mpi_cuda_amd.parallel import decomp as D  # noqa: E402

# knobs that keep construction cheap and do not feed the plan
CHEAP = {"PE_PLACEMENT_TRIES": "1", "PE_HALO_TUNE": "0"}
NORES = {"PE_RESIDENT": "0"}


def case(name, M, N, P=1, spec="device", rank=0, comm=False, algo=0, variant=0, shift=0.0, env=None, tuned=False):
    return dict(name=name, M=M, N=N, P=P, spec=spec, rank=rank, comm_size=P if comm else 1, algo=algo, variant=variant,
                shift=shift, env=dict(env or {}), tuned=tuned)


def cases():
    c = []
    # steps / fused: single-rank blocks of 7 and 8 rows
    c += [case("single-7", 8, 8), case("single-8", 9, 9), case("single-8-nores", 9, 9, env=NORES),
          case("single-7-nores", 8, 8, env=NORES)]
    # row slabs of 7, 8, 11 and 12 rows per rank on the delay transport
    for m1 in (31, 32, 45, 48):
        c.append(case(f"slab4-{m1}", m1 + 1, 40, 4, "rows", 1, comm=True))
    # 2x2 blocks of 11 and 12 rows and columns: comm and virtual ranks
    for M in (24, 25):
        c.append(case(f"2x2-comm-{M}", M, M, 4, "2x2", 2, comm=True))
        c.append(case(f"2x2-virtual-{M}", M, M, 4, "2x2", 2))
    # one row per block: the single sweep cannot run
    c.append(case("slab4-one-row", 8, 40, 4, "rows", 1, comm=True))
    c.append(case("variant1", 40, 40, variant=1))
    c.append(case("shift40", 40, 40, shift=40.0))
    for a in (1, 2, 3, 4):
        c.append(case(f"algo{a}-40", 40, 40, algo=a))
        c.append(case(f"algo{a}-130x200-nores", 130, 200, algo=a, env=NORES))
    for st in (1, 2):
        c.append(case(f"slab4-48-steps{st}", 49, 40, 4, "rows", 1, comm=True, env={"PE_STEPS": str(st)}))
        c.append(case(f"400x600-nores-steps{st}", 400, 600, env=dict(NORES, PE_STEPS=str(st))))
    # resident: held, refused, tile heights 64 and 65, switched off
    c += [case("400x600", 400, 600), case("800x1200", 800, 1200), case("1600x2400", 1600, 2400, env={"PE_TI_TUNE": "0"}),
          case("1600x2400-tuned", 1600, 2400, tuned=True),
          case("tile-64", 1601, 1200, env={"PE_TI_TUNE": "0"}), case("tile-65", 1602, 1200, env={"PE_TI_TUNE": "0"}),
          case("400x600-nores", 400, 600, env=NORES)]
    # sizes: tuning starts at 2^20 nodes; the 2^24 class
    c += [case("2p20-less", 1025, 1024, env=NORES), case("2p20", 1025, 1025, env=dict(NORES, PE_TI_TUNE="0")),
          case("2p20-tuned", 1025, 1025, env=NORES, tuned=True), case("2p20-resident", 1025, 1025),
          case("2p20-single-less", 1025, 1024, algo=2, env=NORES),
          case("2p20-single", 1025, 1025, algo=2, env=dict(NORES, PE_TI_TUNE="0")),
          case("2p20-single-tuned", 1025, 1025, algo=2, env=NORES, tuned=True),
          case("2p20-two", 1025, 1025, algo=3, env={"PE_TI_TUNE": "0"}),
          case("1025x1026", 1025, 1026, env={"PE_TI_TUNE": "0"})]
    for a in (0, 2, 3):
        c.append(case(f"2p24-less-algo{a}", 4097, 4096, algo=a, env={"PE_TI_TUNE": "0"}))
        c.append(case(f"2p24-algo{a}", 4097, 4097, algo=a, env={"PE_TI_TUNE": "0"}))
    c.append(case("2p24-tuned", 4097, 4097, tuned=True))
    c.append(case("2p24-less-single-tuned", 4097, 4096, algo=2, tuned=True))
    # PE_TI, PE_ORDER
    for a in (2, 3, 4):
        c.append(case(f"ti13-algo{a}", 400, 600, algo=a, env=dict(NORES, PE_TI="13")))
        c.append(case(f"bands-algo{a}", 400, 600, algo=a, env=dict(NORES, PE_TI="-1")))
    c.append(case("ti13-classic", 400, 600, algo=1, env={"PE_TI": "13"}))
    c.append(case("order3-single", 400, 600, algo=2, env=dict(NORES, PE_ORDER="3")))
    c.append(case("order3-three", 400, 600, algo=4, env=dict(NORES, PE_ORDER="3")))
    c.append(case("order3-classic", 400, 600, algo=1, env={"PE_ORDER": "3"}))
    c.append(case("order1-classic", 400, 600, algo=1, env={"PE_ORDER": "1"}))
    # chunk: a forced odd length on the streaming single, two- and three-step sweeps and the resident kernel
    c.append(case("chunk7-resident", 400, 600))
    c[-1]["chunk"] = 7
    for a in (2, 3, 4):
        c.append(case(f"chunk7-algo{a}", 400, 600, algo=a, env=NORES))
        c[-1]["chunk"] = 7
    # larger multi-rank blocks (the chunk's multi-rank term, slabs of a mid-size grid)
    c.append(case("slab8-2048", 2048, 2048, 8, "rows", 4, comm=True))
    c.append(case("4x2-2048", 2048, 2048, 8, "4x2", 4, comm=True))
    return c


def leading(rows):
    """The candidate heights: the ascending positive prefix of ti_tuning_rows."""
    out = []
    for r in rows:
        if r <= 0 or (out and r <= out[-1]):
            break
        out.append(r)
    return out


def observe(nat, c):
    for k in [k for k in os.environ if k.startswith("PE_")]:
        del os.environ[k]
    os.environ.update(CHEAP)
    os.environ.update(c["env"])
    prob = pe.EllipseProblem(c["M"], c["N"], shift=c["shift"]).to_native()
    blk = nat.decompose(c["M"], c["N"], D.grid(c["P"], c["M"], c["N"], c["spec"]), c["rank"])
    opt = nat.SolveOptions()
    opt.algo, opt.variant, opt.check_tol = c["algo"], c["variant"], False
    if "chunk" in c:
        opt.chunk = c["chunk"]
    comm = nat.make_delay_comm(c["comm_size"], 0.0, 0.0) if c["comm_size"] > 1 else None
    s = nat.DeviceSolver(prob, blk, comm, opt)
    rows = list(s.ti_tuning_rows)
    got = dict(fused=s.fused, steps=s.sweep_steps, resident=s.resident, order=s.order, chunk=s.chunk, strips=s.strips,
               tuned=len(rows) > 0, candidates=leading(rows), nx=blk.nx, ny=blk.ny)
    if s.fused and not s.resident:
        q = s.layout_request
        got.update(wave_caps=list(q["wave_caps"]), cus=q["cus"])
    if not rows:  # (the chosen height and layout depend on the timings)
        got.update(ti=s.ti, layout_name=s.layout_name, nitems=s.nitems, blocks=s.blocks)
        if s.fused and not s.resident:
            got.update(request_layout=s.layout_request["layout"])
    if got["tuned"] != c["tuned"]:
        print(f"{c['name']}: tuning {'ran' if got['tuned'] else 'did not run'}, the case list expected otherwise", flush=True)
    return got


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "solver_plans.json")
    nat = pe.native()
    nat.set_device(0)
    commit = sys.argv[2] if len(sys.argv) > 2 else subprocess.run(
        ["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip()
    recs = []
    for c in cases():
        try:
            c["observed"] = observe(nat, c)
        except ValueError as e:  # (a refusal: std::invalid_argument, nothing was launched)
            c["observed"] = dict(refused=str(e))
        recs.append(c)
        print(c["name"], json.dumps(c["observed"]), flush=True)
    doc = dict(recorded=dict(commit=commit, device=nat.device_name(0), cheap_knobs=CHEAP,
                             note="decisions of live solvers; tuned records keep only that the tuning ran and its "
                                  "candidate heights"),
               records=recs)
    with open(out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(f"{len(recs)} records -> {out}")


if __name__ == "__main__":
    main()
