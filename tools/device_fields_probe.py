"""Cost of handing user fields to the device solver: host arrays against GPU
tensors (profiles/device_fields.txt, docs/PERFORMANCE.md "Fields in device
memory").

    python tools/device_fields_probe.py M {host|device|device-gen}

One process, one variant: a DeviceSession at M × M, then four solves with
rhs = 1 + x + y — the first use in the process (lazy kernel loading; its
report also carries the construction), the same solve again ("cold": w⁰ = 0),
and two continuation steps (rhs · 1.01 from the previous w, and back).
host: numpy arrays in, return_w=True.  device: GPU tensors in,
return_w="device".  device-gen: the same, the fields computed on the GPU, so
that a memory-copy trace of the process holds no upload of the probe's own.
Wall time is taken around solve() with a device synchronise on either side;
"fields" = wall − timers["solver"] is the field handling.  Prints one JSON
line.  Run fresh processes and alternate the variants for an A/B; run it under
`rocprofv3 --kernel-trace --stats` or `--memory-copy-trace --stats` (one at a
time) for kSliceField / kGatherW and the copies."""

import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem  # noqa: E402


def main(argv) -> int:
    M, variant = int(argv[1]), argv[2]
    if variant not in ("host", "device", "device-gen"):
        raise SystemExit(__doc__)
    prob = EllipseProblem(M, M)
    x = prob.A1 + np.arange(1, M, dtype=np.float64) * prob.h1
    y = prob.A2 + np.arange(1, M, dtype=np.float64) * prob.h2
    dev = variant != "host"
    if variant == "device-gen":
        f = 1.0 + torch.from_numpy(x).cuda()[:, None] + torch.from_numpy(y).cuda()[None, :]
        f2 = 1.01 * f
    else:
        f = 1.0 + x[:, None] + y[None, :]
        f2 = 1.01 * f
        if dev:
            f, f2 = torch.from_numpy(f).cuda(), torch.from_numpy(f2).cuda()
    rw = "device" if dev else True

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rep = fn()
        torch.cuda.synchronize()
        return rep, time.perf_counter() - t0

    t0 = time.perf_counter()
    session = DeviceSession(prob)
    out = dict(M=M, variant=variant, ctor_s=round(time.perf_counter() - t0, 3))
    first, t_first = timed(lambda: session.solve(rhs=f, return_w=rw))
    cold, t_cold = timed(lambda: session.solve(rhs=f, return_w=rw))
    cont, t_cont = timed(lambda: session.solve(rhs=f2, w0=cold.w, return_w=rw))
    back, t_back = timed(lambda: session.solve(rhs=f, w0=cont.w, return_w=rw))
    out["algo"] = cold.algo
    for name, rep, t in (("first", first, t_first), ("cold", cold, t_cold), ("cont", cont, t_cont),
                         ("back", back, t_back)):
        solver = rep.timers["solver"] - rep.timers["construct"]
        out[name] = dict(iters=rep.iters, wall_ms=round(1e3 * t, 3), solver_ms=round(1e3 * solver, 3),
                         fields_ms=round(1e3 * (t - solver), 3), res_true=rep.res_true)
    out["w_sum"] = float(back.w.sum())
    session.close()
    print("PROBE " + json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
