"""Time the operator pass (kApplyField) against the torch route, on one GPU.

  python tools/operator_perf.py [M N] [--calls 200] [--repeats 3]

Per repeat, alternating in one process, device events around `calls` calls after a warm-up:
  session  DeviceSession.apply(v, out="device"): the public call (argument checks with their
           isfinite pass, the output allocation, the kernel, the state read)
  native   DeviceSolver.apply_device into a preallocated tensor: the kernel and the state read
  torch    torch_ref.apply_A on cuda with pre-assembled a, b — the only route without this pass
Bytes: the algorithmic 16 B per node (8 read + 8 written) over the native time."""

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem  # noqa: E402
from poisson_ellipse_openmp_mpi_cuda_amd.ops import torch_ref  # noqa: E402


def timed(fn, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / calls  # ms per call


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("M", nargs="?", type=int, default=8192)
    ap.add_argument("N", nargs="?", type=int, default=8192)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    M, N = a.M, a.N
    prob = EllipseProblem(M, N)
    g = torch.Generator(device="cuda").manual_seed(1)
    v = torch.rand(M - 1, N - 1, dtype=torch.float64, device="cuda", generator=g) - 0.5
    ca, cb, _ = torch_ref.assemble(prob, device="cuda")
    V = torch.zeros(M + 1, N + 1, dtype=torch.float64, device="cuda")
    V[1:-1, 1:-1] = v
    nodes = (M - 1) * (N - 1)
    with DeviceSession(prob) as s:
        out = torch.empty((M - 1, N - 1), dtype=torch.float64, device="cuda")
        stream = torch.cuda.current_stream().cuda_stream

        def session():
            return s.apply(v, out="device")

        def native():
            return s.solver.apply_device(v.data_ptr(), v.stride(0), v.stride(1), False, False, out.data_ptr(),
                                         out.stride(0), out.stride(1), 0, 0, stream)

        def torch_route():
            return torch_ref.apply_A(V, ca, cb, prob.h1, prob.h2)

        ref = torch_route()[1:-1, 1:-1]
        got = session().field
        native()
        dev = float((got - ref).abs().max() / ref.abs().max())
        print(f"operator-perf {M}x{N} calls={a.calls} field vs torch route: {dev:.2e}, native == session: "
              f"{bool(torch.equal(out, got))}")
        for fn in (session, native, torch_route):  # warm-up
            for _ in range(5):
                fn()
        for rep in range(a.repeats):
            ms = {fn.__name__: timed(fn, a.calls) for fn in (session, native, torch_route)}
            print(f"repeat {rep}: session {ms['session']:.4f} ms  native {ms['native']:.4f} ms  torch {ms['torch_route']:.4f} ms"
                  f"  | native {16.0 * nodes / (ms['native'] * 1e-3) / 1e12:.3f} TB/s over 16 B/node"
                  f"  | torch / native {ms['torch_route'] / ms['native']:.2f}x, torch / session "
                  f"{ms['torch_route'] / ms['session']:.2f}x")
    return 0


if __name__ == "__main__":
    sys.exit(main())
