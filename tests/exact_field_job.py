"""One rank of the multi-process tests of the user exact solution (launched
with torch.distributed.run): every rank loads the same global rhs, w0 and
exact, solves, and saves its report (and its share of w).

  hip       row slabs through a DeviceSession: the three fields as tensors on
            this rank's device, return_w="device"; saves this rank's block.
  dist-cpu  solve(backend="dist-cpu", decomp=DECOMP, return_w=True); rank 0
            saves the gathered w.

usage: exact_field_job.py BACKEND M N rhs.npy w0.npy exact.npy OUT [DECOMP]   ->  OUT.r<rank>.json / .npy"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve  # noqa: E402


def main(argv) -> int:
    backend, M, N = argv[1], int(argv[2]), int(argv[3])
    f, g, u, out = np.load(argv[4]), np.load(argv[5]), np.load(argv[6]), argv[7]
    prob = EllipseProblem(M, N)
    extra = {}
    if backend == "hip":
        import torch

        with DeviceSession(prob, "rows") as session:
            dev = f"cuda:{session.device_index}"
            rep = session.solve(rhs=torch.from_numpy(f).to(dev), w0=torch.from_numpy(g).to(dev),
                                exact=torch.from_numpy(u).to(dev), return_w="device")
            blk = session.block
            assert tuple(rep.w.shape) == (blk.nx, blk.ny) and rep.w_origin == (blk.i0, blk.j0)
            extra["user_exact"] = bool(session.solver.user_exact)
        w = rep.w.cpu().numpy()
    else:
        rep = solve(prob, backend=backend, decomp=argv[8], rhs=f, w0=g, exact=u, return_w=True)
        w = rep.w
    d = rep.to_dict()
    d.update(extra)
    if w is not None:
        np.save(f"{out}.r{rep.rank}.npy", w)
    with open(f"{out}.r{rep.rank}.json", "w") as fh:
        json.dump(d, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
