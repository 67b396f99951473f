"""One rank of the multi-process test of the residual stop rule (launched with
torch.distributed.run): every rank loads the same global rhs and w0, solves
under EllipseProblem(stop="residual") on its block through a DeviceSession —
the fields as tensors on this rank's device, return_w="device" — and saves its
report and its block.

usage: stop_job.py M N SHIFT TOL ATOL rhs.npy w0.npy OUT DECOMP   ->  OUT.r<rank>.json / .npy"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem  # noqa: E402


def main(argv) -> int:
    import torch

    M, N, sigma, tol, atol = int(argv[1]), int(argv[2]), float(argv[3]), float(argv[4]), float(argv[5])
    f, g, out, decomp = np.load(argv[6]), np.load(argv[7]), argv[8], argv[9]
    prob = EllipseProblem(M, N, shift=sigma, tol=tol, stop="residual", atol=atol)
    with DeviceSession(prob, decomp) as session:
        dev = f"cuda:{session.device_index}"
        rep = session.solve(rhs=torch.from_numpy(f).to(dev), w0=torch.from_numpy(g).to(dev), return_w="device")
        blk = session.block
        assert tuple(rep.w.shape) == (blk.nx, blk.ny) and rep.w_origin == (blk.i0, blk.j0)
        w = rep.w.cpu().numpy()
    d = rep.to_dict()
    d["origin"] = list(rep.w_origin)
    np.save(f"{out}.r{rep.rank}.npy", w)
    with open(f"{out}.r{rep.rank}.json", "w") as fh:
        json.dump(d, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
