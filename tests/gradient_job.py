"""One rank of the multi-process tests of return_grad (launched with
torch.distributed.run): every rank loads the same global rhs and w0, solves
with the gradient, and saves its report and its share of w and of the gradient.

  hip       row slabs through a DeviceSession, the fields as tensors on this
            rank's device, return_w="device" and return_grad="device": saves
            this rank's blocks (w (nx, ny), grad (2, nx, ny)).
  dist-cpu  solve(backend="dist-cpu", decomp=DECOMP, return_w=True,
            return_grad=True); rank 0 saves the gathered arrays.

usage: gradient_job.py BACKEND M N MAX_ITER rhs.npy w0.npy OUT [DECOMP]  ->  OUT.r<rank>.json / .w.npy / .g.npy"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, solve  # noqa: E402


def main(argv) -> int:
    backend, M, N, max_iter = argv[1], int(argv[2]), int(argv[3]), int(argv[4])
    f, g0, out = np.load(argv[5]), np.load(argv[6]), argv[7]
    prob = EllipseProblem(M, N)
    prob.max_iter = max_iter
    if backend == "hip":
        import torch

        with DeviceSession(prob, "rows") as session:
            dev = f"cuda:{session.device_index}"
            rep = session.solve(rhs=torch.from_numpy(f).to(dev), w0=torch.from_numpy(g0).to(dev), return_w="device",
                                return_grad="device")
            blk = session.block
            assert tuple(rep.w.shape) == (blk.nx, blk.ny) and tuple(rep.grad.shape) == (2, blk.nx, blk.ny)
            assert rep.w_origin == (blk.i0, blk.j0) and rep.grad.is_cuda
        w, g = rep.w.cpu().numpy(), rep.grad.cpu().numpy()
    else:
        rep = solve(prob, backend=backend, decomp=argv[8], rhs=f, w0=g0, return_w=True, return_grad=True)
        w, g = rep.w, rep.grad
    if w is not None:
        np.save(f"{out}.r{rep.rank}.w.npy", w)
    if g is not None:
        np.save(f"{out}.r{rep.rank}.g.npy", g)
    with open(f"{out}.r{rep.rank}.json", "w") as fh:
        json.dump(rep.to_dict(), fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
