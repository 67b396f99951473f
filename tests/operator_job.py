"""One rank of the multi-process tests of apply_operator / residual (launched
with torch.distributed.run): every rank loads the same global operand and
right-hand side, applies the operator and forms the residual, and saves its
share.

  hip       a DeviceSession on DECOMP, the fields as tensors on this rank's
            device, out="device": saves this rank's blocks and their origin.
  dist-cpu  apply_operator / residual(backend="dist-cpu"); rank 0 saves the fields.

usage: operator_job.py BACKEND M N v.npy rhs.npy OUT DECOMP  ->  OUT.r<rank>.json / .a.npy / .r.npy"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, apply_operator, residual  # noqa: E402


def main(argv) -> int:
    backend, M, N = argv[1], int(argv[2]), int(argv[3])
    v, f, out, decomp = np.load(argv[4]), np.load(argv[5]), argv[6], argv[7]
    prob = EllipseProblem(M, N)
    origin = None
    if backend == "hip":
        import torch

        with DeviceSession(prob, decomp) as session:
            dev = f"cuda:{session.device_index}"
            vt, ft = torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)
            a = session.apply(vt, out="device")
            r = session.residual(vt, rhs=ft, out="device")
            blk, rank = session.block, session.rank
            for res in (a, r):
                assert res.field.is_cuda and tuple(res.field.shape) == (blk.nx, blk.ny) and res.origin == (blk.i0, blk.j0)
            origin = a.origin
        af, rf = a.field.cpu().numpy(), r.field.cpu().numpy()
    else:
        from poisson_ellipse_openmp_mpi_cuda_amd.parallel import dist

        a = apply_operator(prob, v, backend=backend, decomp=decomp)
        r = residual(prob, v, rhs=f, backend=backend, decomp=decomp)
        rank = dist.init().rank
        af, rf = a.field, r.field
        assert (af is None) == (rank != 0) and (rf is None) == (rank != 0)
    if af is not None:
        np.save(f"{out}.r{rank}.a.npy", af)
        np.save(f"{out}.r{rank}.r.npy", rf)
    with open(f"{out}.r{rank}.json", "w") as fh:
        json.dump(dict(rank=rank, origin=origin, apply_sum=a.sum, resid_sum=r.sum), fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
