"""One rank of test_two_processes_with_device_fields (launched with
torch.distributed.run): load the global fields onto this rank's device, solve
through a DeviceSession with return_w="device", check the planes the solver
cut against block_fields and save this rank's block and report.

usage: device_fields_job.py M N rhs.npy w0.npy OUT   ->  OUT.r<rank>.npy / .json"""

import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from poisson_ellipse_openmp_mpi_cuda_amd import DeviceSession, EllipseProblem, native  # noqa: E402


def main(argv) -> int:
    M, N = int(argv[1]), int(argv[2])
    f, g, out = np.load(argv[3]), np.load(argv[4]), argv[5]
    prob = EllipseProblem(M, N)
    nat = native()
    with DeviceSession(prob, "rows") as session:
        dev = f"cuda:{session.device_index}"
        rep = session.solve(rhs=torch.from_numpy(f).to(dev), w0=torch.from_numpy(g).to(dev), return_w="device")
        want_f, want_g = nat.block_fields(M, N, session.block, f, g)
        planes_equal = bool(np.array_equal(session.solver.user_plane(0), want_f)
                            and np.array_equal(session.solver.user_plane(1), want_g))
        blk = session.block
        assert tuple(rep.w.shape) == (blk.nx, blk.ny) and rep.w_origin == (blk.i0, blk.j0)
    d = rep.to_dict()
    d.update(planes_equal=planes_equal, w_is_cuda=bool(rep.w.is_cuda))
    np.save(f"{out}.r{rep.rank}.npy", rep.w.cpu().numpy())
    with open(f"{out}.r{rep.rank}.json", "w") as fh:
        json.dump(d, fh)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
