"""One rank of the multi-process test of the reaction field (launched with
torch.distributed.run): every rank loads the same global rhs, w0 and field c,
runs a fixed number of iterations of (A + diag(c)) w = B through a
DeviceSession — the fields as tensors on this rank's device,
return_w="device" — and saves its report and its block.

usage: reaction_job.py M N K rhs.npy w0.npy c.npy OUT DECOMP   ->  OUT.r<rank>.json / .npy"""

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

    M, N, K = int(argv[1]), int(argv[2]), int(argv[3])
    f, g, c, out, decomp = np.load(argv[4]), np.load(argv[5]), np.load(argv[6]), argv[7], argv[8]
    prob = EllipseProblem(M, N, max_iter=K)
    # (the host array at construction — the session's device is known only after it — the tensor per solve)
    with DeviceSession(prob, decomp, reaction=c, check_tol=False) as session:
        dev = f"cuda:{session.device_index}"
        rep = session.solve(rhs=torch.from_numpy(f).to(dev), w0=torch.from_numpy(g).to(dev), return_w="device",
                            reaction=torch.from_numpy(c).to(dev))
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
