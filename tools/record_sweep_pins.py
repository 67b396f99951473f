#!/usr/bin/env python3
"""Record the fixtures of tests/test_sweep_pins.py (tests/golden/sweep_pins/*.npz).

Run on an MI355X from a checkout whose kS3 is the one to pin — the fixtures in
the repository were recorded on the commit before the uniform march's lateral
differences and per-item row coefficients (tests/pin_checks.py copied into
that checkout's tests/).

usage: tools/record_sweep_pins.py [OUTDIR]   (default: tests/golden/sweep_pins)
"""
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pin_checks  # noqa: E402

import poisson_ellipse_openmp_mpi_cuda_amd as pe  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else pin_checks.GOLDEN
    os.makedirs(out, exist_ok=True)
    nat = pe.native()
    nat.set_device(0)
    for name in pin_checks.NAMES:
        with tempfile.TemporaryDirectory() as tmp:
            got = pin_checks.run_case(nat, name, tmp)
        path = os.path.join(out, name + ".npz")
        np.savez_compressed(path, **got)
        print(f"{name}: {', '.join(f'{k}{list(v.shape)}' for k, v in got.items())} -> {os.path.getsize(path)} bytes",
              flush=True)


if __name__ == "__main__":
    main()
