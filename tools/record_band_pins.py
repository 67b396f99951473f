#!/usr/bin/env python3
"""Record the fixtures of tests/test_band_pins.py (tests/golden/band_pins/*.npz).

Run on an MI355X from a checkout whose kS3 is the one to pin — the fixtures in
the repository were recorded on the commit before the band march's steady
groups and per-row state (tests/band_checks.py copied into that checkout's
tests/).

usage: tools/record_band_pins.py [OUTDIR]   (default: tests/golden/band_pins)
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import band_checks  # noqa: E402
import numpy as np  # noqa: E402

import poisson_ellipse_openmp_mpi_cuda_amd as pe  # noqa: E402


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else band_checks.GOLDEN
    os.makedirs(out, exist_ok=True)
    nat = pe.native()
    nat.set_device(0)
    for name in band_checks.NAMES:
        got = band_checks.run_case(nat, name)
        path = os.path.join(out, name + ".npz")
        np.savez_compressed(path, **got)
        print(f"{name}: {', '.join(f'{k}{list(v.shape)}' for k, v in got.items())} -> {os.path.getsize(path)} bytes",
              flush=True)


if __name__ == "__main__":
    main()
