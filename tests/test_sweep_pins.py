"""MI355X bit pins of the three-step sweep (kS3): the r, p and w planes, the 19
reduced sums, and the iteration count, w and recurrence residual of converged
solves, equal bit for bit (np.array_equal, no tolerance) to fixtures recorded
on the commit before the uniform march stopped recomputing its lateral
differences and row coefficients (tests/golden/sweep_pins/,
tools/record_sweep_pins.py).  That change alters no floating-point operation
and no sum order, so any bit that moves is a bug in it; the fp64 comparisons
of test_sweep_family.py and test_sweep_addressing.py would let a last-bit
difference through.

Cases, what each is there for and the assertions from the live item list that
uniform items — with the steady groups the case is about — are present:
pin_checks.py."""

import numpy as np
import pin_checks
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", pin_checks.NAMES)
def test_bits_equal_recorded(gpu, nat, name, tmp_path):
    with np.load(pin_checks.fixture_path(name)) as f:
        want = {k: f[k] for k in f.files}
    got = pin_checks.run_case(nat, name, tmp_path)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        differ = int((got[k].view(np.uint8) != want[k].view(np.uint8)).reshape(got[k].shape + (-1,)).any(axis=-1).sum())
        print(f"sweep-pin {name} {k}: {got[k].size} values, {differ} differ")
    for k in sorted(want):
        assert np.array_equal(got[k], want[k]), (name, k)
