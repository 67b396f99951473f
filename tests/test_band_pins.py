"""MI355X bit pins of the three-step sweep's band march (kS3, items that hold
a boundary-band row): the r, p and w planes, the 19 reduced sums, and the
iteration count, w and recurrence residual of whole solves, equal bit for bit
(np.array_equal, no tolerance) to fixtures recorded on the commit before the
band march got steady groups and took a row's class and coefficients once
(tests/golden/band_pins/, tools/record_band_pins.py).  That change alters no
floating-point operation and no sum order, so any bit that moves is a bug in
it.

Cases, what each is there for and the assertions from the live item list that
band items — with the steady groups the case is about — are present:
band_checks.py."""

import band_checks
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", band_checks.NAMES)
def test_bits_equal_recorded(gpu, nat, name):
    with np.load(band_checks.fixture_path(name)) as f:
        want = {k: f[k] for k in f.files}
    got = band_checks.run_case(nat, name)
    assert sorted(got) == sorted(want)
    for k in sorted(want):
        assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype, k
        differ = int((got[k].view(np.uint8) != want[k].view(np.uint8)).reshape(got[k].shape + (-1,)).any(axis=-1).sum())
        print(f"band-pin {name} {k}: {got[k].size} values, {differ} differ")
    for k in sorted(want):
        assert np.array_equal(got[k], want[k]), (name, k)
