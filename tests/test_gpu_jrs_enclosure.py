"""The JRS scalars on the device (tests/gpu_unit/libjrs_test.so: jrs_joint with the ocml directed
rounding and the hand-made div_dn / sqrt_dn / sqrt_up of interval.h) against their definition in high
precision — the cases, samples, exact values and slack of tests/test_jrs_enclosure.py — and against the
host build's 13 doubles to 1e-12 * max(1, |q0|)."""
import numpy as np
import pytest

import jrs_unit as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def outputs():
    return U.jrs_outputs(U.Lib(device=True))


def test_device_jrs_scalars_enclose_the_trajectory(outputs):
    U.check_jrs(outputs, print)


def test_device_jrs_scalars_match_the_host_build(outputs):
    host = U.jrs_outputs(U.Lib(device=False))
    q0 = U.fixture()["cases"][:, 0]
    tol = 1e-12 * np.maximum(1.0, np.abs(q0))
    d = np.abs(outputs - host)
    print(f"device against host: worst |difference| {d.max():.3e}, in units of the tolerance {(d / tol[:, None]).max():.3e}")
    assert np.all(d <= tol[:, None]), np.argwhere(d > tol[:, None])[:5]
