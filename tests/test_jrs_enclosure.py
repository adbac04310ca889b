"""The JRS scalars (reach.h jrs_joint, host build of tests/gpu_unit/jrs_test.hip: the fesetround side
of interval.h that the emulation runs) against their definition in high precision.

For joint 0 of the built-in Kinova at T = 10, starts from 0 to +-1000 rad (multiples of pi/2, multi-turn
angles, the ends of the continuous range) crossed with five rate pairs (rest and nearly-rest starts
included) and four intervals, twelve samples (t, k, e) each — the eight corners of the interval's ends,
k = +-k_range and e = +-1, and four interior points — must satisfy

    |cos(q(t; k) + e qe) - (cos_c + cos_k k/k_range)| <= |cos_e|      (likewise sin)
    |qd(t; k) + e qde    - (qd_c  + qd_k  k/k_range)| <= |qd_e|
    |qdd(t; k) + e qddae - (qdd_c + qdd_k k/k_range)| <= |qdd_e|

with q(t; k) the degree-5 Bernstein curve of tests/point_model.control_points evaluated by mpmath at 50
digits (tests/golden/jrs_samples.npz holds the exact values as (hi, lo) double pairs; compared in long
double). Slack: 16 * 2^-52 * max(1, |q0| + |qd0| + |qdd0|), for the round-to-nearest operations on the
centres.

Measured on the host build (2026-10-20, ROCm clang, x86-64): cos / sin excess at most 3.9e-17 (at the
corners of rest starts, where the radius is attained; 0.011 of the slack), otherwise negative; rate
excess at most 0.04 (qd, 5.4e-16) and 0.49 (qdd, 5.1e-15; at q0 = +-pi/2) of the slack. Before the
rates were taken about q0 = 0 beyond one turn (reach.h jrs_joint) the acceleration centre at
q0 = 3.5 pi, (qd0, qdd0) = (-1.39, 1), s = 0 missed by 5.0e-14, 1.04 of the slack: the Bernstein
differences rounded q0 + ... and lost |q0| ulps in rates that do not depend on q0.
"""
import numpy as np
import pytest

import jrs_unit as U


@pytest.fixture(scope="module")
def host():
    return U.Lib(device=False)


def test_fixture_is_what_the_generator_writes():
    """the committed exact values are mpmath's (skipped parts: none; without mpmath the fixture alone
    is checked for shape)"""
    fx = U.fixture()
    assert fx["cases"].shape == (12 * 5 * 4, 4) and fx["exact"].shape == (240, 12, 4, 2)
    try:
        import mpmath  # noqa: F401
    except ImportError:
        return
    import sys

    sys.path.insert(0, U.os.path.join(U.HERE, "golden"))
    import make_jrs_samples as G

    new = G.generate()
    assert sorted(new) == sorted(fx)
    for k in new:
        np.testing.assert_array_equal(new[k], fx[k], err_msg=k)


def test_host_jrs_scalars_enclose_the_trajectory(host):
    U.check_jrs(U.jrs_outputs(host), print)


def test_host_jrs_samples_reach_the_ends():
    """the sample set includes both interval ends, k = +-k_range and e = +-1"""
    p = U.fixture()["points"]
    c = U.fixture()["cases"]
    T = int(U.fixture()["consts"][0])
    ds = 1.0 / T
    assert np.all(p[:, :, 0].min(axis=1) == c[:, 3] * ds) and np.all(p[:, :, 0].max(axis=1) == (c[:, 3] + 1) * ds)
    for col in (1, 2):
        assert np.all(p[:, :, col].min(axis=1) == -1) and np.all(p[:, :, col].max(axis=1) == 1)
