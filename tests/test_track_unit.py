"""The host build of armour-dev_amd/csrc/track.h (tests/track_unit: the serial form the device kernels
instantiate) against tests/track_model.py, without a device.

  * the serial rollouts on the fixed case list of tests/track_cases.py, every output within TOL (the
    tolerance of the device tests; the host build and the model differ in the order of a few sums and
    in the rotation matrices' last bit);
  * the RNEA radius equals the model's radius, and encloses |u(corner) - u(nominal)| over 64 random
    sign corners of the parameter box (mass_i (1 +- dm), every inertia entry (1 +- dI), signs per link
    and per entry), the corner torques computed by point_model.rnea, which shares no code with either.
    Slack 1e-12: the rounding of a torque of tens of N m in fp64, 1e-14 relative, with a factor of ten.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import point_model as pm
import track_cases as TC
import track_model as TM
from armour_amd import robot_tables as RT

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = os.path.join(HERE, "track_unit")
NAME = "libtrack_test_host.so"
_vp = ctypes.c_void_p
NF = 7


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


@pytest.fixture(scope="module")
def host():
    if not os.path.exists(os.path.join(UNIT, NAME)):   # built by __graft_entry__.build(); cheap
        subprocess.run(["make", "-C", UNIT, NAME], check=True, capture_output=True)
    L = ctypes.CDLL(os.path.join(UNIT, NAME))
    L.track_host_rollouts.argtypes = [_vp, ctypes.c_int, _vp, ctypes.c_int, _vp, _vp, ctypes.c_double, ctypes.c_double,
                                      ctypes.c_int, _vp, _vp]
    L.track_host_rnea.argtypes = [_vp, ctypes.c_int, _vp, _vp, _vp, _vp, _vp, ctypes.c_int, ctypes.c_int, _vp, _vp]
    return L


def host_rollouts(L, tb, traj, scale, err0, t0, t1, steps):
    traj = np.ascontiguousarray(traj, dtype=np.float64)
    N = traj.shape[0]
    S = 1 if scale is None and err0 is None else (scale if scale is not None else err0).shape[1]
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float64)
    err0 = None if err0 is None else np.ascontiguousarray(err0, dtype=np.float64)
    R = N * S
    out = np.full(37 * R, np.nan)
    st = np.full(R, -1, dtype=np.int32)
    s = RT.to_struct(tb)
    assert L.track_host_rollouts(ctypes.byref(s), N, _p(traj), S, _p(scale), _p(err0), t0, t1, steps, _p(out), _p(st)) == 0
    return dict(max_pos_err=out[:7 * R].reshape(N, S, NF), max_vel_err=out[7 * R:14 * R].reshape(N, S, NF),
                max_torque=out[14 * R:21 * R].reshape(N, S, NF), max_V=out[21 * R:22 * R].reshape(N, S),
                max_robust=out[22 * R:23 * R].reshape(N, S), end_state=out[23 * R:].reshape(N, S, 2, NF), status=st.reshape(N, S))


@pytest.mark.parametrize("window", TC.WINDOWS)
@pytest.mark.parametrize("robot", TC.ROBOTS)
def test_serial_rollouts_follow_the_model(host, robot, window):
    ref = TC.reference(robot, window)
    for shape in TC.SHAPES:
        tb, traj, scale, err0 = TC.case_inputs(robot, shape)
        got = host_rollouts(host, tb, traj, scale, err0, window[0], window[1], TC.STEPS)
        assert not got["status"].any() and not ref[shape]["status"].any()
        for k in TC.FIELDS:
            d = np.abs(got[k] - ref[shape][k]).max()
            print(f"{robot} {shape} {window} {k}: {d:.2e} (tol {TC.TOL[k]:.2e})")
            assert d <= TC.TOL[k], (robot, shape, window, k, d)


def test_null_scale_and_err0_are_ones_and_zeros(host):
    tb, traj, scale, err0 = TC.case_inputs("kinova", (5, 1))
    a = host_rollouts(host, tb, traj, None, None, 0.0, 0.5, 10)
    b = host_rollouts(host, tb, traj, np.ones_like(scale), np.zeros_like(err0), 0.0, 0.5, 10)
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_a_rollout_that_stops_being_finite_keeps_its_last_state(host):
    """a start so far off that K e overflows: status 1 at the first record, the state it started with
    kept, every output finite, and the other rollouts of the batch untouched"""
    tb, traj, scale, err0 = TC.case_inputs("kinova", (3, 5))
    clean = host_rollouts(host, tb, traj, scale, err0, 0.0, 0.5, 10)
    bad = err0.copy()
    bad[1, 2, 0, 3] = 1e308
    got = host_rollouts(host, tb, traj, scale, bad, 0.0, 0.5, 10)
    want = np.zeros((3, 5), dtype=np.int32)
    want[1, 2] = 1
    assert np.array_equal(got["status"], want)
    for k in TC.FIELDS:
        assert np.all(np.isfinite(got[k])), k
        keep = np.ones((3, 5), dtype=bool)
        keep[1, 2] = False
        assert np.array_equal(got[k][keep], clean[k][keep]), k
    assert got["end_state"][1, 2, 0, 3] == 1e308 and np.all(got["max_torque"][1, 2] == 0)


@pytest.mark.parametrize("robot", ("kinova", "KINOVA_REV", "KINOVA_9", "fetch"))
def test_radius_equals_the_model_and_encloses_the_corners(host, robot):
    tb = TC.tables(robot)
    nj = int(tb["num_joints"])
    rng = np.random.default_rng(5)
    n, corners = 16, 64
    q, qd, qa, qdda = (np.ascontiguousarray(rng.uniform(-1.5, 1.5, (n, NF))) for _ in range(4))
    u = np.full((n, NF), np.nan)
    rho = np.full((n, NF), np.nan)
    s = RT.to_struct(tb)
    assert host.track_host_rnea(ctypes.byref(s), n, _p(q), _p(qd), _p(qa), _p(qdda), None, 1, 1, _p(u), _p(rho)) == 0
    um, rm = TM.rnea_radius(tb, q, qd, qa, qdda)
    assert np.abs(u - um).max() <= 1e-12 * max(1.0, np.abs(um).max())
    assert np.abs(rho - rm).max() <= 1e-12 * max(1.0, np.abs(rm).max())
    assert np.all(rho >= 0)
    dm, dI = float(tb["mass_uncertainty"]), float(tb["inertia_uncertainty"])
    sm = rng.choice([-1.0, 1.0], (n, corners, nj))
    sI = rng.choice([-1.0, 1.0], (n, corners, nj, 3, 3))
    mass = (tb["mass"] * (1 + dm * sm)).reshape(n * corners, nj)
    inertia = (tb["inertia"] * (1 + dI * sI)).reshape(n * corners, nj, 3, 3)
    rep = lambda x: np.repeat(x, corners, axis=0)   # noqa: E731
    uc = pm.rnea(tb, rep(q), rep(qd), rep(qa), rep(qdda), mass=mass, inertia=inertia).reshape(n, corners, NF)
    un = pm.rnea(tb, q, qd, qa, qdda)
    assert np.abs(un - u).max() <= 1e-12 * max(1.0, np.abs(un).max())   # the point RNEA itself
    excess = (np.abs(uc - un[:, None, :]) - rho[:, None, :]).max()
    print(f"{robot}: largest excess of a corner over the radius {excess:.3e}; smallest radius {rho.min():.3e}")
    assert excess <= 1e-12


def test_true_parameters_scale_mass_and_inertia(host):
    """the per-link scales reach the RNEA as mass_i * scale and inertia_i * scale (against point_model)"""
    tb = TC.tables("KINOVA_9")
    nj = int(tb["num_joints"])
    rng = np.random.default_rng(6)
    n = 8
    q, qd, qa, qdda = (np.ascontiguousarray(rng.uniform(-1.5, 1.5, (n, NF))) for _ in range(4))
    scale = np.ascontiguousarray(rng.uniform(0.8, 1.2, (n, 2, nj)))
    u = np.full((n, NF), np.nan)
    rho = np.full((n, NF), np.nan)
    s = RT.to_struct(tb)
    assert host.track_host_rnea(ctypes.byref(s), n, _p(q), _p(qd), _p(qa), _p(qdda), _p(scale), 1, 1, _p(u), _p(rho)) == 0
    want = pm.rnea(tb, q, qd, qa, qdda, mass=tb["mass"] * scale[:, 0], inertia=tb["inertia"] * scale[:, 1, :, None, None])
    assert np.abs(u - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
