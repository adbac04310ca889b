"""armour_track on the device: planners at T = 10, max_obstacles = 3, max_worlds = 1, 50 steps, the
shapes (N, S) = (3, 5), (5, 1), (1, 17) (partial rows and waves, and a rollout count that crosses a
wave) and the windows [0, 0.5] and [0.5, 1].

Parity runs the fixed case list of tests/track_cases.py against tests/track_model.py: the six kinds of
rollout on the built-in Kinova, KINOVA_REV and KINOVA_9, and the Fetch fixture with nominal parameters
and zero err0 only (quasi-static; see track_cases.FETCH_MOTION). A case is on the list when the model's
own spread under a one-ulp perturbation of every input is below 1e-9 in every output; the list is fixed
in that file and not filtered at run time. Measured with track_model on a CPU (8 draws, both windows,
all shapes), the largest spread per field:

    robot       max_pos_err  max_vel_err  max_torque  max_V     max_robust  end_state
    kinova      3.3e-16      2.2e-16      8.4e-14     5.5e-16   1.5e-13     4.4e-16
    KINOVA_REV  4.4e-16      3.3e-16      6.7e-14     9.6e-16   4.8e-14     6.7e-16
    KINOVA_9    2.2e-16      3.1e-16      9.5e-14     2.7e-16   1.2e-13     5.4e-16
    fetch       2.2e-15      7.8e-15      5.7e-14     1.6e-28   0           7.8e-15

The tolerance per field is 100 x the largest spread of that field (track_cases.TOL): the perturbation
stands for input rounding only; the device also differs in sin / cos by an ulp or two, over 200
chained stages. The mirror identity and the chaining test are held to the same tolerance.
"""
import ctypes
import os

import numpy as np
import pytest

import armour_amd as A
import robot_variants as RV
import track_cases as TC
from paths import TRACK_ROW, TRACK_SERIAL, assert_paths

pytestmark = pytest.mark.gpu
NF = 7
_PLANNERS = {}


def planner(robot):
    if robot not in _PLANNERS:
        _PLANNERS[robot] = A.Planner(T=10, max_obstacles=3, max_worlds=1, robot=None if robot == "kinova" else TC.tables(robot))
    return _PLANNERS[robot]


@pytest.fixture(scope="module", autouse=True)
def close_planners():
    yield
    for P in _PLANNERS.values():
        P.close()
    _PLANNERS.clear()


class kernel:
    """context manager: armour_track runs the serial kernel ("serial") or the default one (None). With
    the planner the body drives, the body's launches are checked on leaving it (the path census): only
    the kernel asked for, in its plain ("": armour_track), recording ("_rec": armour_track_motion) or
    episode ("_episode": a tracked episode's step) form"""

    def __init__(self, name, planner=None, form=""):
        self.name, self.planner, self.form = name, planner, form

    def __enter__(self):
        self.before = self.planner.path_counts() if self.planner is not None else None
        self.prev = os.environ.get("ARMOUR_TRACK_KERNEL")
        if self.name:
            os.environ["ARMOUR_TRACK_KERNEL"] = self.name
        else:
            os.environ.pop("ARMOUR_TRACK_KERNEL", None)

    def __exit__(self, *exc):
        if self.prev is None:
            os.environ.pop("ARMOUR_TRACK_KERNEL", None)
        else:
            os.environ["ARMOUR_TRACK_KERNEL"] = self.prev
        if self.planner is not None and exc[0] is None:
            after = self.planner.path_counts()
            mine = ("track_serial" if self.name == "serial" else "track_row") + self.form
            assert_paths({k: after[k] - self.before[k] for k in after}, ran=(mine,),
                         not_ran=tuple(n for n in TRACK_ROW + TRACK_SERIAL if n != mine))


def run(robot, shape, window, steps=TC.STEPS):
    tb, traj, scale, err0 = TC.case_inputs(robot, shape)
    return planner(robot).track(traj, scale, err0, window[0], window[1], steps)


# ---- 4. parity with the model --------------------------------------------------------------------
@pytest.mark.parametrize("window", TC.WINDOWS)
@pytest.mark.parametrize("robot", TC.ROBOTS)
def test_parity_with_the_model(robot, window):
    ref = TC.reference(robot, window)
    worst = {k: 0.0 for k in TC.FIELDS}
    for shape in TC.SHAPES:
        got = run(robot, shape, window)
        assert got["max_pos_err"].shape == shape + (NF,) and got["end_state"].shape == shape + (2, NF)
        assert not got["status"].any(), (robot, shape, window)
        assert got["track_ms"] > 0 and got["qe"] == pytest.approx(TC.qe_of(TC.tables(robot)), rel=1e-14)
        for k in TC.FIELDS:
            worst[k] = max(worst[k], float(np.abs(got[k] - ref[shape][k]).max()))
    print(robot, window, " ".join(f"{k} {v:.2e}/{TC.TOL[k]:.2e}" for k, v in worst.items()))
    for k in TC.FIELDS:
        assert worst[k] <= TC.TOL[k], (robot, window, k, worst[k], TC.TOL[k])


# ---- 5. bitwise agreement and isolation -----------------------------------------------------------
@pytest.mark.parametrize("window", TC.WINDOWS)
@pytest.mark.parametrize("shape", TC.SHAPES)
def test_row_kernel_is_bitwise_the_serial_kernel_and_reruns(shape, window):
    for robot in ("kinova", "KINOVA_9"):
        with kernel(None, planner(robot)):
            a = run(robot, shape, window)
            b = run(robot, shape, window)
        with kernel("serial", planner(robot)):
            c = run(robot, shape, window)
        for k in TC.FIELDS + ("status",):
            assert np.array_equal(a[k], b[k]), ("rerun", robot, k)
            assert np.array_equal(a[k], c[k]), ("serial", robot, k)


@pytest.mark.parametrize("name", (None, "serial"))
def test_a_rollout_alone_is_bitwise_its_value_in_every_batch(name):
    P = planner("kinova")
    with kernel(name, P):
        for shape in TC.SHAPES:
            tb, traj, scale, err0 = TC.case_inputs("kinova", shape)
            full = P.track(traj, scale, err0, 0.0, 0.5, TC.STEPS)
            for n in range(shape[0]):
                for s in range(shape[1]):
                    one = P.track(traj[n:n + 1], scale[n:n + 1, s:s + 1], err0[n:n + 1, s:s + 1], 0.0, 0.5, TC.STEPS)
                    for k in TC.FIELDS + ("status",):
                        assert np.array_equal(one[k][0, 0], full[k][n, s]), (shape, n, s, k)


def test_null_scale_and_err0_and_skipped_outputs():
    P = planner("kinova")
    tb, traj, scale, err0 = TC.case_inputs("kinova", (5, 1))
    a = P.track(traj, None, None, 0.0, 0.5, 10)
    b = P.track(traj, np.ones_like(scale), np.zeros_like(err0), 0.0, 0.5, 10)
    for k in TC.FIELDS + ("status",):
        assert np.array_equal(a[k], b[k]), k
    # every output pointer is optional
    out = A.TrackOutput()
    t = np.ascontiguousarray(traj)
    assert A.lib().armour_track(P.h, 5, A._ptr(t), 1, None, None, 0.0, 0.5, 10, ctypes.byref(out)) == 0
    assert out.track_ms > 0
    V = np.full(5, np.nan)
    out.max_V = A._ptr(V)
    assert A.lib().armour_track(P.h, 5, A._ptr(t), 1, None, None, 0.0, 0.5, 10, ctypes.byref(out)) == 0
    assert np.array_equal(V, a["max_V"][:, 0])


def test_a_rollout_that_stops_being_finite_keeps_its_last_state():
    """a start so far off that K e overflows (finite inputs, so the entry accepts it): status 1, the
    state it started with, finite outputs, the other rollouts bitwise untouched; both kernels"""
    P = planner("kinova")
    tb, traj, scale, err0 = TC.case_inputs("kinova", (3, 5))
    bad = err0.copy()
    bad[1, 2, 0, 3] = 1e308
    want = np.zeros((3, 5), dtype=np.int32)
    want[1, 2] = 1
    keep = want == 0
    for name in (None, "serial"):
        with kernel(name, P):
            clean = P.track(traj, scale, err0, 0.0, 0.5, 10)
            got = P.track(traj, scale, bad, 0.0, 0.5, 10)
        assert np.array_equal(got["status"], want)
        for k in TC.FIELDS:
            assert np.all(np.isfinite(got[k])), k
            assert np.array_equal(got[k][keep], clean[k][keep]), k
        assert got["end_state"][1, 2, 0, 3] == 1e308 and np.all(got["max_torque"][1, 2] == 0)


# ---- 6. the mirror identity -----------------------------------------------------------------------
@pytest.mark.parametrize("window", TC.WINDOWS)
def test_mirror_identity(window):
    joints = RV.SPECS["KINOVA_REV"][2]
    sg = RV.sigma(joints)
    for shape in TC.SHAPES:
        tb, traj, scale, err0 = TC.case_inputs("kinova", shape)
        a = planner("kinova").track(traj, scale, err0, window[0], window[1], TC.STEPS)
        b = planner("KINOVA_REV").track(traj * sg, scale, err0 * sg, window[0], window[1], TC.STEPS)
        assert not a["status"].any() and not b["status"].any()
        for k in ("max_pos_err", "max_vel_err", "max_torque", "max_V", "max_robust"):
            d = np.abs(a[k] - b[k]).max()
            assert d <= TC.TOL[k], (shape, k, d)
        d = np.abs(a["end_state"] * sg - b["end_state"]).max()
        assert d <= TC.TOL["end_state"], (shape, d)


# ---- 7. chaining ----------------------------------------------------------------------------------
def test_two_windows_chain_into_one():
    import point_model as pm

    P = planner("kinova")
    for shape in TC.SHAPES:
        tb, traj, scale, err0 = TC.case_inputs("kinova", shape)
        one = P.track(traj, scale, err0, 0.0, 0.5, 50)
        first = P.track(traj, scale, err0, 0.0, 0.25, 25)
        beta = pm.control_points(traj[:, 0], traj[:, 1], traj[:, 2], traj[:, 3] * TC.TM.K_RANGE)
        q, qd, _ = pm.bezier(beta, 0.25)
        mid = first["end_state"] - np.stack([q, qd], axis=1)[:, None]
        second = P.track(traj, scale, mid, 0.25, 0.5, 25)
        assert not (one["status"].any() or first["status"].any() or second["status"].any())
        d = np.abs(second["end_state"] - one["end_state"]).max()
        assert d <= TC.TOL["end_state"], (shape, d)
        for k in ("max_pos_err", "max_vel_err", "max_torque", "max_V", "max_robust"):
            d = np.abs(np.maximum(first[k], second[k]) - one[k]).max()
            assert d <= TC.TOL[k], (shape, k, d)


# ---- 8. refusals and no side effects ----------------------------------------------------------------
def _raw(P, N, traj, S, scale, err0, t0, t1, steps, out=True):
    o = A.TrackOutput()
    keep = [np.ascontiguousarray(v, dtype=np.float64) if v is not None else None for v in (traj, scale, err0)]
    rc = A.lib().armour_track(P.h if P is not None else None, N, A._ptr(keep[0]), S, A._ptr(keep[1]), A._ptr(keep[2]),
                              float(t0), float(t1), int(steps), ctypes.byref(o) if out else None)
    return rc, A.lib().armour_last_error().decode()


def test_refusals():
    P = planner("kinova")
    tb, traj, scale, err0 = TC.case_inputs("kinova", (3, 5))
    good = (P, 3, traj, 5, scale, err0, 0.0, 0.5, 10)
    assert _raw(*good)[0] == 0

    def refused(word, **change):
        names = ("P", "N", "traj", "S", "scale", "err0", "t0", "t1", "steps")
        args = dict(zip(names, good))
        out = change.pop("out", True)
        args.update(change)
        rc, msg = _raw(*[args[n] for n in names], out=out)
        assert rc == A.ARMOUR_E_ARG and word in msg, (change, rc, msg)

    refused("null", P=None)
    refused("null", traj=None)
    refused("null", out=False)
    refused("num_traj", N=0)
    refused("num_samples", S=0)
    for bad in (np.nan, np.inf, -np.inf):
        for field, word in ((0, "traj"), (1, "traj"), (2, "traj"), (3, "traj")):
            t = traj.copy()
            t[2, field, 6] = bad
            refused(word, traj=t)
        s = scale.copy()
        s[2, 4, 1, 6] = bad
        refused("scale", scale=s)
        e = err0.copy()
        e[2, 4, 1, 6] = bad
        refused("err0", err0=e)
    t = traj.copy()
    t[1, 3, 0] = np.nextafter(1.0, 2.0)
    refused("k", traj=t)
    t = traj.copy()
    t[1, 0, 0] = -np.nextafter(1e4, 2e4)
    refused("ARMOUR_MAX_ABS_ANGLE", traj=t)
    for bad in (0.0, -1.0):
        s = scale.copy()
        s[0, 0, 0, 0] = bad
        refused("scale", scale=s)
    refused("steps", steps=0)
    refused("steps", steps=A.TRACK_MAX_STEPS + 1)
    for t0, t1 in ((-0.1, 0.5), (0.5, 0.5), (0.6, 0.5), (0.5, np.nextafter(1.0, 2.0)), (np.nan, 0.5), (0.0, np.nan)):
        refused("window", t0=t0, t1=t1)
    assert _raw(*good)[0] == 0
    Q = A.ArmtdPlanner(T=10, max_obstacles=3, max_worlds=1)
    rc, msg = _raw(Q, *good[1:])
    assert rc == A.ARMOUR_E_ARG and "ARMTD" in msg
    Q.close()
    os.environ["ARMOUR_EVAL_F32"] = "1"
    try:
        Q = A.Planner(T=10, max_obstacles=3, max_worlds=1)
    finally:
        os.environ.pop("ARMOUR_EVAL_F32", None)
    rc, msg = _raw(Q, *good[1:])
    assert rc == A.ARMOUR_E_ARG and "fp32" in msg
    Q.close()


def test_tracking_leaves_the_batch_and_the_next_plan_unchanged():
    world = A.make_world(3, 3)
    tb, traj, scale, err0 = TC.case_inputs("kinova", (3, 5))
    # first use, a call that grows the buffers, and the first call again in the larger buffers
    calls = [(traj, scale, err0, 0.0, 0.5, TC.STEPS), (np.repeat(traj, 40, axis=0), None, None, 0.5, 1.0, 5),
             (traj, scale, err0, 0.0, 0.5, TC.STEPS)]
    tracked = []

    def plans(with_track):
        P = A.Planner(T=10, max_obstacles=3, max_worlds=1)
        r1, _ = P.plan([world])
        g1 = P.constraints(0)
        if with_track:
            tracked.extend(P.track(*c) for c in calls)
        g2 = P.constraints(0)
        c2 = P.link_centers(0)
        r2, _ = P.plan([world])
        g3 = P.constraints(0)
        P.close()
        return r1, g1, g2, c2, r2, g3

    a, b = plans(True), plans(False)
    assert np.array_equal(a[1], a[2])
    for x, y in zip(a[1:4] + a[5:], b[1:4] + b[5:]):
        assert np.array_equal(x, y)
    for ra, rb in ((a[0], b[0]), (a[4], b[4])):
        assert np.array_equal(ra[0]["k_opt"], rb[0]["k_opt"]) and ra[0]["iterations"] == rb[0]["iterations"]
    # every tracking output, before and after the grow, is bitwise a fresh planner's that makes only that call
    for c, out in zip(calls[:2], tracked[:2]):
        Q = A.Planner(T=10, max_obstacles=3, max_worlds=1)
        ref = Q.track(*c)
        Q.close()
        for k in TC.FIELDS + ("status",):
            assert out[k].shape == ref[k].shape and out[k].tobytes() == ref[k].tobytes(), k
    for k in TC.FIELDS + ("status",):
        assert tracked[2][k].tobytes() == tracked[0][k].tobytes(), k


def test_tracking_needs_no_batch():
    P = A.Planner(T=10, max_obstacles=3, max_worlds=1)
    tb, traj, scale, err0 = TC.case_inputs("kinova", (5, 1))
    out = P.track(traj, scale, err0, 0.0, 0.5, 10)
    assert not out["status"].any()
    with pytest.raises(A.ArmourError):
        P.constraints(0)
    P.close()
