"""armour_track_motion on the device against tests/tracked_model.py: planners at T = 10, max_obstacles = 3,
the case list of tests/tracked_cases.py: shapes (W, S) = (3, 5), (5, 1), (1, 17) (partial rows, one sample,
a rollout count that crosses a wave), mixed batches of worlds with 3, 0, 1, 3, 1 obstacles, 50 steps,
check_samples 2, 11 and 51, the windows [0, 0.5] and [0.5, 1] (and [0.5, 1] chained from the end state of
[0, 0.5], each side from its own), on the Kinova, KINOVA_REV and KINOVA_9.

Tolerances (tracked_cases.py has the rule and the measurement): the rollouts' fields as armour_track's
(track_cases.TOL); the recorded quantities 100 x the model's spread under one-ulp perturbations of every
input; the clearance additionally the rounding bound of its pair (about 1e-13 m). `where` is compared
where the model's runner-up exceeds twice the tolerance, which tests/test_tracked_model.py asserts for
the whole list on the CPU, so here it is compared everywhere. Flags and status are exact; the same CPU
test asserts that every flag's quantity sits further from its threshold than the tolerance.

Measured with tracked_model on a CPU (8 draws, the three windows, all shapes, check_samples 2, 11, 51),
the largest spread, and the tolerance (100 x the largest):

    robot       recorded (q, qd)   clearance
    kinova      5.6e-16            8.9e-16
    KINOVA_REV  8.9e-16            7.5e-16
    KINOVA_9    6.1e-16            7.3e-16
    tolerance   8.9e-14            8.9e-14 + the pair's rounding bound

Measured on the MI355X: the largest differences from the model were 3.5e-16 in the end state, 1.7e-13 in
max_torque, 1.3e-13 in max_robust and 3.7e-16 m in the clearance; `where`, flags and status equal in
every case.
"""
import ctypes
import os

import numpy as np
import pytest

import armour_amd as A
import track_cases as TC
import tracked_cases as KC
import tracked_model as KM
from test_gpu_track import kernel

pytestmark = pytest.mark.gpu
NF = 7
OUTPUTS = TC.FIELDS + ("status", "clearance", "where", "flags", "world_clearance", "world_where")
_PLANNERS = {}


def planner(robot, W):
    """a planner of `robot` for W worlds (one per robot and size, kept for the module)"""
    if (robot, W) not in _PLANNERS:
        _PLANNERS[(robot, W)] = A.Planner(T=10, max_obstacles=3, max_worlds=W, robot=None if robot == "kinova" else TC.tables(robot))
    return _PLANNERS[(robot, W)]


@pytest.fixture(scope="module", autouse=True)
def close_planners():
    yield
    for P in _PLANNERS.values():
        P.close()
    _PLANNERS.clear()


def batch(robot, shape):
    """the planner with the case's worlds as its last batch, and the case"""
    tb, traj, scale, err0, obs = KC.case_inputs(robot, shape)
    P = planner(robot, shape[0])
    P.reach_mixed(KC.worlds(traj, obs))
    return P, traj, scale, err0, obs


def same(a, b, keys=OUTPUTS):
    for k in keys:
        assert a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), k


def compare(tag, got, ref, worst=None):
    """parity of one call with the model in every field"""
    assert np.array_equal(got["status"], ref["status"]), tag
    for k in TC.FIELDS:
        d = float(np.abs(got[k] - ref[k]).max())
        if worst is not None:
            worst[k] = max(worst.get(k, 0.0), d)
        assert d <= TC.TOL[k], (tag, k, d, TC.TOL[k])
    fin = np.isfinite(ref["clearance"])
    assert np.array_equal(np.isfinite(got["clearance"]), fin), tag
    assert np.all(got["clearance"][~fin] == np.inf) and np.all(got["where"][~fin] == -1), tag
    if fin.any():
        d = np.abs(got["clearance"][fin] - ref["clearance"][fin])
        allowed = (KC.TOL["clearance"] + ref["bound"])[fin]
        if worst is not None:
            worst["clearance"] = max(worst.get("clearance", 0.0), float(d.max()))
        assert np.all(d <= allowed), (tag, "clearance", float((d / allowed).max()))
    assert np.array_equal(got["where"], ref["where"]), (tag, got["where"], ref["where"])
    assert np.array_equal(got["flags"], ref["flags"]), (tag, got["flags"], ref["flags"])
    wf = np.isfinite(ref["world_clearance"])
    assert np.array_equal(got["world_where"], ref["world_where"]), tag
    assert np.all(got["world_clearance"][~wf] == np.inf), tag
    # the world's value is its first best rollout's, bit for bit
    for w in np.nonzero(wf)[0]:
        s = got["world_where"][w, 0]
        assert got["world_clearance"][w] == got["clearance"][w, s] == got["clearance"][w].min(), (tag, w)
        assert np.array_equal(got["world_where"][w, 1:], got["where"][w, s]), (tag, w)


# ---- parity with the model, and the embedded outputs against armour_track ---------------------------
@pytest.mark.parametrize("shape", KC.SHAPES)
@pytest.mark.parametrize("robot", KC.ROBOTS)
def test_parity_with_the_model(robot, shape):
    P, traj, scale, err0, obs = batch(robot, shape)
    worst = {}
    first = None
    for window in ("first", "second", "chained"):
        t0, t1 = KC.WINDOWS[window]
        e0 = err0 if window != "chained" else KC.chained_err0(traj, first["end_state"])
        plain = P.track(traj, scale, e0, t0, t1, KC.STEPS)
        for C in KC.CHECKS:
            got = P.track_motion(traj, scale, e0, t0, t1, KC.STEPS, C)
            assert got["track_ms"] > 0 and got["check_ms"] > 0 and got["qe"] == plain["qe"]
            same(got, plain, TC.FIELDS + ("status",))      # the embedded outputs are armour_track's, bit for bit
            compare((robot, shape, window, C), got, KC.reference(robot, shape, window, C), worst)
            if window == "first" and C == 11:
                first = got
    print(robot, shape, " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


def test_parity_with_more_check_points_than_lanes():
    """tracked_cases' long record: 65 and 129 check points, the second and third trip of the finish kernel's
    lane-strided loop over them (its minimisers lie at check points 79 .. 81 of 129), with the tolerances and
    the admission of the list (tests/test_tracked_model.py asserts the latter for this case)"""
    tb, traj, scale, err0, obs = KC.long_inputs()
    t0, t1 = KC.LONG_WINDOW
    P = planner("kinova", 2)
    P.reach_mixed(KC.worlds(traj, obs))
    plain = P.track(traj, scale, err0, t0, t1, KC.LONG_STEPS)
    worst, got = {}, {}
    for C in KC.LONG_CHECKS:
        got[C] = P.track_motion(traj, scale, err0, t0, t1, KC.LONG_STEPS, C)
        same(got[C], plain, TC.FIELDS + ("status",))       # the rollouts are armour_track's, bit for bit
        compare(("long", C), got[C], KC.long_reference(C), worst)
    print("long record", " ".join(f"{k} {v:.2e}" for k, v in worst.items()), "where", got[129]["where"].reshape(-1, 3).tolist())
    half, full = got[65], got[129]
    # the even check points of 129 are the 65: a minimiser found among them is the same record, bit for bit
    even = full["where"][..., 0] % 2 == 0
    assert np.array_equal(full["where"][..., 0][even], 2 * half["where"][..., 0][even])
    assert full["clearance"][even].tobytes() == half["clearance"][even].tobytes()
    assert np.all(full["clearance"] <= half["clearance"])


# ---- bitwise agreement and independence -------------------------------------------------------------
@pytest.mark.parametrize("shape", KC.SHAPES)
def test_row_kernel_is_bitwise_the_serial_kernel_and_reruns(shape):
    for robot in ("kinova", "KINOVA_9"):
        P, traj, scale, err0, obs = batch(robot, shape)
        for C in (2, 11):
            with kernel(None, P, "_rec"):
                a = P.track_motion(traj, scale, err0, 0.5, 1.0, KC.STEPS, C)
                b = P.track_motion(traj, scale, err0, 0.5, 1.0, KC.STEPS, C)
            with kernel("serial", P, "_rec"):
                c = P.track_motion(traj, scale, err0, 0.5, 1.0, KC.STEPS, C)
            same(a, b)
            same(a, c)


def test_a_world_alone_is_bitwise_its_value_in_every_batch():
    for shape in ((3, 5), (5, 1)):
        P, traj, scale, err0, obs = batch("kinova", shape)
        full = P.track_motion(traj, scale, err0, 0.0, 0.5, KC.STEPS, 11)
        for w in range(shape[0]):
            Q = planner("kinova", 1)
            Q.reach_mixed(KC.worlds(traj[w:w + 1], obs[w:w + 1]))
            one = Q.track_motion(traj[w:w + 1], scale[w:w + 1], err0[w:w + 1], 0.0, 0.5, KC.STEPS, 11)
            for k in OUTPUTS:
                assert one[k][0].tobytes() == full[k][w].tobytes(), (shape, w, k)
            if len(obs[w]) == 0:
                assert np.all(one["clearance"] == np.inf) and np.all(one["where"] == -1)
                assert one["world_clearance"][0] == np.inf and np.all(one["world_where"] == -1)


def test_uniform_batch_and_batch_after_a_plan():
    """defined after any reach or plan entry, uniform or mixed: the same worlds give the same bits"""
    tb, traj, scale, err0, obs = KC.case_inputs("kinova", (5, 1))
    keep = [0, 3]                                            # the two worlds with 3 obstacles
    ws = KC.worlds(traj[keep], [obs[w] for w in keep])
    P = planner("kinova", 2)
    P.reach_mixed(ws)
    a = P.track_motion(traj[keep], scale[keep], err0[keep], 0.0, 0.5, KC.STEPS, 11)
    P.reach(ws)
    b = P.track_motion(traj[keep], scale[keep], err0[keep], 0.0, 0.5, KC.STEPS, 11)
    P.plan(ws)
    c = P.track_motion(traj[keep], scale[keep], err0[keep], 0.0, 0.5, KC.STEPS, 11)
    same(a, b)
    same(a, c)


# ---- against armour_check_motion --------------------------------------------------------------------
def test_nominal_clearance_is_within_the_tracking_error_of_check_motion():
    """at nominal parameters and zero err0: |true - desired| <= L sum_j max_pos_err[j] + the rounding bounds
    (the bound tests/test_tracked_model.py pins on the CPU)"""
    tb = KM._shaped(TC.tables("kinova"))
    nj = int(tb["num_joints"])
    L = np.abs(tb["trans"][:nj]).sum() + (np.abs(tb["link_center"][:nj]).sum(-1) + np.abs(tb["link_generators"][:nj]).sum(-1)).max()
    for shape in ((3, 5), (5, 1)):
        P, traj, _, _, obs = batch("kinova", shape)
        for t0, t1 in TC.WINDOWS:
            got = P.track_motion(traj, None, None, t0, t1, KC.STEPS, 11)
            des, _ = P.check_motion(traj, t0, t1, 11)
            ref = KM.track_motion(tb, traj, obs, None, None, t0, t1, KC.STEPS, 11)
            assert got["clearance"].shape == (shape[0], 1) and not got["status"].any()
            for w in range(shape[0]):
                if len(obs[w]) == 0:
                    assert got["clearance"][w, 0] == np.inf and des[w] == np.inf
                    continue
                allowed = L * got["max_pos_err"][w, 0].sum() + 2 * ref["bound"][w, 0]
                d = abs(got["clearance"][w, 0] - des[w])
                print(f"{shape} [{t0}, {t1}] world {w}: true {got['clearance'][w, 0]:+.6e} desired {des[w]:+.6e} diff {d:.2e} "
                      f"allowed {allowed:.2e}")
                assert d <= allowed


# ---- the flags --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", KC.FLAG_CASES)
def test_flag_cases(name):
    case, ref = KC.flag_reference(name)
    P = A.Planner(T=10, max_obstacles=3, max_worlds=1, robot=case["tables"] if name == "input" else None)
    try:
        P.reach_mixed(KC.worlds(case["traj"], case["obstacles"]))
        got = P.track_motion(case["traj"], case["scale"], case["err0"], case["window"][0], case["window"][1], KC.STEPS, case["C"])
    finally:
        P.close()
    print(name, "flags", got["flags"].tolist(), "clearance", got["clearance"].tolist(), "where", got["where"].tolist())
    compare(name, got, ref)
    assert got["flags"][0, case["rollout"]] & case["bit"]
    for s in case["others"]:
        assert not got["flags"][0, s] & case["bit"]
    if name == "collision":
        assert np.all(got["where"][0, :, 0] == 0) and np.all(got["clearance"] < 0)


def test_a_rollout_that_stops_being_finite_is_flagged_and_the_others_are_untouched():
    """a start so far off that K e overflows (finite inputs): NOT_FINITE, status 1, the state it started with
    in the record's limit test; every other rollout bitwise what it was; both kernels. The rollout sits in
    the world without obstacles."""
    P, traj, scale, err0, obs = batch("kinova", (3, 5))
    assert len(obs[1]) == 0
    bad = err0.copy()
    bad[1, 2, 0, 3] = 1e308
    keep = np.ones((3, 5), dtype=bool)
    keep[1, 2] = False
    for name in (None, "serial"):
        with kernel(name, P, "_rec"):
            clean = P.track_motion(traj, scale, err0, 0.0, 0.5, 10, 6)
            got = P.track_motion(traj, scale, bad, 0.0, 0.5, 10, 6)
        assert got["status"][1, 2] == 1 and not got["status"][keep].any()
        assert got["flags"][1, 2] & KM.NOT_FINITE and not (got["flags"][keep] & KM.NOT_FINITE).any()
        assert got["clearance"][1, 2] == np.inf and got["end_state"][1, 2, 0, 3] == 1e308
        for k in TC.FIELDS + ("status", "clearance", "where", "flags"):
            assert np.array_equal(got[k][keep], clean[k][keep]), k
        same(got, clean, ("world_clearance", "world_where"))
    R = KM.track_motion(TC.tables("kinova"), traj, obs, scale, bad, 0.0, 0.5, 10, 6)
    assert np.array_equal(got["flags"], R["flags"]) and np.array_equal(got["status"], R["status"])


# ---- refusals and no side effects -------------------------------------------------------------------
def _raw(P, traj, S, steps, C, t0=0.0, t1=0.5):
    o = A.TrackMotionOutput()
    t = np.ascontiguousarray(traj, dtype=np.float64)
    rc = A.lib().armour_track_motion(P.h, A._ptr(t), S, None, None, float(t0), float(t1), int(steps), int(C), ctypes.byref(o))
    return rc, A.lib().armour_last_error().decode(), o


def test_state_and_argument_errors():
    tb, traj, scale, err0, obs = KC.case_inputs("kinova", (3, 5))
    Q = A.Planner(T=10, max_obstacles=3, max_worlds=3)
    rc, msg, _ = _raw(Q, traj, 1, 50, 11)
    assert rc == A.ARMOUR_E_STATE and "batch" in msg           # before any batch
    Q.reach_mixed(KC.worlds(traj, obs))
    rc, msg, o = _raw(Q, traj, 1, 50, 11)
    assert rc == 0 and o.check_ms > 0 and o.track.track_ms > 0  # (every output pointer is optional)
    for steps, C, word in ((50, 12, "multiple"), (50, 1, "check_samples"), (0, 2, "steps"), (A.TRACK_MAX_STEPS + 1, 2, "steps")):
        rc, msg, o = _raw(Q, traj, 1, steps, C)
        assert rc == A.ARMOUR_E_ARG and word in msg and o.check_ms == 0 and o.track.track_ms == 0, (steps, C, msg)
    rc, msg, _ = _raw(Q, traj, 0, 50, 11)
    assert rc == A.ARMOUR_E_ARG and "num_samples" in msg
    rc, msg, _ = _raw(Q, traj, 65536, 50, 11)
    assert rc == A.ARMOUR_E_ARG and "num_samples" in msg
    rc, msg, _ = _raw(Q, traj, 1, 50, 11, 0.5, 0.5)
    assert rc == A.ARMOUR_E_ARG and "window" in msg
    t = traj.copy()
    t[2, 3, 0] = np.nextafter(1.0, 2.0)
    rc, msg, _ = _raw(Q, t, 1, 50, 11)
    assert rc == A.ARMOUR_E_ARG and "k" in msg
    with pytest.raises(A.ArmourError, match="multiple"):
        Q.track_motion(traj, scale, err0, 0.0, 0.5, 50, 4)
    Q.close()
    Q = A.ArmtdPlanner(T=10, max_obstacles=3, max_worlds=3)
    rc, msg, _ = _raw(Q, traj, 1, 50, 11)
    assert rc == A.ARMOUR_E_ARG and "ARMTD" in msg
    Q.close()
    os.environ["ARMOUR_EVAL_F32"] = "1"
    try:
        Q = A.Planner(T=10, max_obstacles=3, max_worlds=3)
    finally:
        os.environ.pop("ARMOUR_EVAL_F32", None)
    rc, msg, _ = _raw(Q, traj, 1, 50, 11)
    assert rc == A.ARMOUR_E_ARG and "fp32" in msg
    Q.close()


def test_plan_state_is_untouched():
    """the getters and the next plan are what they would have been, against a second planner that never tracked;
    the calls include the first use, one that grows the buffers, and a smaller one in the larger buffers"""
    tb, traj, scale, err0, obs = KC.case_inputs("kinova", (3, 5))
    ws = KC.worlds(traj, obs)
    tracked = []

    def plans(with_track):
        P = A.Planner(T=10, max_obstacles=3, max_worlds=3)
        r1, _ = P.plan_mixed(ws)
        g1 = [P.constraints(w) for w in range(3)]
        if with_track:
            tracked.append(P.track_motion(traj, scale[:, :2], err0[:, :2], 0.0, 0.5, 10, 3))
            tracked.append(P.track_motion(traj, scale, err0, 0.5, 1.0, KC.STEPS, 51))
            tracked.append(P.track_motion(traj, scale[:, :2], err0[:, :2], 0.0, 0.5, 10, 3))
        g2 = [P.constraints(w) for w in range(3)]
        c2 = [P.link_centers(w) for w in range(3)]
        r2, _ = P.plan_mixed(ws)
        g3 = [P.constraints(w) for w in range(3)]
        P.close()
        return r1, g1, g2, c2, r2, g3

    a, b = plans(True), plans(False)
    for x, y in zip(a[1] + a[2] + a[3] + a[5], b[1] + b[2] + b[3] + b[5]):
        assert np.array_equal(x, y)
    for ra, rb in ((a[0], b[0]), (a[4], b[4])):
        for x, y in zip(ra, rb):
            assert np.array_equal(x["k_opt"], y["k_opt"]) and x["iterations"] == y["iterations"] and x["feasible"] == y["feasible"]
    same(tracked[0], tracked[2])
    compare("after a plan", tracked[1], KC.reference("kinova", (3, 5), "second", 51))
