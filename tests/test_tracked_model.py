"""tests/tracked_model.py, the yardstick of the armour_track_motion tests, and the conditions its case list
(tests/tracked_cases.py) has to meet, on the CPU:

  * with the record on, the rollouts are track_model's bit for bit;
  * at nominal parameters and zero err0 the true arm's clearance differs from the desired arm's
    (episode_model.clearance at the same times) by at most L * sum_j max_pos_err[j] plus the two rounding
    bounds, L the lever-arm bound of episode_model.fk_bound: a model whose record was taken at the wrong
    stage, or whose forward kinematics read another state, would fail here;
  * every rollout of the list and of the flag cases sits further from each flag's threshold, and from
    clearance 0, than the tolerance the device test allows; the minimiser is unique beyond twice the
    tolerance (or tied exactly, by equal states), no minimiser is a fragile pair, and each flag case
    raises its bit where it should and only there. The list is fixed, not filtered at run time.
"""
import numpy as np
import pytest

import episode_model as E
import track_cases as TC
import track_model as TM
import tracked_cases as KC
import tracked_model as KM


@pytest.mark.parametrize("window", TC.WINDOWS)
def test_the_record_leaves_the_rollouts_bitwise(window):
    tb, traj, scale, err0, _ = TC.flat_inputs("kinova")
    R = TM.Rollouts(tb, traj, scale, err0)
    want = R.run(window[0], window[1], TC.STEPS)
    for C in (2, 11):
        got, rec = KM.run_recorded(R, window[0], window[1], TC.STEPS, C)
        for k in TC.FIELDS + ("status",):
            assert got[k].tobytes() == want[k].tobytes(), (C, k)
        assert rec.shape == (C, R.R, 2, 7)
        assert np.array_equal(rec[-1], want["end_state"])
        start = KC.desired_state(traj, window[0]) + err0
        assert np.abs(rec[0] - start).max() <= 4 * 2.0 ** -52 * np.abs(start).max()


def test_nominal_true_clearance_stays_within_the_tracking_error_of_the_desired_one():
    tb = KM._shaped(TC.tables("kinova"))
    nj = int(tb["num_joints"])
    L = np.abs(tb["trans"][:nj]).sum() + (np.abs(tb["link_center"][:nj]).sum(-1) + np.abs(tb["link_generators"][:nj]).sum(-1)).max()
    worst = 0.0
    for shape in ((3, 5), (5, 1)):
        _, traj, _, _, obs = KC.case_inputs("kinova", shape)
        for t0, t1 in TC.WINDOWS:
            out = KM.track_motion(tb, traj, obs, None, None, t0, t1, KC.STEPS, 11)
            assert not out["status"].any() and not out["flags"][out["clearance"] > 0].any()
            for w in range(shape[0]):
                des = E.clearance(tb, tuple(traj[w]), obs[w], t0, t1, 11)
                if len(obs[w]) == 0:
                    assert out["clearance"][w, 0] == np.inf and des["clearance"] == np.inf
                    continue
                allowed = L * out["max_pos_err"][w, 0].sum() + des["bound"] + out["bound"][w, 0]
                d = abs(out["clearance"][w, 0] - des["clearance"])
                print(f"{shape} [{t0}, {t1}] world {w}: true {out['clearance'][w, 0]:+.6e} desired {des['clearance']:+.6e} "
                      f"diff {d:.2e} allowed {allowed:.2e}")
                assert d <= allowed
                worst = max(worst, d / allowed)
    assert worst > 0   # (the two are not the same computation)


def check_case(tag, ref, bits=()):
    """the conditions on one case's model outputs; bits: {(w, s): bit that must be raised}"""
    tol_c = KC.TOL["clearance"] + ref["bound"]
    fin = np.isfinite(ref["clearance"])
    assert not ref["fragile"].any(), tag
    assert np.all(np.abs(ref["clearance"][fin]) > tol_c[fin]), (tag, "a clearance inside the tolerance of 0")
    assert np.all(ref["runner_up"][fin] > 2 * tol_c[fin]), (tag, "a minimiser that is not unique beyond the tolerance")
    for w in range(ref["clearance"].shape[0]):
        v = np.unique(ref["clearance"][w][fin[w]])
        assert v.size < 2 or np.diff(v).min() > 2 * tol_c[w].max(), (tag, w, "samples neither tied nor apart")
    m = ref["margins"]
    assert np.all(np.abs(m[KM.INPUT]) > TC.TOL["max_torque"]), tag
    assert np.all(np.abs(m[KM.BOUND]) > max(TC.TOL["max_pos_err"], TC.TOL["max_vel_err"])), tag
    assert np.all(np.abs(m[KM.LIMIT]) > KC.TOL["rec"]), tag
    for (w, s), bit in bits:
        assert ref["flags"][w, s] & bit, (tag, w, s, bit)


@pytest.mark.parametrize("robot", KC.ROBOTS)
def test_the_list_sits_clear_of_every_threshold(robot):
    assert all(KC.TOL[k] == 100 * KC.SPREAD[k] and 0 < KC.SPREAD[k] < TC.ADMISSION for k in KC.SPREAD)
    for shape in KC.SHAPES:
        for window in KC.WINDOWS:
            for C in KC.CHECKS:
                ref = KC.reference(robot, shape, window, C)
                assert not ref["status"].any()
                check_case((robot, shape, window, C), ref)
                counts = np.array(KC.COUNTS[:shape[0]])
                assert np.all(np.isfinite(ref["clearance"]) == (counts > 0)[:, None])
                assert np.all((ref["world_where"] >= 0).all(axis=1) == (counts > 0))


def test_the_long_record_sits_clear_of_every_threshold():
    """the case with more check points than a wave has lanes meets the list's conditions, and its 65 check
    points are the even ones of its 129"""
    full, half = (KC.long_reference(C) for C in reversed(KC.LONG_CHECKS))
    for C, ref in zip(reversed(KC.LONG_CHECKS), (full, half)):
        assert ref["rec"].shape[0] == C and not ref["status"].any()
        check_case(("long", C), ref)
        assert np.all(np.isfinite(ref["clearance"]))
    assert np.array_equal(full["rec"][::2], half["rec"])
    # some minimiser lies past the first trip of a lane-strided loop over the check points
    assert full["where"][..., 0].max() >= 64 or half["where"][..., 0].max() >= 64


@pytest.mark.parametrize("name", KC.FLAG_CASES)
def test_each_flag_case_raises_its_flag_and_only_where_it_should(name):
    case, ref = KC.flag_reference(name)
    S = ref["flags"].shape[1]
    raised = [s for s in range(S) if s not in case["others"]] if name in ("collision", "input") else [case["rollout"]]
    check_case(name, ref, [((0, s), case["bit"]) for s in raised])
    for s in case["others"]:
        assert not ref["flags"][0, s] & case["bit"], (name, s)
    assert not ref["status"].any()
    if name == "collision":
        assert np.all(ref["where"][0, :, 0] == 0) and np.all(ref["where"][0, :, 1] == 4) and ref["world_where"][0, 1] == 0
    if name == "bound":
        assert ref["flags"][0, 1] == KM.BOUND


def test_episode_steps_of_the_model():
    """a tracked world without obstacles over a plan, its braking half and a step at rest: the true arms end
    near the desired state, the record accumulates, a start 1.5 qe off raises BOUND at step 0 and stops the
    world only when asked to"""
    tb = KM._shaped(TC.tables("kinova"))
    qe, _ = KM.thresholds(tb)
    q0 = TC.trajectories(1, 7)[0, 0]
    goal = q0 + 0.5
    world = (q0, np.zeros(7), np.zeros(7), q0, np.zeros((0, 12)))
    scale = np.ones((3, 2, int(tb["num_joints"])))
    scale[1], scale[2] = 1.03, 0.97
    st = E.begin(tb, world, goal)
    tr = KM.episode_begin(st, 3)
    k = np.full(7, 0.5)
    seen = []
    for step, accept in enumerate((True, False, False)):
        seg = KM.episode_segment(st, k, accept)
        assert seg[1] == ((0.0, 0.5), (0.5, 1.0), (0.0, 0.5))[step]
        st, tr, so = KM.episode_step(tb, st, tr, k, accept, world[4], goal, scale, steps=50)
        assert st["status"] == 0 and st["steps"] == step + 1 and tr["flags"] == 0 and tr["clearance"] == np.inf
        assert np.abs(tr["true"][:, 0] - st["q"]).max() < qe and np.all(tr["max_pos_err"] < qe)
        seen.append(tr["max_pos_err"].copy())
    assert np.all(seen[1] >= seen[0]) and np.all(seen[2] >= seen[1]) and seen[0].max() > 0
    assert np.all(st["qd"] == 0) and st["mode"] == 0
    err0 = np.zeros((3, 2, 7))
    err0[1, 0, 2] = 1.5 * qe
    for stop, status in ((1, 6), (0, 0)):
        s0 = E.begin(tb, world, goal)
        s1, t1, so = KM.episode_step(tb, s0, KM.episode_begin(s0, 3, err0), k, True, world[4], goal, scale, steps=50, stops=(1, stop, 0))
        assert s1["status"] == status and t1["flags"] == KM.BOUND and t1["flag_step"] == [-1, -1, 0, -1, -1]
        assert t1["last_flags"].tolist() == [0, KM.BOUND, 0]
        frozen, t2, none = KM.episode_step(tb, s1, t1, k, True, world[4], goal, scale, steps=50, stops=(1, stop, 0))
        assert (none is None) == bool(stop)


def test_one_draw_of_the_spread_is_within_the_table():
    w = KC.measure_spread(draws=1, robots=("kinova",), shapes=((3, 5),), report=lambda s: None)["kinova"]
    for k in KC.SPREAD:
        assert w[k] <= KC.SPREAD[k], (k, w[k])
