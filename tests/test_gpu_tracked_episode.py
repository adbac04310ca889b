"""Tracked episodes on the GPU (armour_episode_track / armour_episode_get_tracked): saved worlds 0-3 at
T = 20 in one mixed batch, 3 true arms per world (armour_amd.uncertainty_samples: nominal, every link at the
top of the stated uncertainty, every link at the bottom), 50 steps and 11 check points per segment.

  (i)   every step to the end: the results and episode_states() are bitwise those of an untracked episode
        of the same worlds on a second planner (tracking does not feed back into planning);
  (ii)  the first 6 steps: after every step the true states and the records equal tests/tracked_model.py
        applied to the device's previous states (desired and true), its previous records and its own k_opt,
        as tests/test_gpu_episode.py compares the desired arm. One step is one window from a given start,
        which is what the tolerances of tests/track_cases.py and tests/tracked_cases.py were measured on
        (their list holds these three kinds of sample and a chained window), so those hold here: the
        rollouts' fields within track_cases.TOL (the true state as end_state), the clearance within
        tracked_cases.TOL plus the rounding bound of its pair; flags, flag steps and status exact. The saved
        worlds' obstacles are upright boxes, so a minimiser may be a fragile pair (episode_model.separations);
        such a clearance is not compared, and no step of this run has one (asserted);
  (iii) at the end every world has reached its goal with no flag set, max_pos_err < qe and a positive
        true clearance;
  (iv)  a veto at one step and a second one: the braking half [0.5, 1] and the at-rest segment are rolled
        out, compared with the model;
  (v)   an err0 of 1.5 qe on one joint of one world: status 6 at step 0 with stop_on_bound, the world frozen
        from then on; without it the world runs on with bit 4 set and flag_step 0;
  (vi)  episode_tracked() returns ARMOUR_E_STATE without episode_track and after plan() ends the episode;
  (vii) a serial-kernel run of the first 3 steps is bitwise the row-kernel run.
"""
import ctypes

import numpy as np
import pytest

import armour_amd as A
import episode_model as E
import track_cases as TC
import tracked_cases as KC
import tracked_model as KM
from test_episode_model import saved
from test_gpu_episode import model_input
from test_gpu_track import kernel

pytestmark = pytest.mark.gpu
T, S, STEPS, C = 20, 3, 50, 11
NF = 7
RECORD = ("clearance", "clearance_at", "max_pos_err", "max_vel_err", "max_torque", "max_V", "max_robust", "flags", "flag_step")


def setup():
    robot = E.kinova()
    pairs = [saved(i) for i in range(4)]
    worlds, goals = [p[0] for p in pairs], np.array([p[1] for p in pairs])
    scale = A.uncertainty_samples(robot, S)
    assert np.all(scale[0] == 1) and np.all(scale[1] > 1) and np.all(scale[2] < 1)
    return robot, worlds, goals, scale, max(len(w[4]) for w in worlds)


def tracked_input(tr, w):
    """the model's tracking state of world w from episode_tracked()"""
    return dict(true=tr["true_state"][w].copy(), clearance=float(tr["clearance"][w]),
                clearance_at=tuple(int(v) for v in tr["clearance_at"][w]), max_pos_err=tr["max_pos_err"][w].copy(),
                max_vel_err=tr["max_vel_err"][w].copy(), max_torque=tr["max_torque"][w].copy(), max_V=float(tr["max_V"][w]),
                max_robust=float(tr["max_robust"][w]), flags=int(tr["flags"][w]), flag_step=[int(v) for v in tr["flag_step"][w]],
                last_flags=tr["last_flags"][w].copy())


def assert_follows_model(robot, before, tr_before, after, tr_after, res, accept, worlds, goals, pending, scale, stops, tag):
    """(ii) for every world of one step; returns (the new pending plans, fragile minimisers met)"""
    W = len(worlds)
    prev = [model_input(before, w, pending[w]) for w in range(W)]
    tprev = [tracked_input(tr_before, w) for w in range(W)]
    segs = [KM.episode_segment(prev[w], res[w]["k_opt"], bool(accept[w])) for w in range(W)]
    rolled = KM.episode_rollouts(robot, segs, [t["true"] for t in tprev], [scale] * W, STEPS, C)
    out, fragile = [], 0
    for w in range(W):
        m = E.step(robot, prev[w], res[w]["k_opt"], bool(accept[w]), worlds[w][4], goals[w], check_samples=C)
        out.append(m["pending"])
        if segs[w] is None:
            for k in RECORD:
                assert np.array_equal(tr_after[k][w], tr_before[k][w]), (tag, w, k)
            assert np.array_equal(tr_after["true_state"][w], tr_before["true_state"][w]), (tag, w)
            assert int(after["status"][w]) == int(m["status"])
            continue
        m, t, so = KM.episode_fold(robot, prev[w], m, tprev[w], rolled[w], worlds[w][4], stops)
        assert not so["status"].any(), (tag, w)
        assert int(after["status"][w]) == int(m["status"]), (tag, w, int(after["status"][w]), int(m["status"]))
        d = np.abs(tr_after["true_state"][w] - t["true"]).max()
        assert d <= TC.TOL["end_state"], (tag, w, "true_state", d)
        for k in ("max_pos_err", "max_vel_err", "max_torque", "max_V", "max_robust"):
            d = np.abs(tr_after[k][w] - t[k]).max()
            assert d <= TC.TOL[k], (tag, w, k, d)
        assert np.array_equal(tr_after["last_flags"][w], t["last_flags"]), (tag, w)
        assert int(tr_after["flags"][w]) == t["flags"] and list(tr_after["flag_step"][w]) == t["flag_step"], (tag, w)
        assert np.all(np.abs(so["margins"][KM.INPUT]) > TC.TOL["max_torque"]) and np.all(np.abs(so["margins"][KM.BOUND]) > TC.TOL["max_pos_err"])
        if so["fragile"].any():
            fragile += 1
            continue
        tol = KC.TOL["clearance"] + so["bound"].max()
        assert abs(tr_after["clearance"][w] - t["clearance"]) <= tol, (tag, w, tr_after["clearance"][w], t["clearance"])
        if np.all(so["runner_up"] > 2 * tol) and abs(so["clearance"].min() - tprev[w]["clearance"]) > 2 * tol:
            assert tuple(tr_after["clearance_at"][w]) == t["clearance_at"], (tag, w, tr_after["clearance_at"][w], t["clearance_at"])
    return out, fragile


@pytest.fixture(scope="module")
def run():
    """one tracked episode of saved worlds 0-3 to the end beside an untracked one; (i) and (ii) are asserted
    while it runs, once"""
    robot, worlds, goals, scale, O = setup()
    P = A.Planner(T=T, max_obstacles=O, max_worlds=4)
    P2 = A.Planner(T=T, max_obstacles=O, max_worlds=4)
    st = P.episode_begin(worlds, goals, check_samples=C)
    P2.episode_begin(worlds, goals, check_samples=C)
    P.episode_track(scale=scale, steps=STEPS)
    tr = P.episode_tracked()
    assert np.all(tr["clearance"] == np.inf) and np.all(tr["flags"] == 0) and np.all(tr["flag_step"] == -1)
    assert np.array_equal(tr["true_state"][:, :, 0], np.repeat(st["q"][:, None], S, axis=1))
    assert np.array_equal(tr["true_state"][:, :, 1], np.repeat(st["qd"][:, None], S, axis=1))
    pending = [None] * 4
    running, steps, fragile = 4, 0, 0
    first_ms = None
    while running and steps < 90:
        running, res, tm = P.episode_step()
        n2, res2, _ = P2.episode_step()
        after, tr_after = P.episode_states(), P.episode_tracked()
        plain = P2.episode_states()
        assert running == n2
        for a, b in zip(res, res2):   # (i)
            assert np.array_equal(a["k_opt"], b["k_opt"]) and all(a[k] == b[k] for k in ("feasible", "status", "iterations", "cost"))
        for k in after:
            assert after[k].tobytes() == plain[k].tobytes(), (steps, k)
        if steps < 6:   # (ii)
            accept = [r["feasible"] for r in res]
            pending, f = assert_follows_model(robot, st, tr, after, tr_after, res, accept, worlds, goals, pending, scale, (1, 1, 0),
                                              f"step {steps}")
            fragile += f
        if first_ms is None:
            first_ms = (tr_after["rollout_ms"], tr_after["check_ms"], tm["check_ms"])
        st, tr = after, tr_after
        steps += 1
    assert fragile == 0
    yield dict(P=P, P2=P2, robot=robot, worlds=worlds, goals=goals, scale=scale, last=st, tracked=tr, steps=steps, ms=first_ms)
    P.close()
    P2.close()


def test_tracking_leaves_the_episode_bitwise_and_follows_the_model(run):
    """(i), (ii): asserted step by step inside the fixture; here: it ran, and timed its parts"""
    assert run["steps"] > 6
    print("step 0: rollouts %.3f ms, true-arm check %.3f ms, desired-arm check %.3f ms" % run["ms"])
    assert run["ms"][0] > 0 and run["ms"][1] > 0


def test_every_world_reaches_its_goal_inside_the_bounds(run):
    """(iii)"""
    last, tr = run["last"], run["tracked"]
    qe, qde = KM.thresholds(run["robot"])
    print("steps", last["steps"], "true clearance", np.round(tr["clearance"], 4), "desired", np.round(last["clearance"], 4),
          "max |e| / qe", np.round(tr["max_pos_err"].max(axis=1) / qe, 4), "max V", tr["max_V"], "max torque", np.round(tr["max_torque"].max(axis=1), 2))
    assert np.all(last["status"] == 1), last["status"]
    assert np.all(tr["flags"] == 0) and np.all(tr["flag_step"] == -1) and np.all(tr["last_flags"] == 0)
    assert np.all(tr["max_pos_err"] < qe) and np.all(tr["max_vel_err"] < qde)
    assert np.all(tr["clearance"] > 0) and np.all(tr["clearance_at"] >= 0)
    assert np.all(tr["clearance_at"][:, 0] < last["steps"]) and np.all(tr["clearance_at"][:, 1] < S)
    # the true arm stays within the tracking error of the desired one
    assert np.all(np.abs(tr["clearance"] - last["clearance"]) < 2.0 * qe * NF)


def test_vetoes_roll_out_the_braking_half_and_the_arm_at_rest(run):
    """(iv)"""
    robot, worlds, goals, scale, P = run["robot"], run["worlds"], run["goals"], run["scale"], run["P2"]
    st = P.episode_begin(worlds, goals, check_samples=C)
    P.episode_track(scale=scale, steps=STEPS)
    tr = P.episode_tracked()
    pending = [None] * 4
    for step in range(5):
        reject = np.zeros(4, dtype=int)
        if step in (2, 3):
            reject[1] = 1
        _, res, _ = P.episode_step(reject)
        after, tr_after = P.episode_states(), P.episode_tracked()
        assert res[1]["feasible"]
        accept = [r["feasible"] and not reject[w] for w, r in enumerate(res)]
        if step in (2, 3):
            seg = KM.episode_segment(model_input(st, 1, pending[1]), res[1]["k_opt"], False)
            assert seg[1] == ((0.5, 1.0) if step == 2 else (0.0, 0.5))
            if step == 3:   # at rest: the constant trajectory at the state, and the true arms keep moving toward it
                assert all(np.all(v == 0) for v in seg[0][1:]) and np.array_equal(seg[0][0], st["q"][1])
                assert np.any(tr_after["true_state"][1] != tr["true_state"][1])
        pending, f = assert_follows_model(robot, st, tr, after, tr_after, res, accept, worlds, goals, pending, scale, (1, 1, 0),
                                          f"veto step {step}")
        assert f == 0
        st, tr = after, tr_after
    assert st["steps"][1] == 5 and st["failed_plans"][1] == 2 and np.all(tr["flags"] == 0)


@pytest.mark.parametrize("stop", (True, False))
def test_a_start_outside_the_ultimate_bound(run, stop):
    """(v)"""
    robot, worlds, goals, scale, P = run["robot"], run["worlds"], run["goals"], run["scale"], run["P2"]
    qe, _ = KM.thresholds(robot)
    err0 = np.zeros((4, S, 2, NF))
    err0[2, 1, 0, 3] = 1.5 * qe
    st0 = P.episode_begin(worlds, goals, check_samples=C)
    P.episode_track(scale=scale, err0=err0, steps=STEPS, stop_on_bound=stop)
    tr0 = P.episode_tracked()
    assert tr0["true_state"][2, 1, 0, 3] == st0["q"][2, 3] + 1.5 * qe
    n, res, _ = P.episode_step()
    st, tr = P.episode_states(), P.episode_tracked()
    assert_follows_model(robot, st0, tr0, st, tr, res, [r["feasible"] for r in res], worlds, goals, [None] * 4, scale,
                         (1, int(stop), 0), f"bound stop {stop}")
    assert tr["flags"][2] == KM.BOUND and tr["flag_step"][2].tolist() == [-1, -1, 0, -1, -1]
    assert tr["last_flags"][2].tolist() == [0, KM.BOUND, 0] and np.all(np.delete(tr["flags"], 2) == 0)
    assert st["status"].tolist() == ([0, 0, 6, 0] if stop else [0, 0, 0, 0]) and n == (3 if stop else 4)
    n, _, _ = P.episode_step()
    st2, tr2 = P.episode_states(), P.episode_tracked()
    if stop:   # frozen: neither the state nor the true arms nor the record move
        for k in st:
            assert np.array_equal(st[k][2], st2[k][2]), k
        for k in RECORD + ("true_state", "last_flags"):
            assert np.array_equal(tr[k][2], tr2[k][2]), k
        assert st2["steps"].tolist() == [2, 2, 1, 2]
    else:
        assert st2["status"][2] == 0 and st2["steps"][2] == 2 and tr2["flags"][2] == KM.BOUND and tr2["flag_step"][2, 2] == 0
        assert np.any(tr2["true_state"][2] != tr["true_state"][2])


def test_state_errors(run):
    """(vi), and the argument checks of episode_track"""
    worlds, goals, scale = run["worlds"], run["goals"], run["scale"]
    P = A.Planner(T=T, max_obstacles=10, max_worlds=4)
    L = A.lib()
    rec = (A.EpisodeTracked * 4)()
    cfg = A.EpisodeTrackConfig(S, None, None, STEPS, 1, 1, 0)
    assert L.armour_episode_track(P.h, ctypes.byref(cfg)) == A.ARMOUR_E_STATE          # before a begin
    assert L.armour_episode_get_tracked(P.h, rec, None, None, None) == A.ARMOUR_E_STATE
    P.episode_begin(worlds, goals, check_samples=C)
    assert L.armour_episode_get_tracked(P.h, rec, None, None, None) == A.ARMOUR_E_STATE   # tracking is not enabled
    assert b"not enabled" in L.armour_last_error()
    for bad, word in ((dict(steps=55), "multiple"), (dict(steps=0), "steps"), (dict(num_samples=0), "num_samples")):
        with pytest.raises(A.ArmourError, match=word):
            P.episode_track(**{**dict(steps=STEPS, num_samples=S), **bad})
    s = np.broadcast_to(scale, (4,) + scale.shape).copy()
    s[3, 2, 1, 6] = 0.0
    with pytest.raises(A.ArmourError, match="scale"):
        P.episode_track(scale=s, steps=STEPS)
    e = np.zeros((4, S, 2, NF))
    e[0, 0, 1, 0] = np.nan
    with pytest.raises(A.ArmourError, match="err0"):
        P.episode_track(err0=e, steps=STEPS)
    with pytest.raises(ValueError, match="scale"):
        P.episode_track(scale=np.ones((3, S, 2, 7)), steps=STEPS)
    P.episode_track(scale=scale, steps=STEPS)
    assert L.armour_episode_get_tracked(P.h, rec, None, None, None) == 0 and rec[0].clearance == np.inf
    P.episode_step()
    assert L.armour_episode_track(P.h, ctypes.byref(cfg)) == A.ARMOUR_E_STATE          # after the first step
    assert P.episode_tracked()["clearance"].shape == (4,)
    P.plan_mixed(worlds)   # any other plan entry ends the episode
    assert L.armour_episode_get_tracked(P.h, rec, None, None, None) == A.ARMOUR_E_STATE
    with pytest.raises(A.ArmourError, match="episode"):
        P.episode_tracked()
    # a new begin ends the tracking; run_episodes with track returns the records
    P.episode_begin(worlds, goals, check_samples=C)
    assert L.armour_episode_get_tracked(P.h, rec, None, None, None) == A.ARMOUR_E_STATE
    out = A.run_episodes(P, worlds[:2], goals[:2], max_steps=2, track=dict(scale=scale, steps=STEPS), check_samples=C)
    assert list(out["steps"]) == [2, 2] and out["tracked"]["true_state"].shape == (2, S, 2, NF) and np.all(out["tracked"]["clearance"] > 0)
    P.close()


def test_serial_kernel_is_bitwise_the_row_kernel(run):
    """(vii)"""
    worlds, goals, scale, P = run["worlds"], run["goals"], run["scale"], run["P2"]
    got = {}
    for name in (None, "serial"):
        with kernel(name, P, "_episode"):
            P.episode_begin(worlds, goals, check_samples=C)
            P.episode_track(scale=scale, steps=STEPS)
            for _ in range(3):
                P.episode_step()
            got[name] = (P.episode_states(), P.episode_tracked())
    for k, v in got[None][0].items():
        assert v.tobytes() == got["serial"][0][k].tobytes(), k
    for k in RECORD + ("true_state", "last_flags"):
        assert got[None][1][k].tobytes() == got["serial"][1][k].tobytes(), k
