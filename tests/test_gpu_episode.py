"""Receding-horizon episodes on the GPU (armour_episode_begin / _step / _get) against the existing
planning entry and the numpy model (tests/episode_model.py).

Saved worlds 0-7 at T = 20 (one mixed batch, 5-10 obstacles), check_samples = 11:
  (i)   the results of each of the first 12 steps are bitwise those of plan_mixed on a second planner
        for the states read before the step;
  (ii)  after every step the states equal the model applied to the previous states and the device's
        own k_opt: q, qd, qdd and q_des within 64 eps (|q0| + |qd0| + |qdd0| + k_range) per joint
        (the advance at t = 0.5 and t = 1 uses Bernstein weights that are exact in binary, the
        waypoint a 7-term norm), status, mode and counters exactly;
  (iii) all 8 reach their goals within 90 steps (the oracle-driven loop needed at most 75) without a
        failed plan, with a positive clearance equal to the model's running minimum;
  (iv)  a vetoed plan (reject) makes the world brake along [0.5, 1] of its previous plan, to rest exactly;
        a second veto leaves it in place; then it resumes;
  (v)   a world whose first plan fails from a moving start gets status 3 and is frozen;
  (vi)  frozen worlds do not change, and between steps eval_candidates at k_opt reproduces the
        results' cost and feasibility (the planned batch is what the evaluation kernels see);
  (vii) plan() ends the episode: step and get then return ARMOUR_E_STATE.

Measured on the MI355X: the 8 worlds take 66, 65, 75, 56, 58, 34, 60 and 67 steps (the oracle-driven
loop: 66 for world 0) with clearances 0.107, 0.077, 0.044, 0.062, 0.072, 0.074, 0.054 and 0.018 m.
"""
import os

import numpy as np
import pytest

import armour_amd as A
import episode_model as E
from test_episode_model import saved

pytestmark = pytest.mark.gpu

T = 20
EPS = 2.0 ** -52
FIELDS = ("feasible", "status", "iterations", "evaluations", "cost", "kkt", "error")
INTS = ("status", "mode", "steps", "failed_plans", "failed_streak")
HERE = os.path.dirname(os.path.abspath(__file__))


def world_states(st, w):
    return {k: (v[w].copy() if isinstance(v[w], np.ndarray) else v[w]) for k, v in st.items()}


def planning_worlds(st, worlds):
    return [(st["q"][w], st["qd"][w], st["qdd"][w], st["q_des"][w], worlds[w][4]) for w in range(len(worlds))]


def model_input(st, w, pending):
    s = world_states(st, w)
    s["clearance_at"] = tuple(int(v) for v in s["clearance_at"])
    s["pending"] = pending
    return s


def assert_follows_model(robot, before, after, res, accept, worlds, goals, pending, tag, clearance_tol):
    """(ii) for every world of one step; returns the new pending plans"""
    out = []
    for w in range(len(worlds)):
        prev = model_input(before, w, pending[w])
        m = E.step(robot, prev, res[w]["k_opt"], bool(accept[w]), worlds[w][4], goals[w])
        tol = 64 * EPS * (np.abs(prev["q"]) + np.abs(prev["qd"]) + np.abs(prev["qdd"]) + E.K_RANGE)
        for k in ("q", "qd", "qdd", "q_des"):
            assert np.all(np.abs(after[k][w] - m[k]) <= tol), (tag, w, k, after[k][w] - m[k])
        for k in INTS:
            assert int(after[k][w]) == int(m[k]), (tag, w, k, int(after[k][w]), int(m[k]))
        assert abs(after["goal_distance"][w] - m["goal_distance"]) <= tol.sum(), (tag, w)
        if np.isfinite(m["clearance"]):
            assert abs(after["clearance"][w] - m["clearance"]) <= clearance_tol, (tag, w, after["clearance"][w], m["clearance"])
        else:
            assert after["clearance"][w] == m["clearance"]
        out.append(m["pending"])
    return out


def assert_bitwise(got, want, tag):
    for w, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(a["k_opt"], b["k_opt"]), (tag, w, a["k_opt"] - b["k_opt"])
        for k in FIELDS:
            assert a[k] == b[k], (tag, w, k, a[k], b[k])


@pytest.fixture(scope="module")
def run():
    """one episode of saved worlds 0-7 to the end, recorded step by step; (i), (ii) and (vi) are
    asserted while it runs, once"""
    robot = E.kinova()
    pairs = [saved(i) for i in range(8)]
    worlds, goals = [p[0] for p in pairs], np.array([p[1] for p in pairs])
    O = max(len(w[4]) for w in worlds)
    P = A.Planner(T=T, max_obstacles=O, max_worlds=8)
    P2 = A.Planner(T=T, max_obstacles=O, max_worlds=8)
    st = P.episode_begin(worlds, goals, check_samples=11)
    for w in range(8):
        # csv_world's first waypoint (its norm is numpy's, the device's a sequential sum: an ulp)
        np.testing.assert_allclose(st["q_des"][w], worlds[w][3], rtol=0, atol=8 * EPS)
        np.testing.assert_allclose(st["q_des"][w], E.waypoint(robot, worlds[w][0], goals[w]), rtol=0, atol=8 * EPS)
        assert st["status"][w] == 0 and st["mode"][w] == 0 and st["clearance"][w] == np.inf
    pending = [None] * 8
    history = [st]
    timings, plans = [], []
    running = 8
    for step in range(90):
        if running == 0:
            break
        before = history[-1]
        running, res, tm = P.episode_step()
        after = P.episode_states()
        assert running == int(np.sum(after["status"] == 0))
        if step < 12:   # (i)
            want, _ = P2.plan_mixed(planning_worlds(before, worlds))
            assert_bitwise(res, want, f"step {step}")
        accept = [r["feasible"] for r in res]
        pending = assert_follows_model(robot, before, after, res, accept, worlds, goals, pending, f"step {step}", 1e-12)
        for w in range(8):   # (vi) frozen worlds do not change
            if before["status"][w] != 0:
                for k in before:
                    assert np.array_equal(before[k][w], after[k][w]), (step, w, k)
        if step in (1, 6):   # (vi) the evaluation kernels see the batch that was planned
            k_opt = np.array([r["k_opt"] for r in res])
            out = P.eval_candidates(k_opt[:, None, :])
            np.testing.assert_allclose(out["cost"][:, 0], [r["cost"] for r in res], rtol=0, atol=1e-12)
            assert np.array_equal(out["feasible"][:, 0], np.array([r["feasible"] for r in res]))
            g = P.constraints(3)
            assert g.shape == (P.num_constraints(len(worlds[3][4])),) and np.all(np.isfinite(g))
        history.append(after)
        timings.append(tm)
        plans.append(np.array([r["k_opt"] for r in res]))
    yield dict(P=P, P2=P2, worlds=worlds, goals=goals, history=history, timings=timings, plans=plans, robot=robot)
    P.close()
    P2.close()


def test_plans_and_states_follow_entry_and_model(run):
    """(i), (ii), (vi): asserted step by step inside the fixture; here: it ran, and timed its parts"""
    assert len(run["history"]) > 12
    tm = run["timings"][0]
    assert tm["check_ms"] > 0 and tm["advance_ms"] > 0 and tm["reach_ms"] > 0 and tm["nlp_ms"] > 0
    print("step 0 timing:", {k: round(v, 3) for k, v in tm.items()})


def test_episodes_finish(run):
    """(iii)"""
    last = run["history"][-1]
    print("steps", last["steps"], "clearance", np.round(last["clearance"], 4), "at", last["clearance_at"].tolist())
    assert np.all(last["status"] == 1), last["status"]
    assert len(run["history"]) - 1 <= 90 and np.all(last["steps"] <= 90)
    assert np.all(last["failed_plans"] == 0) and np.all(last["failed_streak"] == 0)
    assert np.all(last["clearance"] > 0)
    assert np.all(last["goal_distance"] <= np.pi / 30 + 0.1)   # (a sample of the last segment was inside the radius)
    # the running minimum of the model over every executed segment (each within 1e-12 m of the
    # device's: the rounding bound of test_gpu_check_motion.py on these worlds is below that)
    robot, worlds = run["robot"], run["worlds"]
    for w in range(8):
        best, at = np.inf, (-1, -1, -1)
        for s in range(int(last["steps"][w])):
            b = run["history"][s]
            c = E.clearance(robot, (b["q"][w], b["qd"][w], b["qdd"][w], run["plans"][s][w]), worlds[w][4], 0.0, 0.5, 11)
            if c["clearance"] < best:
                best, at = c["clearance"], (s, c["where"][1], c["where"][2])
        assert abs(last["clearance"][w] - best) <= 1e-12, (w, last["clearance"][w], best)
        assert tuple(last["clearance_at"][w]) == at, (w, last["clearance_at"][w], at)


def test_reject_and_braking(run):
    """(iv)"""
    robot, worlds, goals = run["robot"], run["worlds"], run["goals"]
    P = run["P2"]
    st = P.episode_begin(worlds, goals, check_samples=11)
    pending = [None] * 8
    k2 = q2 = None
    for step in range(7):
        reject = np.zeros(8, dtype=int)
        if step in (3, 4):
            reject[2] = 1
        before = st
        _, res, _ = P.episode_step(reject if step != 0 else None)
        st = P.episode_states()
        accept = [r["feasible"] and not reject[w] for w, r in enumerate(res)]
        pending = assert_follows_model(robot, before, st, res, accept, worlds, goals, pending, f"reject step {step}", 1e-12)
        assert res[2]["feasible"]   # (so that the veto, not the solver, decides what world 2 does)
        if step == 2:
            q2, k2 = before["q"][2].copy(), res[2]["k_opt"].copy()
            assert st["mode"][2] == 1
        if step == 3:   # the braking half of step 2's plan: at rest exactly at its end point
            assert np.array_equal(st["q"][2], q2 + k2 * E.K_RANGE)
            assert np.all(st["qd"][2] == 0) and np.all(st["qdd"][2] == 0)
            assert st["mode"][2] == 0 and st["failed_plans"][2] == 1 and st["failed_streak"][2] == 1 and st["steps"][2] == 4
        if step == 4:   # a second veto: in place
            for k in ("q", "qd", "qdd", "q_des", "clearance", "goal_distance"):
                assert np.array_equal(st[k][2], before[k][2]), k
            assert st["mode"][2] == 0 and st["failed_plans"][2] == 2 and st["failed_streak"][2] == 2 and st["steps"][2] == 5
        if step == 5:   # it resumes
            assert st["mode"][2] == 1 and st["failed_plans"][2] == 2 and st["failed_streak"][2] == 0 and st["steps"][2] == 6
            assert np.any(st["q"][2] != before["q"][2]) and np.any(st["qd"][2] != 0)


def test_no_fail_safe_from_a_moving_start():
    """(v): boundary_small_T20_O6 worlds 2 and 10 (graze_moving, infeasible at their moving start)"""
    fx = np.load(os.path.join(HERE, "golden", "boundary_small_T20_O6.npz"))
    idx = [2, 3, 10, 0]
    worlds = [tuple(fx[k][i] for k in ("q0", "qd0", "qdd0", "q_des", "obstacles")) for i in idx]
    goals = np.array([w[0] + 12 * (w[3] - w[0]) for w in worlds])
    P = A.Planner(T=T, max_obstacles=6, max_worlds=4)
    st0 = P.episode_begin(worlds, goals, check_samples=11)
    assert list(st0["mode"]) == [1, 1, 1, 0] and np.all(st0["status"] == 0)
    n, res, _ = P.episode_step()
    st = P.episode_states()
    assert [r["feasible"] for r in res] == [False, True, False, True]
    assert list(st["status"]) == [3, 0, 3, 0] and n == 2
    for w in (0, 2):
        assert st["failed_plans"][w] == 1 and st["steps"][w] == 0 and st["clearance"][w] == np.inf
        for k in ("q", "qd", "qdd", "q_des"):
            assert np.array_equal(st[k][w], st0[k][w])
    assert st["mode"][1] == 1 and st["mode"][3] == 1 and np.all(st["steps"][[1, 3]] == 1)
    n2, _, _ = P.episode_step()
    st2 = P.episode_states()
    for w in (0, 2):   # frozen
        for k in st:
            assert np.array_equal(st[k][w], st2[k][w]), (w, k)
    assert np.all(st2["steps"][[1, 3]] == 2)
    P.close()


def test_state_errors(run):
    """(vii), and the argument checks of begin"""
    worlds, goals = run["worlds"], run["goals"]
    P = A.Planner(T=T, max_obstacles=10, max_worlds=8)
    L = A.lib()
    st = (A.EpisodeState * 8)()
    assert L.armour_episode_step(P.h, None, None, None, None) == A.ARMOUR_E_STATE   # before a begin
    assert L.armour_episode_get(P.h, st) == A.ARMOUR_E_STATE
    P.episode_begin(worlds, goals)
    with pytest.raises(A.ArmourError):   # no batch has been planned yet
        P.constraints(0)
    assert L.armour_check_motion(P.h, A._ptr(np.zeros((8, 4, 7))), 0.0, 1.0, 3, None, None) == A.ARMOUR_E_STATE
    n, res, _ = P.episode_step()
    assert n == 8
    P.plan_mixed(worlds)   # any other plan entry ends the episode
    assert L.armour_episode_step(P.h, None, None, None, None) == A.ARMOUR_E_STATE
    assert L.armour_episode_get(P.h, st) == A.ARMOUR_E_STATE
    with pytest.raises(A.ArmourError, match="episode"):
        P.episode_step()
    # begin: bad goals, bad config, a world outside the input domain; q_des is ignored
    bad = goals.copy()
    bad[3, 2] = np.nan
    with pytest.raises(A.ArmourError, match="goals"):
        P.episode_begin(worlds, bad)
    bad[3, 2] = 2e4
    with pytest.raises(A.ArmourError, match="goals"):
        P.episode_begin(worlds, bad)
    for cfg in (dict(check_samples=1), dict(lookahead=0.0), dict(goal_radius=-1.0), dict(lookahead=np.nan)):
        with pytest.raises(A.ArmourError, match="config"):
            P.episode_begin(worlds, goals, **cfg)
    w0 = list(worlds[0])
    w0[1] = np.full(7, np.inf)
    with pytest.raises(A.ArmourError, match="qd0"):
        P.episode_begin([tuple(w0)] + worlds[1:], goals)
    w0 = list(worlds[0])
    w0[3] = np.full(7, np.nan)
    st1 = P.episode_begin([tuple(w0)] + worlds[1:], goals)
    assert np.all(np.isfinite(st1["q_des"]))
    # a world already inside the goal radius starts with status 1 and is never advanced
    near = goals.copy()
    near[5] = worlds[5][0] + 0.01
    st2 = P.episode_begin(worlds, near)
    assert st2["status"][5] == 1 and np.all(np.delete(st2["status"], 5) == 0)
    n, _, _ = P.episode_step()
    st3 = P.episode_states()
    assert n == 7 and st3["steps"][5] == 0 and np.array_equal(st3["q"][5], st2["q"][5])
    out = A.run_episodes(P, worlds[:2], goals[:2], max_steps=3)
    assert list(out["steps"]) == [3, 3] and out["status"].shape == (2,) and np.all(out["clearance"] > 0)
    P.close()
