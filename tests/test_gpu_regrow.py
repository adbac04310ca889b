"""The planner's grow-on-demand buffers and its creation-time settings on the GPU.

armour_eval_candidates, armour_check_motion and armour_track allocate their buffers on first use and
regrow them when a call brings more candidates, samples or rollouts (planner.hip GrowSet; the
tracking buffers' grow step is in test_gpu_track.py). Growing, and then using the larger buffers for
a small call again, must not change a bit of any output: every call here is compared with a fresh
planner that makes only that call. A batch the input check refuses leaves no batch state behind, and
the next plan is a fresh planner's. Settings are read when the planner is created: a change of
ARMOUR_ROW_CHUNK afterwards does not reach it.

Shapes: two worlds of two obstacles, T = 10 (the shortest horizon test_gpu_edge plans at)."""
import os

import numpy as np
import pytest

import armour_amd as A
from paths import assert_paths

pytestmark = pytest.mark.gpu
T, O = 10, 2
WORLDS = [A.make_world(900 + s, O) for s in range(2)]
KC = 32  # candidates per block of cand_rows (nlp_kernels.hip CAND_KC)


def planner(T=T):
    return A.Planner(T=T, max_obstacles=O, max_worlds=len(WORLDS))


def same(a, b):
    """bitwise equality of two outputs (arrays, tuples of arrays or dicts of arrays)"""
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def plan_record(P, res):
    return ([(r["k_opt"], r["cost"], r["iterations"], r["evaluations"], r["status"], r["feasible"], r["kkt"]) for r in res],
            [P.constraints(w) for w in range(len(res))], [P.link_centers(w) for w in range(len(res))])


def candidates(N):
    return np.random.default_rng(N).uniform(-1.0, 1.0, (len(WORLDS), N, 7))


def trajectories():
    k = np.random.default_rng(7).uniform(-0.5, 0.5, (len(WORLDS), 7))
    return np.array([[w[0], w[1], w[2], k[i]] for i, w in enumerate(WORLDS)])


def test_candidate_buffers_regrow_without_changing_a_bit():
    sizes = [1, KC + 1, 1]   # first use, one full chunk plus one (a regrow), then a small call in the larger buffers
    P = planner()
    P.plan(WORLDS)
    got = [P.eval_candidates(candidates(N)) for N in sizes]
    P.close()
    for N, g in zip(sizes, got):
        Q = planner()
        Q.plan(WORLDS)
        ref = Q.eval_candidates(candidates(N))
        Q.close()
        assert g["cost"].shape == (len(WORLDS), N)
        assert same(g, ref), N


def test_motion_buffers_regrow_without_changing_a_bit():
    sizes = [2, 13, 2]
    traj = trajectories()
    P = planner()
    P.plan(WORLDS)
    got = [P.check_motion(traj, 0.0, 1.0, S) for S in sizes]
    P.close()
    for S, g in zip(sizes, got):
        Q = planner()
        Q.plan(WORLDS)
        ref = Q.check_motion(traj, 0.0, 1.0, S)
        Q.close()
        assert np.isfinite(g[0]).all() and (g[1][:, 0] < S).all()
        assert same(g, ref), S


def test_a_refused_batch_leaves_no_state_and_the_next_plan_is_a_fresh_planners():
    Q = planner()
    ref = plan_record(Q, Q.plan(WORLDS)[0])
    Q.close()
    P = planner()
    P.plan(WORLDS)
    q0 = WORLDS[1][0].copy()
    q0[3] = np.nan
    bad = [WORLDS[0], (q0,) + tuple(WORLDS[1][1:])]
    with pytest.raises(A.ArmourError, match=r"armour error %d: q0\[3\] is not finite" % A.ARMOUR_E_ARG):
        P.plan(bad)
    with pytest.raises(A.ArmourError, match="armour error %d:" % A.ARMOUR_E_STATE):
        P.eval_constraints(0, np.zeros(7))
    assert same(plan_record(P, P.plan(WORLDS)[0]), ref)
    P.close()


def test_row_chunk_is_fixed_when_the_planner_is_created():
    """ARMOUR_ROW_CHUNK sizes the row passes' partial-sum buffers, so it is read at creation only. At
    T = 14 a world has 98 torque + 14 * 7 * 2 collision + 28 extremum rows + 7 variables = 329 rows:
    one block of 1024 rows, two of 256 (at T = 10 the 245 rows are one block either way, and the
    test could not tell the settings apart). A planner created under 1024 and planned with the
    variable at 256 gives bitwise the plan of one that never saw the change."""
    prev = os.environ.get("ARMOUR_ROW_CHUNK")
    try:
        os.environ["ARMOUR_ROW_CHUNK"] = "1024"
        P, Q = planner(14), planner(14)
        ref = plan_record(Q, Q.plan(WORLDS)[0])
        ref_paths = Q.path_counts()
        Q.close()
        os.environ["ARMOUR_ROW_CHUNK"] = "256"
        got = plan_record(P, P.plan(WORLDS)[0])
        got_paths = P.path_counts()
        P.close()
    finally:
        if prev is None:
            os.environ.pop("ARMOUR_ROW_CHUNK", None)
        else:
            os.environ["ARMOUR_ROW_CHUNK"] = prev
    assert same(got, ref)
    # and the same launches, one by one: the row passes of both ran on one block per world
    assert_paths(got_paths, ran=("ipm_iter_sync", "da_regs"), not_ran=("da_lds",))
    assert got_paths == ref_paths, (got_paths, ref_paths)
