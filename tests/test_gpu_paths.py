"""The host's dispatch decisions at their boundaries, by the path census (Planner.path_counts): on each
side of a threshold the predicted path ran, and the results are right (against the oracle, or bitwise
against the setting that switches the path off). And the census of the default dispatch on small
batches, written out, so that a change of the default paths is made on purpose.

T = 20 throughout; at most 6 obstacles and 256 worlds, except the nine-joint batch whose 360 (link,
obstacle) pairs are the case."""
import numpy as np
import pytest

import armour_amd as A
import robot_variants as RV
from armour_amd import robot_tables as RT
from oracle import OraclePlanner
from paths import JOB, LANE, assert_paths, taken
from test_boundary import load, world
from test_gpu_parity import TOL
from test_gpu_plane_cache import env

pytestmark = pytest.mark.gpu
T = 20
_oracle = {}


def plain(s):
    """a world of three obstacles whose plan converges in 6 to 9 iterations without a restoration phase"""
    return A.make_world(900 + s, 3)


def oracle(s, max_iter=0):
    """(the oracle after reach(), its plan) of plain(s), computed once and left unchanged"""
    if s not in _oracle:
        R = OraclePlanner(*plain(s), T=T, threads=4)
        R.reach()
        _oracle[s] = (R, {})
    R, plans = _oracle[s]
    if max_iter not in plans:
        plans[max_iter] = R.plan(max_iter=max_iter)
    return R, plans[max_iter]


def assert_bitwise(P, Q, ra, rb):
    for w, (a, b) in enumerate(zip(ra, rb)):
        assert np.array_equal(a["k_opt"], b["k_opt"]) and a["cost"] == b["cost"], w
        assert (a["iterations"], a["evaluations"], a["status"], a["feasible"], a["error"]) == \
            (b["iterations"], b["evaluations"], b["status"], b["feasible"], b["error"]), w
        assert np.array_equal(P.constraints(w), Q.constraints(w)), w


def test_engine_choice_at_the_job_limit():
    """jobs == job_max takes the per-job engine, job_max + 1 .. the bundle engine: ARMOUR_JOB_ENGINE_JOBS=40,
    batches of 2 and 3 worlds (40 and 60 jobs) on one planner; both against the oracle"""
    with env("ARMOUR_JOB_ENGINE_JOBS", "40"):
        P = A.Planner(T=T, max_obstacles=3, max_worlds=3)
    for W, mine, other in ((2, JOB, LANE), (3, LANE, JOB)):
        worlds = [plain(s) for s in range(W)]
        with taken(P) as d:
            P.reach(worlds)
            for w in range(W):
                R = oracle(w)[0]
                np.testing.assert_allclose(P.torque_radius(w), R.torque_radius(), rtol=0, atol=TOL)
                np.testing.assert_allclose(P.link_generators(w), R.link_gens(), rtol=0, atol=TOL)
            res, _ = P.plan(worlds)
        assert_paths(d, not_ran=other + ("reach_retry",), exactly={mine: 2})
        for w, r in enumerate(res):
            ro = oracle(w)[1]
            assert (r["feasible"], r["status"], r["iterations"], r["error"]) == (ro["feasible"], ro["status"], ro["iterations"], 0), w
            np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=1e-8)
    P.close()


def test_row_pass_form_on_both_sides_of_four_blocks_per_cu():
    """ipm_rows_DA_lds runs where nblk * nrun >= 4 * CUs. The small boundary set at ARMOUR_ROW_CHUNK=256:
    1015 rows, 4 blocks per world, so the bound is one world per CU. With as many worlds as the device has
    CUs the iterations in which every world still runs take the LDS form (the second one at least: no
    world finishes in its first); with one world fewer none does. Both bitwise ARMOUR_DA_REGS' plans."""
    ncu = A.lib().armour_device_compute_units(0)
    assert ncu > 12
    fx = load("boundary_small_T20_O6")
    O = fx["obstacles"].shape[1]
    base = [world(fx, w) for w in range(len(fx["kinds"]))]
    with env("ARMOUR_ROW_CHUNK", "256"):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=ncu)
        with env("ARMOUR_DA_REGS", "1"):
            Q = A.Planner(T=T, max_obstacles=O, max_worlds=ncu)
    assert P.num_constraints(O) + 7 == 1015 and -(-1015 // 256) == 4
    for W in (ncu, ncu - 1):
        worlds = [base[w % len(base)] for w in range(W)]
        with taken(P) as dp, taken(Q) as dq:
            (ra, _), (rb, _) = P.plan(worlds), Q.plan(worlds)
        assert min(r["iterations"] for r in ra) >= 1
        if W == ncu:
            assert_paths(dp, ran=("da_lds", "da_regs"))
        else:
            assert_paths(dp, ran=("da_regs",), not_ran=("da_lds",))
        assert_paths(dq, ran=("da_regs",), not_ran=("da_lds",))
        assert dp["da_lds"] + dp["da_regs"] == dq["da_regs"], (dp, dq)  # the same iterations, one launch each
        assert_bitwise(P, Q, ra, rb)
    P.close()
    Q.close()


def test_sync_free_tail_at_its_world_limit():
    """nrun == tail_worlds runs sync-free, tail_worlds + 1 synchronised: ARMOUR_TAIL_WORLDS=4 with 4 and
    5 worlds, none of which restarts (so a loop's only forced synchronised iteration is its first). With 4
    every later iteration is in the tail; with 5 the second one at least is synchronised, and the tail
    starts once a world has converged. Both bitwise ARMOUR_TAIL_WORLDS=0's plans."""
    with env("ARMOUR_TAIL_WORLDS", "4"):
        P = A.Planner(T=T, max_obstacles=3, max_worlds=5)
    with env("ARMOUR_TAIL_WORLDS", "0"):
        Q = A.Planner(T=T, max_obstacles=3, max_worlds=5)
    for W in (4, 5):
        worlds = [plain(s) for s in range(W)]
        with taken(P) as dp, taken(Q) as dq:
            (ra, _), (rb, _) = P.plan(worlds), Q.plan(worlds)
        assert min(r["iterations"] for r in ra) >= 3 and len({r["iterations"] for r in ra}) > 1
        assert_paths(dp, ran=("ipm_iter_tail",), exactly={"ipm_restarts": 0})
        assert (dp["ipm_iter_sync"] == 1) if W == 4 else (dp["ipm_iter_sync"] >= 2), dp
        assert_paths(dq, ran=("ipm_iter_sync",), not_ran=("ipm_iter_tail", "ls_one_round"))
        assert dp["ipm_iter_sync"] + dp["ipm_iter_tail"] >= dq["ipm_iter_sync"], (dp, dq)  # (the tail may run one idle iteration)
        assert_bitwise(P, Q, ra, rb)
        for w, r in enumerate(ra):
            assert r["iterations"] == oracle(w)[1]["iterations"], w
    P.close()
    Q.close()


@pytest.mark.parametrize("max_iter", [3, 1])
def test_iteration_cap(max_iter):
    """armour_config.max_iter against OraclePlanner.plan(max_iter=...): every one of the six worlds needs
    6 to 9 iterations, so each stops at the cap with status 1 and exactly max_iter iterations"""
    seeds = range(6)
    P = A.Planner(T=T, max_obstacles=3, max_worlds=len(seeds), max_iter=max_iter)
    res, _ = P.plan([plain(s) for s in seeds])
    capped = 0
    for s, r in zip(seeds, res):
        ro, free = oracle(s, max_iter)[1], oracle(s)[1]
        assert (r["status"], r["feasible"], r["iterations"], r["error"]) == (ro["status"], ro["feasible"], ro["iterations"], 0), s
        np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=1e-8)
        if free["iterations"] > max_iter:
            capped += 1
            assert (r["status"], r["iterations"]) == (1, max_iter), (s, r)
    assert capped >= 2
    assert_paths(P.path_counts(), ran=("ipm_iter_sync",))
    c = P.path_counts()
    assert c["ipm_iter_sync"] + c["ipm_iter_tail"] <= max_iter + 2, c  # no launches far past the cap
    P.close()


def test_nine_joints_forty_obstacles_take_the_full_capacity_kernels():
    """360 (link, obstacle) pairs: the pair tables do not fit the small evaluation kernels' buffers although
    the reach sets do (planner.hip launch_eval, launch_trials), so every evaluation and trial launch is a
    full-capacity one; values against the oracle, plans by tests/test_gpu_boundary.py's rules"""
    robot = RV.variant("KINOVA_9")
    O, seeds = 40, (80, 81)
    worlds = [A.make_world(s, O, robot=RT.geometry(robot)) for s in seeds]
    P = A.Planner(T=T, max_obstacles=O, max_worlds=len(worlds), robot=robot)
    P.reach(worlds)
    occ = P.occupancy()
    assert occ["link_monomials"][0] <= 16 and occ["torque_monomials"][0] <= 64 and P.NJ * O == 360
    refs = []
    x = np.linspace(-0.6, 0.6, 7)
    for w, wd in enumerate(worlds):
        R = OraclePlanner(*wd, T=T, threads=8, robot=RT.to_struct(robot))
        R.reach()
        refs.append(R)
        g, J = P.eval_constraints(w, x)
        go, Jo = R.eval(x)
        np.testing.assert_allclose(g, go, rtol=0, atol=TOL)
        np.testing.assert_allclose(J, Jo, rtol=0, atol=TOL)
    res, _ = P.plan(worlds)
    for w, (r, R) in enumerate(zip(res, refs)):
        ro = R.plan()
        assert (r["feasible"], r["status"], r["error"]) == (ro["feasible"], ro["status"], 0), w
        stalled = r["status"] == 4 and not r["feasible"]
        assert abs(r["iterations"] - ro["iterations"]) <= (5 if stalled else 0), (w, r["iterations"], ro["iterations"])
        if not stalled:
            np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=1e-8 if (r["status"] == 0 or r["feasible"]) else 1e-3)
    assert_paths(P.path_counts(), ran=("eval_f64", "eval_cached", LANE), not_ran=("eval_small", "trials_small", "eval_full_scan") + JOB)
    P.close()


# the default dispatch of one planner (no variable set) of T = 20, 6 obstacles, 64 worlds: the counters
# that are non-zero after each call, on a device of at least 64 CUs. A world's reach sets here hold at
# most 16 / 64 monomials, so the small-capacity kernels serve every evaluation.
SOLVE = {"pc_builds", "eval_cached", "eval_small", "solve_adaptive", "ipm_iter_sync", "ipm_iter_tail", "da_regs", "reach_sq"}
CENSUS = {
    # one world: the per-job engine's 256-thread kernel; every iteration after the first in the tail, with
    # round 0 and the speculative round (this world accepts round 0's trial: never the one-round search)
    "one world": SOLVE | {"batch_uniform", "reach_job_256", "ls_speculative", "trials_small"},
    # 64 worlds, 1280 jobs: the per-job engine (at most 5120 jobs) at 128 threads (more than 2 jobs per CU);
    # restoration phases inside the loop, on the second stream beside the tail
    "uniform": SOLVE | {"batch_uniform", "reach_job_128", "ls_one_round", "trials_all", "ls_speculative", "trials_small",
                        "resto_inline", "resto_one_round", "resto_second_stream", "resto_solver_stream", "resto_after_loop",
                        "ipm_restarts"},
    # four worlds, all in the tail: their phases start after the loop has ended (the tail learns of a failed
    # search two iterations late), on the solver stream
    "mixed": SOLVE | {"batch_mixed", "reach_job_256", "ls_one_round", "trials_all", "ls_speculative", "trials_small",
                      "resto_after_loop", "resto_one_round", "resto_solver_stream"},
    "candidates": {"cand_small", "cand_chunks"},
    "motion": {"motion_chunks"},
    "episode step": SOLVE | {"reach_job_256", "ls_one_round", "trials_all", "ls_speculative", "trials_small",
                             "resto_after_loop", "resto_one_round", "resto_solver_stream", "motion_chunks", "track_row_episode"},
}


def test_default_dispatch_census():
    fx = load("boundary_small_T20_O6")
    base = [world(fx, w) for w in range(len(fx["kinds"]))]
    O = fx["obstacles"].shape[1]
    P = A.Planner(T=T, max_obstacles=O, max_worlds=64)
    got = {}
    with taken(P) as got["one world"]:
        P.plan([base[0]])
    with taken(P) as got["uniform"]:
        res, _ = P.plan([base[w % len(base)] for w in range(64)])
    assert all(r["error"] == 0 for r in res)
    counts = [2, 0, 3, 6]
    mixed = [base[w][:4] + (base[w][4][:c],) for w, c in enumerate(counts)]
    with taken(P) as got["mixed"]:
        rm, _ = P.plan_mixed(mixed)
    with taken(P) as got["candidates"]:
        P.eval_candidates(np.random.default_rng(3).uniform(-1, 1, (len(counts), 40, 7)))
    z = np.zeros(7)
    with taken(P) as got["motion"]:
        P.check_motion(np.array([np.stack([w[0], z, z, r["k_opt"]]) for w, r in zip(mixed, rm)]), 0.0, 1.0, 5)
    goals = np.array([w[3] for w in mixed])
    P.episode_begin(mixed, goals, check_samples=6)
    P.episode_track(num_samples=2, steps=10)
    with taken(P) as got["episode step"]:
        P.episode_step()
    for k, d in got.items():
        print("census", k, {n: v for n, v in d.items() if v})
    assert got["candidates"]["cand_chunks"] == 2 and got["motion"]["motion_chunks"] == 5
    for k, d in got.items():
        nonzero = {n for n, v in d.items() if v}
        assert nonzero == CENSUS[k], (k, "unexpected", sorted(nonzero - CENSUS[k]), "missing", sorted(CENSUS[k] - nonzero))
    P.close()
