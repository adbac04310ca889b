"""The small-capacity evaluation kernels (eval_kernel_small, eval_trials_small: LDS sized for the
batch's largest PZs, five blocks per CU) against the full-capacity ones
(ARMOUR_EVAL_FULL=1): constraint values, Jacobians and whole plans bitwise equal, on survey worlds
and on the config 3 decision-boundary fixture (280 pairs, the largest the small kernels take)."""
import numpy as np
import pytest

import armour_amd as A
from conftest import engine
from paths import assert_paths, engine_paths, taken
from test_boundary import load, world
from test_gpu_plane_cache import check_eval, check_plan, env

pytestmark = pytest.mark.gpu


def planners(T, O, W, eng=None):
    with engine(eng):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
        with env("ARMOUR_EVAL_FULL", "1"):
            Q = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    return P, Q


def check_both(P, Q, worlds, rng, n, eng=None):
    """check_eval and check_plan, and the census: the default planner evaluated on the small kernels
    wherever it read the plane cache (a point outside the certified box takes the full-capacity
    full scan on both), the ARMOUR_EVAL_FULL planner never"""
    with taken(P) as dp, taken(Q) as dq:
        check_eval(P, Q, worlds, rng, n=n)
    assert_paths(dp, ran=("eval_small", "eval_full_scan") + engine_paths(eng)["ran"], not_ran=engine_paths(eng)["not_ran"])
    assert dp["eval_small"] == dp["eval_cached"] and dp["eval_f64"] == dp["eval_full_scan"], dp
    assert_paths(dq, ran=("eval_f64", "eval_cached"), not_ran=("eval_small",))
    with taken(P) as dp, taken(Q) as dq:
        check_plan(P, Q, worlds)
    assert_paths(dp, ran=("eval_small", "trials_small"), not_ran=("eval_f64", "trials_full", "eval_full_scan"))
    assert_paths(dq, ran=("eval_f64", "trials_full"), not_ran=("eval_small", "trials_small", "eval_full_scan"))


def test_eval_small_survey_worlds():
    T, O, W = 100, 20, 40
    worlds = [A.make_world(3000 + s, O, profile="survey") for s in range(W)]
    P, Q = planners(T, O, W, "lane")  # the bundle engine records the PZ sizes
    check_both(P, Q, worlds, np.random.default_rng(5), 2, "lane")
    occ = P.occupancy()
    assert occ["link_monomials"][0] <= 16 and occ["torque_monomials"][0] <= 64  # the small kernels ran


def test_eval_small_boundary_config3():
    fx = load("boundary_config3_T200_O40")
    T, W, O = int(fx["T"]), len(fx["kinds"]), fx["obstacles"].shape[1]
    worlds = [world(fx, w) for w in range(W)]
    P, Q = planners(T, O, W)
    check_both(P, Q, worlds, np.random.default_rng(9), 3)
