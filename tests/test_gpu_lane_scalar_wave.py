"""The bundle engine with its wave index held in a scalar register (lane_kernel.hip), on bundles that
are nearly empty: with one or two live lanes every keep mask of a compacting round has at most two
bits, most groups of a round vanish, and the slots, prefix masks and rmask addresses a wave derives from its
index decide where the few kept rows land.

Survey worlds with O = 2, ARMOUR_ENGINE=lane, both kernel shapes. The planner's constructor takes
even T only (num_time_steps, KPR/Parameters.h:16: T = 1 and T = 65 are rejected), so a world has an
even number of jobs and a bundle cannot hold one live lane alone; the cases are the nearest ones it
accepts, T = 2 (the smallest) and T = 66, with two live lanes where one was meant:
  t2     1 world,  T = 2:  one bundle with two live lanes
  t66    1 world,  T = 66: two bundles, the second with two live lanes
  t66x2  2 worlds, T = 66: 132 jobs in three bundles, the second holding jobs of both worlds, the
                           third with four live lanes

Every case against OraclePlanner at the same T (torque radii, link generators, constraints and
Jacobian at the three points of lane_onepass_cases.XS; 1e-9 absolute, test_gpu_parity.py's bound),
and the two shapes against each other bit for bit."""
import numpy as np
import pytest

import armour_amd as A
import lane_onepass_cases as C
from oracle import OraclePlanner
from paths import assert_paths

pytestmark = pytest.mark.gpu
TOL = 1e-9  # test_gpu_parity.TOL
O = 2
CASES = {"t2": (1, 2), "t66": (1, 66), "t66x2": (2, 66)}  # worlds, T
SEED = 5300

_gpu, _ref, _paths = {}, {}, {}


def worlds_of(case):
    return [A.make_world(SEED + s, O, profile="survey") for s in range(CASES[case][0])]


def gpu(case, shape):
    """one run per (case, shape), shared by the tests below and left unchanged"""
    if (case, shape) not in _gpu:
        T = CASES[case][1]
        worlds = worlds_of(case)
        with C.env(ARMOUR_ENGINE="lane", ARMOUR_LANE_SHAPE=shape):
            P = A.Planner(T=T, max_obstacles=O, max_worlds=len(worlds))
        P.reach(worlds)
        out = []
        for w in range(len(worlds)):
            rec = {"torque_radius": P.torque_radius(w), "link_generators": P.link_generators(w)}
            for k, x in enumerate(C.XS):
                rec[f"g_x{k}"], rec[f"J_x{k}"] = P.eval_constraints(w, x)
            out.append({k: np.array(v) for k, v in rec.items()})
        _paths[case, shape] = P.path_counts()
        P.close()
        _gpu[case, shape] = out
    other = "dense" if shape == "wide" else "wide"
    assert_paths(_paths[case, shape], ran=("reach_lane_" + shape,), not_ran=("reach_lane_" + other, "reach_job_256", "reach_job_128"))
    return _gpu[case, shape]


def ref(case):
    """the oracle's values of the same items, once per case"""
    if case not in _ref:
        out = []
        for world in worlds_of(case):
            R = OraclePlanner(*world, T=CASES[case][1], threads=4)
            R.reach()
            rec = {"torque_radius": R.torque_radius(), "link_generators": R.link_gens()}
            for k, x in enumerate(C.XS):
                rec[f"g_x{k}"], rec[f"J_x{k}"] = R.eval(x)
            out.append({k: np.array(v) for k, v in rec.items()})
        _ref[case] = out
    return _ref[case]


@pytest.mark.parametrize("shape", C.SHAPES)
@pytest.mark.parametrize("case", list(CASES))
def test_against_oracle(case, shape):
    got, want = gpu(case, shape), ref(case)
    assert len(got) == len(want) == CASES[case][0]
    for w, (g, r) in enumerate(zip(got, want)):
        for k in r:
            assert g[k].shape == r[k].shape, (w, k)
            np.testing.assert_allclose(g[k], r[k], rtol=0, atol=TOL, err_msg=f"world {w} {k}")


@pytest.mark.parametrize("case", list(CASES))
def test_shapes_agree_bitwise(case):
    wide, dense = gpu(case, "wide"), gpu(case, "dense")
    for w, (a, b) in enumerate(zip(wide, dense)):
        for k in a:
            np.testing.assert_array_equal(a[k], b[k], err_msg=f"world {w} {k}")
