"""HIP path on the degenerate quadratic of the extremum roots (tests/degenerate_roots.py; fixture
tests/golden/degenerate_roots.npz): start states with qdd0 D = -6 qd0 (1 + delta) and parameters with
12 k_range x = (6 T qd0 + T^2 qdd0) (1 + delta), delta from 0 to 1e-3, where (p +- disc) / den loses its
denominator. The oracle shares the formula, so the device is held to exact values, not to the oracle:

  * the device build of jrs_joint encloses the exact trajectory at its critical times (the inequality and
    slack of tests/jrs_unit.py) and agrees with the host build's 13 doubles to 1e-12 * max(1, |q0|);
  * the extremum rows of g and J after reach() / eval_constraints, after reach_mixed() (the _mx kernels)
    and, as the class maximum, from eval_candidates (cand_rows), within 16 * 2^-52 * S and 1e-9 of the
    fixture, on every reach engine (the small-capacity kernels) and with ARMOUR_EVAL_FULL=1 (the
    full-capacity ones);
  * a world with every joint on the start-state surface: the point models inside its sets at k_opt and
    at x = 0 (tests/test_gpu_containment.py);
  * the row-case worlds planned (eval_trials_body runs only inside a solve): status, feasibility,
    iterations and k_opt against a fresh oracle at the bars of tests/test_gpu_domain_edges.py.
"""
import os

import numpy as np
import pytest

import armour_amd as A
import degenerate_roots as DR
import jrs_unit as U
from conftest import engine
from oracle import OraclePlanner
from paths import assert_paths, engine_paths, taken
from test_oracle_containment import SLACK, containment, kinova

pytestmark = pytest.mark.gpu
T, O = DR.T, DR.O
ENGINES = ["lane", "job", "narrow"]
CAND = {"cand_small", "cand_full"}
EVAL = {"eval_small", "eval_f64", "eval_mx"}


@pytest.fixture(scope="module")
def device_outputs():
    return DR.start_outputs(U.Lib(device=True))


def test_device_jrs_scalars_enclose_the_trajectory_on_the_surface(device_outputs):
    DR.check_start_enclosure(device_outputs, print)


def test_device_jrs_scalars_match_the_host_build_on_the_surface(device_outputs):
    host = DR.start_outputs(U.Lib(device=False))
    tol = 1e-12 * np.maximum(1.0, np.abs(DR.fixture()["start_cases"][:, 0]))
    d = np.abs(device_outputs - host)
    print(f"device against host: worst |difference| {d.max():.3e}, in units of the tolerance {(d / tol[:, None]).max():.3e}")
    assert np.all(d <= tol[:, None]), np.argwhere(~(d <= tol[:, None]))[:5]


def _rows_arm(P, tag, worlds, X, index, jac=True):
    misses, wv, wu, wj = [], 0.0, 0.0, 0.0
    for w in range(len(worlds)):
        g, J = P.eval_constraints(w, X[w])
        v, u, j, bad = DR.check_rows(g, J, index[w])
        wv, wu, wj = max(wv, v), max(wu, u), max(wj, j)
        misses += bad
    print(f"{tag}: worst |row - exact| {wv:.3e} ({wu:.3g} of its bar), worst Jacobian error {wj:.3e}")
    assert not misses, (tag, len(misses), sorted({b[1] for b in misses}), misses[:8])


def _three_arms(P, tag, reach_paths, eval_uniform, eval_mixed, cand):
    """the row cases through reach() + eval_constraints, eval_candidates and reach_mixed() +
    eval_constraints on planner P, each arm asserting the paths it took"""
    worlds, X, index = DR.row_worlds()
    W = len(worlds)
    # a uniform batch
    with taken(P) as d:
        P.reach(worlds)
        _rows_arm(P, f"{tag} uniform", worlds, X, index)
    assert_paths(d, ran=reach_paths["ran"] + ("batch_uniform", eval_uniform),
                 not_ran=tuple(reach_paths["not_ran"]) + ("batch_mixed", "eval_mx") + tuple(EVAL - {eval_uniform}))
    # candidates: the largest excess of the extremum rows over the joint bounds
    with taken(P) as d:
        out = P.eval_candidates(X[:, None, :])
    bounds = P.joint_bounds()
    worst = 0.0
    for w in range(W):
        want, tol = DR.rows_violation(index[w], bounds)
        got = out["violation"][w, 0, 2]
        worst = max(worst, abs(got - want) / tol)
        assert abs(got - want) <= tol, (tag, w, got, want, tol)
    print(f"{tag} candidates: worst |class maximum - exact| {worst:.3g} of its bar")
    assert_paths(d, ran=(cand,), not_ran=tuple(CAND - {cand}), exactly={"cand_chunks": 1})
    # the same worlds through the mixed entry: the _mx instantiations
    with taken(P) as d:
        P.reach_mixed(worlds)
        _rows_arm(P, f"{tag} mixed", worlds, X, index)
    assert_paths(d, ran=reach_paths["ran"] + ("batch_mixed", eval_mixed),
                 not_ran=tuple(reach_paths["not_ran"]) + ("batch_uniform",) + tuple(EVAL - {eval_mixed}))


@pytest.mark.parametrize("eng", ENGINES)
def test_device_extremum_rows_on_the_surface(eng):
    with engine(eng):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=len(DR.row_worlds()[0]))
    _three_arms(P, eng, engine_paths(eng), "eval_small", "eval_small", "cand_small")


def test_device_extremum_rows_full_capacity_kernels():
    """the same through eval_kernel_t, eval_kernel_mx and cand_rows, which a T = 10 batch does not reach
    by itself"""
    prev = os.environ.get("ARMOUR_EVAL_FULL")
    os.environ["ARMOUR_EVAL_FULL"] = "1"
    try:
        P = A.Planner(T=T, max_obstacles=O, max_worlds=len(DR.row_worlds()[0]))
    finally:
        os.environ.pop("ARMOUR_EVAL_FULL") if prev is None else os.environ.update(ARMOUR_EVAL_FULL=prev)
    _three_arms(P, "full", engine_paths(None), "eval_f64", "eval_mx", "cand_full")


@pytest.mark.parametrize("eng", ENGINES)
def test_surface_world_sets_contain_the_point_models(eng):
    """every joint starts with qdd0 D = -6 qd0: the critical times 1/4 and 3/4 of q and qdd lie inside
    intervals 2 and 7 of T = 10, where jrs_joint's k-independent bounds lost them"""
    world = DR.surface_world()
    with engine(eng):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=1)
    res, _ = P.plan([world])
    robot, rng = kinova(), np.random.default_rng(31)
    for tag, x in (("k_opt", res[0]["k_opt"]), ("x = 0", np.zeros(7))):
        g = P.eval_constraints(0, x, jac=False)
        lw, tw, _ = containment(robot, world, T, x, P.link_centers(0), P.link_generators(0), g[:7 * T].reshape(T, 7),
                                P.torque_radius(0), rng, n_t=8)
        print(f"{eng} {tag}: worst link excess {lw:.3e} m, worst torque excess {tw:.3e} N m")
        assert lw <= SLACK, f"{tag}: a link point lies {lw:.3e} m outside its set"
        assert tw <= SLACK, f"{tag}: a torque lies {tw:.3e} N m outside centre +- radius"
    assert_paths(P.path_counts(), **engine_paths(eng))


def test_row_case_worlds_plan_as_the_oracle():
    """the solver on the row-case worlds: its trial points evaluate the extremum rows through
    eval_trials_body. A world that ends in local infeasibility (status 4) follows the rule of
    tests/test_gpu_boundary.py: the iteration count within 5, k_opt not compared."""
    worlds, _, _ = DR.row_worlds()
    P = A.Planner(T=T, max_obstacles=O, max_worlds=len(worlds))
    res, _ = P.plan(worlds)
    for w, world in enumerate(worlds):
        R = OraclePlanner(*world, T=T, threads=4)
        R.reach()
        r, ro = res[w], R.plan()
        dk = np.abs(r["k_opt"] - ro["k_opt"]).max()
        print(f"world {w}: feasible={r['feasible']} status={r['status']} iterations={r['iterations']} "
              f"(oracle {ro['iterations']}) |dk_opt|={dk:.1e}")
        assert r["error"] == 0, w
        assert r["feasible"] == ro["feasible"] and r["status"] == ro["status"], (w, r["status"], ro["status"])
        if r["status"] == 4:
            assert abs(r["iterations"] - ro["iterations"]) <= 5, (w, r["iterations"], ro["iterations"])
        else:
            assert r["iterations"] == ro["iterations"], (w, r["iterations"], ro["iterations"])
            assert dk <= 1e-8, (w, dk)
    assert_paths(P.path_counts(), ran=(("trials_small", "trials_full", "trials_all"),))
