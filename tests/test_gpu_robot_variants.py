"""The HIP path on the robot variants of tests/robot_variants.py: reversed joint axes, nine joints,
fixed frames with a generic roll / pitch / yaw.

Shapes: T = 20, O = 4, W = 3. Kinova-derived variants run on both reach engines and the per-job
engine's two widths ("lane", "job", "narrow" of conftest.engine) where their program fits the per-job
engine's payload pool, and must be refused there with ARMOUR_E_CAPACITY where it does not (9 joints:
1208 doubles of 1024); Fetch-derived variants run on the engine the planner picks (the bundle engine:
their program does not fit either).

  * containment (test_gpu_containment._check): the sets enclose the point models, at SLACK;
  * the mirror identity (robot_variants.mirror_rows), which needs no reference: robot B =
    reversed_robot(A, S) at the mirrored state is robot A. Every evaluation line within TOL = 1e-9
    (measured on the oracle at these seeds: 4e-15), collision decisions identical; plans at the bar
    of test_rerun_bitwise_and_batch_position_stable; candidates at test_gpu_candidates' tolerance.
    Seeds: robot_variants.MIRROR_CASES, chosen on the oracle alone (its comment says why most seeds
    cannot serve, and why Fetch has no infeasible world among them);
  * oracle parity (test_gpu_parity._compare_batch) on the four variants;
  * nine joints through the solver's other paths: constraint count, mixed batches, candidates,
    the plane cache on and off and its pair count.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import armour_amd as A
import robot_variants as RV
from armour_amd import robot_tables as RT
from conftest import engine
from oracle import OraclePlanner
from paths import assert_paths, engine_paths
from test_gpu_candidates import candidates, check_against_oracle, oracle_candidates
from test_gpu_containment import _check
from test_gpu_mixed_obstacles import assert_bitwise
from test_gpu_parity import ENGINES, TOL, _compare_batch
from test_gpu_plane_cache import assert_cache_paths, check_eval, check_plan, env

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import emu  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T, O, W = 20, 4, 3
KINOVA_DERIVED = ("KINOVA_REV", "KINOVA_9")
# (variant, engine): every engine for the Kinova-derived ones, the planner's choice for Fetch's
CASES = [(n, e) for n in KINOVA_DERIVED for e in ENGINES] + [("FETCH_REV", None), ("FETCH_9_REV", None)]
IDS = [f"{n}-{e or 'default'}" for n, e in CASES]


def fits_per_job_engine(robot):
    return emu.program_size(RT.to_struct(robot))[1] <= emu.POOL_DOUBLES


def planner(robot, eng=None, max_obstacles=O, max_worlds=W):
    """a planner of the robot tables (None: the built-in Kinova) on reach engine `eng`"""
    with engine(eng):
        return A.Planner(T=T, max_obstacles=max_obstacles, max_worlds=max_worlds, robot=robot)


def refused(robot, eng):
    """True after asserting the documented refusal: a program that does not fit the per-job engine's
    payload pool, where ARMOUR_ENGINE=job forces that engine"""
    if eng not in ("job", "narrow") or fits_per_job_engine(robot):
        return False
    with pytest.raises(A.ArmourError, match=r"payload doubles \(per-job engine: 1024\)"):
        planner(robot, eng)
    with engine(eng):
        cfg = A.Config(0, T, O, W, 0, 0)
        rs = RT.to_struct(robot)
        assert not A.lib().armour_create_robot(ctypes.byref(cfg), ctypes.byref(rs))
    return True


def worlds_of(robot, seeds, profile="default", counts=None):
    geo = RT.geometry(robot) if robot is not None else A.KINOVA
    return [A.make_world(s, O if counts is None else counts[i], robot=geo, profile=profile) for i, s in enumerate(seeds)]


def test_reach_program_unchanged_for_kinova_and_fetch():
    """armour_get_reach_program: the op codes recorded before reversed axes were honoured"""
    with open(os.path.join(GOLD, "reach_program_parent.json")) as f:
        want = json.load(f)
    for name, robot in (("kinova", None), ("fetch", RV.fetch())):
        P = planner(robot)
        assert np.array_equal(P.reach_program(), np.array(want[name])[:, 0]), name
        assert_paths(P.path_counts(), not_ran=tuple(P.path_counts()))  # reading the program launches nothing
        P.close()
    P = planner(RV.variant("KINOVA_REV"))
    assert np.array_equal(P.reach_program(), np.array(want["kinova"])[:, 0])
    P.close()


@pytest.mark.parametrize("name,eng", CASES, ids=IDS)
def test_sets_contain_point_models(name, eng):
    robot = RV.variant(name)
    if refused(robot, eng):
        return
    P = planner(robot, eng)
    n, worst = _check(P, worlds_of(robot, (40, 41, 42), profile="survey"), robot, np.random.default_rng(4))
    print(f"{name} {eng}: {n} time samples, worst excess {worst}")
    # (Fetch's programs and the nine-joint ones fit the bundle engine only: planner.hip job_fits)
    assert_paths(P.path_counts(), **engine_paths(eng if fits_per_job_engine(robot) else "lane"))
    P.close()


@pytest.mark.parametrize("name,eng", CASES, ids=IDS)
def test_oracle_parity(name, eng):
    robot = RV.variant(name)
    if refused(robot, eng):
        return
    _compare_batch(T, O, [70, 71, 72], [np.zeros(7), np.linspace(-0.6, 0.6, 7)], robot=robot, eng=eng)


# ---- the mirror identity -------------------------------------------------------------------------
MIRROR = [("kinova", e) for e in ENGINES] + [("fetch", None), ("kinova9", None)]


def _gpu_eval(P, w, x):
    g, J = P.eval_constraints(w, x)
    return dict(centers=P.link_centers(w), gens=P.link_generators(w), radius=P.torque_radius(w), g=g, J=J)


@pytest.mark.parametrize("case,eng", MIRROR, ids=[f"{c}-{e or 'default'}" for c, e in MIRROR])
def test_mirror_identity(case, eng):
    """B = reversed_robot(A, S) at mirror_world(world, S) and x_B = sigma x_A against A at world, x_A.
    Oracle alone at these seeds (test_robot_variants.test_mirror_identity_on_the_oracle): evaluation
    lines within 4e-15, k_opt within 5e-10; the GPU is held to TOL = 1e-9 and 1e-8."""
    build, joints, seeds = RV.MIRROR_CASES[case]
    Ar = build()
    Br = RV.reversed_robot(Ar, joints)
    s = RV.sigma(joints)
    NJ = int(Ar["num_joints"])
    wA = worlds_of(Ar, seeds)
    wB = [RV.mirror_world(w, joints) for w in wA]
    PA = planner(None if case == "kinova" else Ar, eng)   # A = the built-in Kinova, not its tables handed back
    PB = planner(Br, eng)
    assert PA.NJ == PB.NJ == NJ
    PA.reach(wA)
    PB.reach(wB)
    for x in RV.MIRROR_X:
        for w in range(W):
            d = RV.mirror_eval_diffs(_gpu_eval(PA, w, x), _gpu_eval(PB, w, s * x), T, NJ, O, joints)
            print(case, eng, seeds[w], {k: f"{v:.1e}" for k, v in d.items()})
            assert max(d.values()) <= TOL, (case, seeds[w], d)
    # candidates: the same points mirrored
    X = np.stack([candidates(w, 16) for w in range(W)])
    ca, cb = PA.eval_candidates(X), PB.eval_candidates(X * s)
    np.testing.assert_array_equal(ca["feasible"], cb["feasible"])
    np.testing.assert_array_equal(ca["best"], cb["best"])
    np.testing.assert_allclose(cb["cost"], ca["cost"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(cb["violation"], ca["violation"], rtol=0, atol=1e-9)
    ra, _ = PA.plan(wA)
    rb, _ = PB.plan(wB)
    for w in range(W):
        print(case, eng, seeds[w], ra[w]["feasible"], ra[w]["status"], ra[w]["iterations"],
              np.abs(rb[w]["k_opt"] - s * ra[w]["k_opt"]).max())
        RV.assert_mirror_plan(ra[w], rb[w], joints, (case, seeds[w]))
        assert ra[w]["status"] == 0 or not ra[w]["feasible"]
    assert tuple(r["feasible"] for r in ra) == RV.MIRROR_FEASIBLE[case]
    for P in (PA, PB):
        assert_paths(P.path_counts(), **engine_paths(eng if fits_per_job_engine(Ar) else "lane"))
    PA.close()
    PB.close()


# ---- nine joints through the solver's other paths ------------------------------------------------
NINE = ("KINOVA_9", "FETCH_9_REV")


@pytest.mark.parametrize("name", NINE)
def test_nine_joints_constraint_count_and_plane_cache(name):
    robot = RV.variant(name)
    worlds = worlds_of(robot, (80, 81, 82))
    P = planner(robot)
    with env("ARMOUR_PLANE_CACHE", "0"):
        Q = planner(robot)
    assert P.NJ == Q.NJ == 9
    assert P.num_constraints(O) == 7 * T + 9 * T * O + 28
    check_eval(P, Q, worlds, np.random.default_rng(9), n=3)
    st = P.plane_cache_stats()
    assert st["pairs"] == W * T * 9 * O
    assert st["blocks_cached"] == st["blocks"] and 1 <= st["max_per_pair"] <= 36
    check_plan(P, Q, worlds)
    assert P.constraints(0).shape == (7 * T + 9 * T * O + 28,)
    assert_cache_paths(P, Q, "lane")  # (nine joints: the bundle engine at every batch size)
    P.close()
    Q.close()


@pytest.mark.parametrize("name", NINE)
def test_nine_joints_mixed_batch_bitwise(name):
    """plan_mixed with counts [2, 0, 3] against uniform batches (armour_plan_batch) of each count,
    bitwise. A nine-joint program runs on the bundle engine only, whose reach sets depend at rounding
    level on the other jobs of a world's bundle (test_rerun_bitwise_and_batch_position_stable), and
    the per-job engine, which test_saved_worlds_mixed_bitwise_on_one_reach_kernel uses to hold the
    reach sets fixed, refuses these robots. With the uniform batch of count c cut down to the worlds
    that carry c obstacles, world 0's plan differed from the mixed call's in the last digits (kkt
    6.769358252984442e-05 against 6.769358252962238e-05). So every uniform batch here carries the
    three worlds' states in the mixed call's order (reach sets do not depend on obstacles, so the
    reach launches are the same jobs in the same bundles), each world with c obstacles of its own
    generator, and the plans of the worlds whose count is c are compared: the solver's per-world row
    layout is what differs between the two calls."""
    robot = RV.variant(name)
    counts = [2, 0, 3]
    seeds = (90, 91, 92)
    worlds = worlds_of(robot, seeds, counts=counts)
    P = planner(robot, max_obstacles=3)
    res, _ = P.plan_mixed(worlds)
    assert [P.world_obstacles(w) for w in range(W)] == counts
    assert [P.constraints(w).shape[0] for w in range(W)] == [7 * T + 9 * T * c + 28 for c in counts]
    assert_paths(P.path_counts(), ran=("batch_mixed", ("eval_small", "eval_mx")) + engine_paths("lane")["ran"],
                 not_ran=("batch_uniform", "eval_f64") + engine_paths("lane")["not_ran"])
    P.close()
    want = [None] * W
    for c in sorted(set(counts)):
        uniform = worlds_of(robot, seeds, counts=[c] * W)
        U = planner(robot, max_obstacles=c)
        out, _ = U.plan(uniform)
        for i, k in enumerate(counts):
            if k == c:
                assert all(np.array_equal(a, b) for a, b in zip(uniform[i], worlds[i]))
                want[i] = out[i]
        assert_paths(U.path_counts(), ran=("batch_uniform",) + engine_paths("lane")["ran"],
                     not_ran=("batch_mixed", "eval_mx") + engine_paths("lane")["not_ran"])
        U.close()
    assert_bitwise(res, want, name)


@pytest.mark.parametrize("name", NINE)
def test_nine_joints_candidates(name):
    """as test_gpu_candidates.test_fetch_links for 8 joints: every candidate against the oracle's g"""
    robot = RV.variant(name)
    worlds = worlds_of(robot, (100, 101))
    N = 8
    X = np.stack([candidates(w, N) for w in range(2)])
    P = planner(robot, max_worlds=2)
    P.reach(worlds)
    out = P.eval_candidates(X)
    for w in range(2):
        R = OraclePlanner(*worlds[w], T=T, threads=8, robot=RT.to_struct(robot))
        R.reach()
        check_against_oracle(out, w, oracle_candidates(R, X[w]), name)
    assert_paths(P.path_counts(), ran=(("cand_small", "cand_full"), "pc_builds") + engine_paths("lane")["ran"],
                 not_ran=engine_paths("lane")["not_ran"], exactly={"cand_chunks": 1})
    P.close()
