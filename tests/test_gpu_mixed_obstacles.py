"""Mixed batches on the GPU: armour_plan_batch_mixed / armour_reach_batch_mixed plan worlds that carry
different numbers of obstacles in one reach launch and one solve.

A world of a mixed batch keeps, inside slabs strided by the batch's largest count, the row layout and
the row-to-block partition it has in a uniform batch of its own count, so every sum it takes is the
same additions in the same order: its plan must be bitwise that uniform batch's plan (the bar of the
project's other A/B tests: concurrent against sequential, speculative against sequential, small
against full evaluation). Shapes: T = 10 (NJ = 7, rows R = 7 T + 7 T O + 35 per world, 1024 rows per
block), counts chosen so that the first world is not the largest, some worlds have no obstacles and
counts repeat; [13, 14] puts a one-block world (R = 1015) into a two-block grid (R = 1085)."""
import contextlib
import os

import numpy as np
import pytest

import armour_amd as A
from conftest import engine
from oracle import OraclePlanner
from paths import assert_paths, engine_paths

pytestmark = pytest.mark.gpu

T = 10
COUNTS_A = [2, 0, 3, 1, 3, 0]
FIELDS = ("feasible", "status", "iterations", "evaluations", "cost", "kkt")


def worlds_of(counts, seed0):
    return [A.make_world(seed0 + s, n) for s, n in enumerate(counts)]


def plan_grouped(worlds, T=T):
    """the existing path: one uniform batch (armour_plan_batch) per obstacle count"""
    counts = [np.asarray(w[4]).reshape(-1, 12).shape[0] for w in worlds]
    out = [None] * len(worlds)
    for n in sorted(set(counts)):
        idx = [i for i, c in enumerate(counts) if c == n]
        P = A.Planner(T=T, max_obstacles=n, max_worlds=len(idx))
        res, _ = P.plan([worlds[i] for i in idx])
        for i, r in zip(idx, res):
            out[i] = r
        P.close()
    return out


def assert_bitwise(got, want, tag=""):
    assert len(got) == len(want)
    for w, (r, u) in enumerate(zip(got, want)):
        for f in FIELDS:
            assert r[f] == u[f], (tag, w, f, r[f], u[f])
        assert np.array_equal(r["k_opt"], u["k_opt"]), (tag, w, r["k_opt"], u["k_opt"])
        assert r["error"] == u["error"] == 0, (tag, w)


@pytest.fixture(scope="module")
def batch_a():
    """batch (a) planned once in a mixed call; the planner stays open for the getters"""
    worlds = worlds_of(COUNTS_A, 300)
    P = A.Planner(T=T, max_obstacles=max(COUNTS_A), max_worlds=len(worlds))
    res, tm = P.plan_mixed(worlds)
    yield worlds, P, res
    P.close()


def test_mixed_equals_uniform_batches_bitwise(batch_a):
    worlds, P, res = batch_a
    assert [P.world_obstacles(w) for w in range(len(worlds))] == COUNTS_A
    assert_bitwise(res, plan_grouped(worlds), "a")
    # only the mixed instantiations ran: every batch of this planner was a mixed one (each solver kernel is
    # then the _mx one), and no launch of the uniform full-capacity evaluation kernel
    assert_paths(P.path_counts(), ran=("batch_mixed", ("eval_small", "eval_mx"), "eval_cached"),
                 not_ran=("batch_uniform", "eval_f64", "eval_f32", "eval_armtd_f64"))


def test_idle_row_block_bitwise():
    """counts [13, 14]: the 13-obstacle world has one row block (R = 1015) in the two-block grid the
    14-obstacle world needs (R = 1085), so its second block idles and its sums take one partial"""
    counts = [13, 14]
    assert 7 * T + 7 * T * 13 + 35 <= 1024 < 7 * T + 7 * T * 14 + 35
    worlds = worlds_of(counts, 320)
    P = A.Planner(T=T, max_obstacles=14, max_worlds=2)
    res, _ = P.plan_mixed(worlds)
    assert_bitwise(res, plan_grouped(worlds), "b")
    P.close()


def test_mixed_against_oracle(batch_a):
    worlds, P, res = batch_a
    refs = []
    for w, world in enumerate(worlds):
        R = OraclePlanner(*world, T=T, threads=4)
        R.reach()
        ro = R.plan()
        refs.append(R)
        assert res[w]["feasible"] == ro["feasible"], w
        np.testing.assert_allclose(res[w]["k_opt"], ro["k_opt"], rtol=0, atol=1e-8, err_msg=str(w))
        g = P.constraints(w)
        assert g.shape == (P.num_constraints(COUNTS_A[w]),) == (7 * T + 7 * T * COUNTS_A[w] + 28,), w
        go, _ = R.eval(res[w]["k_opt"])
        np.testing.assert_allclose(g, go, rtol=0, atol=1e-9, err_msg=str(w))
    # the reach half alone, then g and J of every world at a fixed point
    P.reach_mixed(worlds)
    x = np.array([0.8, -0.55, 0.3, -0.8, 0.05, 0.62, -0.17])
    for w, R in enumerate(refs):
        g, J = P.eval_constraints(w, x)
        m = P.num_constraints(COUNTS_A[w])
        assert g.shape == (m,) and J.shape == (m, 7), w
        go, Jo = R.eval(x)
        np.testing.assert_allclose(g, go, rtol=0, atol=1e-9, err_msg=str(w))
        np.testing.assert_allclose(J, Jo, rtol=0, atol=1e-9, err_msg=str(w))


def test_mixed_without_plane_cache_bitwise(batch_a):
    worlds, _, res = batch_a
    os.environ["ARMOUR_PLANE_CACHE"] = "0"
    try:
        P = A.Planner(T=T, max_obstacles=max(COUNTS_A), max_worlds=len(worlds))
    finally:
        os.environ.pop("ARMOUR_PLANE_CACHE", None)
    with pytest.raises(A.ArmourError, match="plane cache off"):
        P.reach_mixed(worlds)
        P.plane_cache_stats()
    full, _ = P.plan_mixed(worlds)
    assert_bitwise(full, res, "d")
    # without the cache every evaluation is eval_kernel_mx on the full scan
    assert_paths(P.path_counts(), ran=("batch_mixed", "eval_mx", "eval_full_scan", "ipm_iter_sync"),
                 not_ran=("batch_uniform", "eval_f64", "eval_small", "eval_cached", "pc_builds", "ls_speculative",
                          "ls_one_round", "ipm_iter_tail"))
    P.close()


def test_plane_cache_stats_count_existing_pairs(batch_a):
    worlds, P, _ = batch_a
    P.reach_mixed(worlds)
    st = P.plane_cache_stats()
    assert st["pairs"] == T * 7 * sum(COUNTS_A)
    assert st["blocks"] == st["blocks_cached"] == T * len(worlds)
    assert 0 < st["planes_kept"] <= 36 * st["pairs"] and st["max_per_pair"] <= 36


def test_saved_worlds_in_one_mixed_call():
    """the reference's 100 saved worlds (5 to 14 obstacles) at T = 100 in one plan_mixed call on one
    planner, against the oracle's plans: the bar of test_saved_worlds_match_oracle"""
    from test_saved_worlds import saved_worlds

    names, worlds, fx = saved_worlds()
    assert len(worlds) == 100 and len(set(fx["num_obstacles"].tolist())) == 10
    P = A.Planner(T=100, max_obstacles=14, max_worlds=100)
    res, _ = P.plan_mixed(worlds)
    assert len(res) == 100
    for i, r in enumerate(res):
        assert P.world_obstacles(i) == int(fx["num_obstacles"][i]), names[i]
        assert r["feasible"] == bool(fx["feasible"][i]), names[i]
        assert r["status"] == int(fx["status"][i]), names[i]
        assert r["iterations"] == int(fx["iterations"][i]), names[i]
        np.testing.assert_allclose(r["k_opt"], fx["k_opt"][i], rtol=0, atol=1e-8, err_msg=str(names[i]))
        np.testing.assert_allclose(r["cost"], fx["cost"][i], rtol=1e-8, atol=1e-12, err_msg=str(names[i]))
    P.close()


def test_saved_worlds_mixed_bitwise_on_one_reach_kernel():
    """T = 100, where a world has 5 to 11 row blocks (R = 735 + 700 O rows): the mixed call against the
    grouped uniform calls, bitwise. Which reach kernel a batch takes depends on its size (100 worlds:
    the bundle engine; the groups of 6 to 22 worlds: the per-job engine's 128-thread kernel; those of
    at most 5: its 256-thread kernel), and the kernels' reach sets differ at rounding level (DESIGN.md
    section 3), as a uniform batch's already do between batch sizes. So both sides are held to the
    per-job engine's 128-thread kernel, whose reach sets do not depend on the batch, and the comparison
    isolates the solver's per-world row layout."""
    from test_saved_worlds import saved_worlds

    _, worlds, fx = saved_worlds()
    counts = [int(c) for c in fx["num_obstacles"]]
    assert {(735 + 700 * n + 1023) // 1024 for n in counts} == set(range(5, 12))   # row blocks per world
    with engine("narrow"):
        P = A.Planner(T=100, max_obstacles=14, max_worlds=100)
        res, _ = P.plan_mixed(worlds)
        assert_paths(P.path_counts(), ran=("batch_mixed",) + engine_paths("narrow")["ran"],
                     not_ran=("batch_uniform",) + engine_paths("narrow")["not_ran"])
        P.close()
        assert_bitwise(res, plan_grouped(worlds, T=100), "one reach kernel")


EDGE_COUNTS = (14, 0, 13, 1)
ARMS = ("default", "rounds", "after_loop", "sequential", "tail")


def arm_of(name):
    """(the setting of a loop form or None, the paths a planner created under it must show)"""
    return {
        "default": (None, dict(ran=("batch_mixed", "resto_inline"))),
        "rounds": (("ARMOUR_RESTO_ROUNDS", "1"), dict(ran=("resto_rounds", "resto_after_loop"), not_ran=("resto_inline",))),
        "after_loop": (("ARMOUR_RESTO_INLINE", "0"), dict(ran=("resto_one_round", "resto_after_loop"), not_ran=("resto_inline",))),
        "sequential": (("ARMOUR_NO_SPEC", "1"), dict(ran=("ls_sequential",), not_ran=("ls_speculative", "ls_one_round"))),
        "tail": (("ARMOUR_TAIL_WORLDS", "1000"), dict(ran=("ipm_iter_tail", ("ls_one_round", "ls_speculative")))),
    }[name]


@pytest.fixture(scope="module")
def edge_worlds():
    """the 33 worlds of domain_edges.plan_cases() (limits, speeds, far goals: 20 end in local
    infeasibility, four of the others backtrack), world i with the first (14, 0, 13, 1)[i % 4] boxes of
    make_world(3, 14) (the first three are the base world's own): two row blocks (R = 1085) for 14
    obstacles, one and an idle second block for the others. With the oracle's verdicts, computed once."""
    import domain_edges as DE

    assert DE.T == T
    boxes = np.asarray(A.make_world(3, 14)[4], dtype=np.float64).reshape(14, 12)
    assert np.array_equal(boxes[:3], np.asarray(DE.base_world()[4]).reshape(3, 12))
    worlds = [tuple(w[:4]) + (boxes[:EDGE_COUNTS[i % 4]].copy(),) for i, (_, w) in enumerate(DE.plan_cases())]
    assert len(worlds) == 33
    want = []
    for world in worlds:
        R = OraclePlanner(*world, T=T, threads=4)
        R.reach()
        ro = R.plan()
        want.append((ro["feasible"], ro["status"]))
    return worlds, want


@pytest.mark.parametrize("arm", ARMS)
def test_phases_and_backtracking_in_a_mixed_batch_bitwise(edge_worlds, arm):
    """The restoration and speculative kernels' mixed instantiations on worlds that enter a phase or
    backtrack, with idle second row blocks inside the phase launches: under each loop form, the mixed
    plan is bitwise the uniform batches' plan under the same setting, every world's verdict is the
    oracle's, and exactly 20 worlds end in local infeasibility."""
    from test_gpu_plane_cache import env

    worlds, want = edge_worlds
    setting, paths = arm_of(arm)
    with env(*setting) if setting else contextlib.nullcontext():
        P = A.Planner(T=T, max_obstacles=14, max_worlds=len(worlds))
        res, _ = P.plan_mixed(worlds)
        counts = P.path_counts()
        P.close()
        grouped = plan_grouped(worlds)
    assert_bitwise(res, grouped, arm)
    for w, (r, (feasible, status)) in enumerate(zip(res, want)):
        assert r["feasible"] == feasible and r["status"] == status, (arm, w, r["feasible"], r["status"])
    stalled = [w for w, r in enumerate(res) if r["status"] == 4]
    print(f"{arm}: locally infeasible {stalled}; evaluations - iterations "
          f"{[r['evaluations'] - r['iterations'] for r in res]}")
    assert len(stalled) == 20, stalled
    assert_paths(counts, **paths)


def test_mixed_errors_and_uniform_list():
    P = A.Planner(T=T, max_obstacles=3, max_worlds=4)
    L = A.lib()
    assert L.armour_world_num_obstacles(P.h, 0) == -4          # ARMOUR_E_STATE: no batch yet
    mixed = worlds_of([2, 4, 1], 340)                          # 4 > max_obstacles, in the middle
    arr = P._worlds(mixed)
    res = (A.Result * 3)()
    assert L.armour_plan_batch_mixed(P.h, 3, arr, res, None) == A.ARMOUR_E_ARG
    with pytest.raises(A.ArmourError, match="max_obstacles"):
        P.plan_mixed(mixed)
    ok = worlds_of([2, 0, 3], 350)
    with pytest.raises(A.ArmourError, match="same num_obstacles"):
        P.plan(ok)                                             # armour_plan_batch keeps its rule
    P.plan_mixed(ok)
    assert L.armour_world_num_obstacles(P.h, 2) == 3
    assert L.armour_world_num_obstacles(P.h, 3) == A.ARMOUR_E_ARG
    # a uniform list through the mixed entry: bitwise armour_plan_batch
    uni = worlds_of([3, 3, 3, 3], 360)
    a, _ = P.plan_mixed(uni)
    b, _ = P.plan(uni)
    assert_bitwise(a, b, "f")
    assert P.constraints(1).shape == (P.num_constraints(3),)
    P.close()
