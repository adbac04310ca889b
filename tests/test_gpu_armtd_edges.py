"""The ARMTD comparison planner on the GPU (jrs_armtd_kernel, the fk-only reach program, the ARMTD
instantiations of the evaluation kernel, armtd_extrema_cost, armtd_main) on the edge worlds of
tests/armtd_edges.py and on crafted radius-free tables: against a fresh oracle at the bar of
tests/test_gpu_armtd.py, and against tests/armtd_model.py with the very functions the oracle is held to in
tests/test_armtd_model.py. T = 100 (the offline tables fix it), O <= 3, W <= 12, both reach engines.
A batch of W worlds is 100 W jobs in bundles of 64: W = 1 is two bundles with 36 live lanes in the second,
W = 3 five with 44 in the last."""
import os
import subprocess

import numpy as np
import pytest

import armour_amd as A
import armtd_edges as E
import armtd_model as M
import boundary_worlds as B
from armour_amd import robot_tables as RT
from conftest import engine
from oracle import OracleArmtd
from paths import assert_paths, engine_paths
from test_armtd_model import EDGE_NAMES, OracleEval, check_jacobians, check_shift
from test_gpu_armtd import EXE, write_armtd_in
from test_gpu_plane_cache import env
from test_oracle_containment import SLACK

pytestmark = pytest.mark.gpu
TOL = 1e-9
T = E.T
ENGINES = ["lane", "job"]
BATCH = tuple(n for n in EDGE_NAMES if n != "none")     # the twelve worlds with three obstacles: one batch
ARMOUR_EVALS = ("eval_f64", "eval_f32", "eval_small", "eval_mx")


@pytest.fixture(scope="module")
def fx():
    return E.load()


@pytest.fixture(scope="module")
def robot():
    return RT.builtin(0)


@pytest.fixture(scope="module")
def refs(fx):
    """one oracle per edge world, its plan, and its rows at the evaluation points: computed once"""
    out = {}
    for name in EDGE_NAMES:
        wd = E.by_name(fx, name)
        ev = OracleEval(wd)
        out[name] = dict(wd=wd, ev=ev, plan=ev.R.plan(), at=[(lb, x, ev.R.eval(x)) for lb, x in E.eval_points(wd)])
    return out


class DeviceEval:
    """the evaluator of tests/armtd_edges.py on world w of a planner's last batch"""

    def __init__(self, P, w):
        self.P, self.w = P, w

    def eval(self, x):
        g, J = self.P.eval_constraints(self.w, x)
        return g, J, self.P.link_centers(self.w)

    def gens(self):
        return self.P.link_generators(self.w)


def planner(eng, W, O=3):
    with engine(eng):
        return A.ArmtdPlanner(T=T, max_obstacles=O, max_worlds=W)


def assert_plan(r, ro, label):
    assert r["feasible"] == ro["feasible"] and r["status"] == ro["status"], label
    assert r["iterations"] == ro["iterations"], (label, r["iterations"], ro["iterations"])
    tol = 1e-8 if (r["status"] == 0 or r["feasible"]) else 1e-3
    np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=tol, err_msg=label)


def assert_rows(P, w, R, x, go, Jo, label):
    O = P.O
    g, J = P.eval_constraints(w, x)
    np.testing.assert_allclose(g, go, rtol=0, atol=TOL, err_msg=label)
    np.testing.assert_allclose(J, Jo, rtol=0, atol=TOL, err_msg=label)
    cs = B.collision_slice(T, 7, O, nt=0)
    np.testing.assert_array_equal(g[cs] > B.COL_THR, go[cs] > B.COL_THR, err_msg=label)
    assert R.feasible(g) == R.feasible(go), label


def armtd_only(eng=None):
    return dict(ran=("eval_armtd_f64", "batch_uniform") + engine_paths(eng)["ran"],
                not_ran=ARMOUR_EVALS + ("eval_armtd_f32",) + engine_paths(eng)["not_ran"])


# ---- parity -------------------------------------------------------------------------------------
@pytest.mark.parametrize("eng", ENGINES)
def test_edge_worlds_parity(refs, eng):
    """every edge world in one batch: link generators, g and J within 1e-9 of the oracle at x in {0, +-1,
    random, -sign(qd0), -0.999 sign(qd0), the x of t_mm = 0.5 and its neighbours}, collision decisions and
    the feasibility re-check identical, status and iterations identical, k_opt within 1e-8 (1e-3 after a
    line-search failure)"""
    worlds = [refs[n]["wd"] for n in BATCH]
    P = planner(eng, len(worlds))
    P.reach(worlds)
    for w, n in enumerate(BATCH):
        R = refs[n]["ev"].R
        np.testing.assert_allclose(P.link_generators(w), R.link_gens(), rtol=0, atol=TOL, err_msg=n)
        for lb, x, (go, Jo) in refs[n]["at"]:
            assert_rows(P, w, R, x, go, Jo, f"{n} {lb}")
    res, _ = P.plan(worlds)
    for w, n in enumerate(BATCH):
        assert_plan(res[w], refs[n]["plan"], n)
        np.testing.assert_allclose(P.constraints(w), refs[n]["ev"].R.eval(res[w]["k_opt"], jac=False), rtol=0, atol=1e-7)
        # the cost of the plan is the model's (armour_result.cost: f / COST_FUNCTION_OPTIMALITY_SCALE)
        q0, qd0, q_des, _, kr, _ = refs[n]["wd"]
        f = M.cost(q0, qd0, kr, q_des, res[w]["k_opt"], RT.builtin(0)["wrap"]) / M.COST_SCALE
        np.testing.assert_allclose(res[w]["cost"], f, rtol=1e-12, atol=1e-15, err_msg=n)
    assert [r["status"] for r in res][BATCH.index("fast")] == 4
    assert_paths(P.path_counts(), **armtd_only(eng))


# ---- the model on the device's own outputs ------------------------------------------------------
@pytest.mark.parametrize("eng", ENGINES)
def test_device_rows_against_the_model(refs, robot, eng):
    """tests/test_armtd_model.py's extremum, Jacobian and whole-turn checks (the same functions) on the
    device's eval_constraints: rows g[-28:] are the curve's exact extrema within 1e-12 and finite at
    qd0 = 0, x = 0 (on the device NaN and infinity comparing false in t_mm > 0 && t_mm < t_move depends
    on how nlp_kernels.hip is compiled); J[-28:, i] k_range[i] is the central difference of the model's
    extrema (the factor stays: the reference differentiates in k_actual), the collision rows' Jacobian that
    of g, both within 1e-7 at h = 1e-6. Measured on the MI355X, both engines: exact extrema within 1.2e-13
    (q0 = 1000 rad), sampling 4.1e-11, extremum Jacobian 4.0e-10, collision Jacobian 2.4e-10, 51 joints
    compared on the interior branch; seven whole turns: rows 2.9e-13, k_opt 4.5e-11"""
    worlds = [refs[n]["wd"] for n in BATCH]
    P = planner(eng, len(worlds))
    P.reach(worlds)
    worst = [0.0, 0.0, 0.0, 0.0]
    n_in = 0
    for w, n in enumerate(BATCH):
        ev, wd = DeviceEval(P, w), refs[n]["wd"]
        for lb, x in E.eval_points(wd):
            d = E.check_extrema(ev, wd, x, f"{n} {lb}")
            worst[0], worst[1] = max(worst[0], d[0]), max(worst[1], d[1])
        we, wc, _, ni = check_jacobians(ev, wd, None, robot, n)
        worst[2], worst[3], n_in = max(worst[2], we), max(worst[3], wc), n_in + ni
    print(f"{eng}: exact {worst[0]:.2e} sampling {worst[1]:.2e} extremum J {worst[2]:.2e} collision J {worst[3]:.2e} "
          f"interior-branch joints {n_in}")
    assert n_in >= 4
    res, _ = P.plan(worlds)
    a, b = BATCH.index("branch_a"), BATCH.index("branch_a_turns")
    check_shift(DeviceEval(P, a), DeviceEval(P, b), 7, res[a], res[b])
    assert_paths(P.path_counts(), **armtd_only(eng))


@pytest.mark.parametrize("eng", ENGINES)
def test_crafted_tables_device_sets_are_the_affine_model(fx, robot, eng):
    """radius-free crafted tables, W = 1 (two bundles, 36 live lanes in the second): parity with the
    oracle, every corner of the affine model inside the device's sliced link zonotopes (SLACK = 1e-9 of
    tests/test_oracle_containment.py; the oracle measures 1.7e-16 m), and the model at -x outside by more
    than 1 cm in more than half of the 700 samples (436 and 429 on the oracle). Measured on the MI355X,
    both engines: excess 1.7e-16 m; 436 and 429 samples out, up to 10.4 cm"""
    wd = E.crafted_world(obstacles=E.by_name(fx, "graze_rest")[5])
    P = planner(eng, 1)
    P.reach([wd])
    R = OracleArmtd(*wd, T=T, threads=8)
    R.reach()
    np.testing.assert_allclose(P.link_generators(0), R.link_gens(), rtol=0, atol=TOL)
    for x in E.crafted_points() + [x for _, x in E.eval_points(wd)]:
        go, Jo = R.eval(x)
        assert_rows(P, 0, R, x, go, Jo, "crafted")
    ev = DeviceEval(P, 0)
    worst = E.check_radius_free(ev, robot, wd, SLACK)
    out = E.check_sensitivity(ev, robot, wd)
    print(f"{eng}: radius-free excess {worst:.3e} m; at -x out of 700, largest [m]: {out}")
    res, _ = P.plan([wd])
    assert_plan(res[0], R.plan(), "crafted")
    assert_paths(P.path_counts(), **armtd_only(eng))


# ---- shapes -------------------------------------------------------------------------------------
def _snapshot(P, worlds, x):
    P.reach(worlds)
    ev = [P.eval_constraints(w, x) for w in range(len(worlds))]
    res, _ = P.plan(worlds)
    return ev, res, [P.constraints(w) for w in range(len(worlds))]


def _same(a, b, bitwise, label):
    (ga, Ja), ra, ca = a
    (gb, Jb), rb, cb = b
    if bitwise:
        np.testing.assert_array_equal(ga, gb, err_msg=label)
        np.testing.assert_array_equal(Ja, Jb, err_msg=label)
        np.testing.assert_array_equal(ra["k_opt"], rb["k_opt"], err_msg=label)
        np.testing.assert_array_equal(ca, cb, err_msg=label)
        assert (ra["status"], ra["iterations"], ra["feasible"]) == (rb["status"], rb["iterations"], rb["feasible"]), label
        return
    # the bundle engine sums a job's pruned amounts over its bundle's union groups: across batch positions
    # values agree to rounding and decisions are identical (test_rerun_bitwise_and_batch_position_stable)
    assert np.abs(ra["k_opt"] - rb["k_opt"]).max() < 1e-8, label
    assert ra["feasible"] == rb["feasible"] and ra["iterations"] == rb["iterations"], label
    assert np.abs(ca - cb).max() < TOL and np.abs(ga - gb).max() < TOL, label
    rows = B.collision_slice(T, 7, 3, nt=0)
    np.testing.assert_array_equal(ca[rows] > B.COL_THR, cb[rows] > B.COL_THR, err_msg=label)


@pytest.mark.parametrize("eng", ENGINES)
def test_batch_shapes_and_positions(refs, eng):
    """W = 1 (2 bundles, 36 live lanes in the second), W = 3 (5 bundles, 44 in the last) and all twelve in
    one batch against the oracle's plans; a world alone, first and last in a batch gives bitwise the same
    rows and plan on the per-job engine, and on the bundle engine agrees within the bound of
    test_rerun_bitwise_and_batch_position_stable; a rerun is bitwise the same on both.
    The per-job engine has two kernels: batches of at most two jobs per CU (W = 1, W = 3) take the
    256-thread one, the twelve-world batch the 128-thread one, whose block reductions sum in another order.
    Measured: 7 of 2128 rows differ by one ulp (1.1e-16) between the two. So the bitwise claim is held
    between positions under one kernel, the twelve-world batch is held to the bundle engine's bound, and
    the census says which kernel each planner took."""
    x = np.linspace(-0.7, 0.7, 7)
    name = "tiny"
    wd = refs[name]["wd"]
    others = [refs[n]["wd"] for n in ("graze_rest", "binedge")]
    P1, P3 = planner(eng, 1), planner(eng, 3)
    Pa = planner(eng, len(BATCH))
    alone = _snapshot(P1, [wd], x)
    assert_plan(alone[1][0], refs[name]["plan"], "W = 1")
    first = _snapshot(P3, [wd] + others, x)
    last = _snapshot(P3, others + [wd], x)
    for w, n in enumerate((name, "graze_rest", "binedge")):
        assert_plan(first[1][w], refs[n]["plan"], f"W = 3 {n}")
    order = [n for n in BATCH if n != name] + [name]
    full = _snapshot(Pa, [refs[n]["wd"] for n in order], x)
    for w, n in enumerate(order):
        assert_plan(full[1][w], refs[n]["plan"], f"W = 12 {n}")
    pick = lambda s, w: (s[0][w], s[1][w], s[2][w])
    bitwise = eng == "job"
    _same(pick(alone, 0), pick(first, 0), bitwise, "alone / first of 3")
    _same(pick(alone, 0), pick(last, 2), bitwise, "alone / last of 3")
    _same(pick(alone, 0), pick(full, len(order) - 1), False, "alone / last of 12")
    if eng == "job":
        for P in (P1, P3):
            assert_paths(P.path_counts(), ran=("reach_job_256",), not_ran=("reach_job_128",))
        assert_paths(Pa.path_counts(), ran=("reach_job_128",), not_ran=("reach_job_256",))
    again = _snapshot(P3, others + [wd], x)
    for w in range(3):
        _same(pick(last, w), pick(again, w), True, f"rerun {w}")
    assert_paths(Pa.path_counts(), **armtd_only(eng))


# ---- no obstacles -------------------------------------------------------------------------------
@pytest.mark.parametrize("eng", ENGINES)
def test_no_obstacles(refs, eng):
    """an ARMTD world with O = 0: m = 28, the rows are the extremum rows alone, the plan is the oracle's,
    the getters have the documented sizes"""
    wd, R = refs["none"]["wd"], refs["none"]["ev"].R
    P = planner(eng, 2)
    assert P.num_constraints(0) == 28 and P.num_constraints(3) == 7 * T * 3 + 28
    P.reach([wd, wd])
    for lb, x, (go, Jo) in refs["none"]["at"]:
        for w in range(2):
            g, J = P.eval_constraints(w, x)
            assert g.shape == (28,) and J.shape == (28, 7)
            np.testing.assert_allclose(g, go, rtol=0, atol=TOL, err_msg=lb)
            np.testing.assert_allclose(J, Jo, rtol=0, atol=TOL, err_msg=lb)
        E.check_extrema(DeviceEval(P, 0), wd, x, f"none {lb}")
    np.testing.assert_allclose(P.link_generators(1), R.link_gens(), rtol=0, atol=TOL)
    res, _ = P.plan([wd, wd])
    for w in range(2):
        assert_plan(res[w], refs["none"]["plan"], "none")
        assert P.constraints(w).shape == (28,)
        assert P.link_centers(w).shape == (T, 7, 3) and P.link_generators(w).shape == (T, 7, 3, 6)
        np.testing.assert_allclose(P.constraints(w), R.eval(res[w]["k_opt"], jac=False), rtol=0, atol=1e-7)
        lc = R.eval(res[w]["k_opt"], centers=True)[2]
        np.testing.assert_allclose(P.link_centers(w), lc, rtol=0, atol=TOL)
    np.testing.assert_array_equal(res[0]["k_opt"], res[1]["k_opt"])
    assert_paths(P.path_counts(), **armtd_only(eng))


# ---- the certified plane cache on the ARMTD instantiation ----------------------------------------
@pytest.mark.parametrize("eng", ENGINES)
def test_plane_cache_against_full_scan(refs, eng):
    """ARMOUR_PLANE_CACHE unset and = 0 give bitwise equal g, J and plans on the graze worlds (collision
    rows within 1e-3 of the threshold): eval_kernel_t<double, true, true> against <double, true, false>"""
    graze = ("tiny", "binedge", "graze_rest", "crafted")
    worlds = [refs[n]["wd"] for n in graze[:3]] + [E.crafted_world(obstacles=refs["graze_rest"]["wd"][5])]
    prev = os.environ.pop("ARMOUR_PLANE_CACHE", None)
    try:
        P = planner(eng, len(worlds))
        with env("ARMOUR_PLANE_CACHE", "0"):
            Q = planner(eng, len(worlds))
    finally:
        if prev is not None:
            os.environ["ARMOUR_PLANE_CACHE"] = prev
    P.reach(worlds)
    Q.reach(worlds)
    rng = np.random.default_rng(11)
    xs = [np.zeros(7), np.ones(7), -np.ones(7)] + [rng.uniform(-1, 1, 7) for _ in range(3)]
    for x in xs:
        for w in range(len(worlds)):
            g, J = P.eval_constraints(w, x)
            gq, Jq = Q.eval_constraints(w, x)
            np.testing.assert_array_equal(g, gq, err_msg=graze[w])
            np.testing.assert_array_equal(J, Jq, err_msg=graze[w])
    ra, _ = P.plan(worlds)
    rb, _ = Q.plan(worlds)
    for w, (a, b) in enumerate(zip(ra, rb)):
        assert a["feasible"] == b["feasible"] and a["status"] == b["status"] and a["iterations"] == b["iterations"], graze[w]
        np.testing.assert_array_equal(a["k_opt"], b["k_opt"], err_msg=graze[w])
        np.testing.assert_array_equal(P.constraints(w), Q.constraints(w), err_msg=graze[w])
    for w, n in enumerate(graze[:3]):
        assert_plan(ra[w], refs[n]["plan"], n)
    pa, pq = armtd_only(eng), armtd_only(eng)
    assert_paths(P.path_counts(), ran=pa["ran"] + ("pc_builds", "eval_cached"), not_ran=pa["not_ran"] + ("pc_fallbacks",))
    assert_paths(Q.path_counts(), ran=pq["ran"] + ("eval_full_scan",), not_ran=pq["not_ran"] + ("pc_builds", "eval_cached"))


# ---- the fp32 study on an ARMTD planner ----------------------------------------------------------
def test_eval_f32_on_an_armtd_planner(refs):
    """ARMOUR_EVAL_F32 on an ARMTD planner (eval_kernel_t<float, true, false>), at the bar of
    tests/test_gpu_fp32.py for the ARMOUR instantiation: every value finite, the collision rows' median
    distance from fp64 below 1e-6, it really ran in float, and the fp64 path is untouched when unset.
    Measured: median 1.8e-8 to 3.0e-8. The largest single row is not part of that bar for the Kinova and is
    printed only: 3.0e-7 on tiny, but 2.4e-2 to 1.1e-1 m on single rows of binedge, branch_b and
    graze_rest. Those rows (3 to 52 per world) are all rows of link 0, whose centre does not depend on x
    (zero Jacobian in both), 15 cm or more clear of the threshold, and the sliced centres agree within 2e-7:
    the difference is in the planes the float scan forms from that link's generators, not in the ARMTD
    slices (cause not traced further; the float path is a study, never the product path)"""
    names = ("tiny", "binedge", "branch_b", "graze_rest")
    worlds = [refs[n]["wd"] for n in names]
    x = np.linspace(-0.6, 0.6, 7)

    def run(f32):
        old = os.environ.pop("ARMOUR_EVAL_F32", None)
        try:
            if f32:
                os.environ["ARMOUR_EVAL_F32"] = "1"
            P = A.ArmtdPlanner(T=T, max_obstacles=3, max_worlds=len(worlds))
        finally:
            os.environ.pop("ARMOUR_EVAL_F32", None)
            if old is not None:
                os.environ["ARMOUR_EVAL_F32"] = old
        P.reach(worlds)
        out = [P.eval_constraints(w, x) for w in range(len(worlds))]
        if f32:
            assert_paths(P.path_counts(), ran=("eval_armtd_f32", "eval_full_scan"),
                         not_ran=ARMOUR_EVALS + ("eval_armtd_f64", "eval_cached", "pc_builds"))
        else:
            assert_paths(P.path_counts(), ran=("eval_armtd_f64", "eval_cached", "pc_builds"),
                         not_ran=ARMOUR_EVALS + ("eval_armtd_f32", "eval_full_scan"))
        return out

    a, b, c = run(False), run(True), run(False)
    nc = 7 * T * 3
    for n, (g64, J64), (g32, J32), (g0, J0) in zip(names, a, b, c):
        assert np.all(np.isfinite(g32)) and np.all(np.isfinite(J32)), n
        dc = np.abs(g32[:nc] - g64[:nc])
        print(f"{n}: collision rows fp32 - fp64 median {np.median(dc):.2e} max {dc.max():.2e}")
        assert np.median(dc) < 1e-6, n
        assert not np.array_equal(g32, g64), n
        assert np.array_equal(g64, g0) and np.array_equal(J64, J0), n


# ---- drop-in ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["rest", "none"])
def test_armtd_main_on_rest_and_no_obstacles(refs, tmp_path, name):
    """armtd_main through the reference's file protocol on the rest start (the reference's first plan
    and every plan after a brake) and on a world without obstacles; inputs rounded by the writer's %.10f
    as in test_armtd_main_protocol"""
    wd = refs[name]["wd"]
    O = len(wd[5])
    write_armtd_in(str(tmp_path), *wd)
    r = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ARMOUR_NUM_TIME_STEPS=str(T)))
    assert r.returncode == 0, r.stderr
    out = [float(v) for v in open(tmp_path / "armtd.out").read().split()]
    rounded = tuple(np.round(np.asarray(a, dtype=np.float64), 10) for a in wd)
    P = A.ArmtdPlanner(T=T, max_obstacles=max(O, 1), max_worlds=1)
    res, _ = P.plan([rounded])
    assert res[0]["feasible"] and refs[name]["plan"]["feasible"]
    assert len(out) == 8
    np.testing.assert_allclose(out[:7], res[0]["k_opt"], rtol=1e-9, atol=1e-9)
    c = np.loadtxt(tmp_path / "armtd_joint_position_center.out")
    assert c.shape == (T * 7, 3)
    np.testing.assert_allclose(c.reshape(T, 7, 3), P.link_centers(0), rtol=1e-9, atol=1e-9)
    gens = np.loadtxt(tmp_path / "armtd_joint_position_radius.out")
    np.testing.assert_allclose(gens.reshape(T, 7, 3, 6), P.link_generators(0), rtol=1e-9, atol=1e-12)
    cons = np.loadtxt(tmp_path / "armtd_constraints.out")
    assert cons.shape == (7 * T * O + 28,)
    np.testing.assert_allclose(cons, P.constraints(0), rtol=1e-5, atol=1e-5)
    assert np.all(np.isfinite(cons))
