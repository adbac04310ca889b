"""The HIP path on general zonotope obstacles (tests/golden/zonotope_worlds.npz; kinds, placement and
figures in tests/test_zonotope_obstacles.py): every obstacle the other GPU tests use is an
axis-aligned box, on which each obstacle generator has one non-zero component and most of the
plane arithmetic of nlp_kernels.hip (mixed_plane, oo_table / oo_complete, the plane cache's bounds)
multiplies zeros.

  * against the oracle, test_gpu_parity.py's bars: g and J within 1e-9, every collision decision
    and the feasibility re-check identical; Fetch included; one Kinova world on a planner built for
    40 obstacles while the batch carries 20;
  * against tests/collision_model.py, on the GPU's own link generators and link centres: the check
    that does not pass through the oracle (bounds and exclusion caps of the CPU test);
  * the evaluation variants bitwise: plane cache against ARMOUR_PLANE_CACHE=0, eval_kernel_small
    against ARMOUR_EVAL_FULL=1, at every point including the one outside the certified box;
  * plans against OraclePlanner.plan(), cached against uncached bitwise;
  * the ARMTD planner and the fp32 study path on the same kinds.

One planner and one run per (world, variant), shared by the tests and left unchanged.

Measured on an MI355X: |g - g_oracle| <= 7.2e-15 and |J - J_oracle| <= 3e-16 over all worlds and points;
against the model, worst |g - g_model| / bound = 0.0067, worst |J - J_model| = 1.88e-13, no row excluded;
5.5 to 6.7 of 36 planes kept per pair by the plane cache; fp32 collision rows within 5.2e-7 of fp64
(8.7e-5 on the 1e3 m obstacle). With one term of mixed_plane<0>'s cross product dropped, or with
oo_table pairing generators (0, 1) twice, test_against_oracle and test_against_model fail on every
world (differences of 1 to 2 cm on rotated and sheared obstacles) while the box-only tests
(parity, boundary, plane cache, ARMTD, small-capacity kernels) still pass.
"""
import numpy as np
import pytest

import armour_amd as A
import boundary_worlds as B
import test_zonotope_obstacles as Z
from conftest import engine
from oracle import OracleArmtd, OraclePlanner
from paths import assert_paths, engine_paths
from test_armtd import load as load_armtd, world as armtd_world
from test_gpu_plane_cache import check_eval, check_plan, env

pytestmark = pytest.mark.gpu
TOL = 1e-9  # test_gpu_parity.TOL
COL_THR = B.COL_THR
KINOVA = [n for n in Z.names() if n.startswith("kinova")]
WIDE = "kinova0"  # runs on a planner built with max_obstacles = 40 while the batch carries 20

_planners, _runs = {}, {}


def planner(name, variant="default"):
    """variant: "default"; "nocache" (ARMOUR_PLANE_CACHE=0); "full" (ARMOUR_EVAL_FULL=1). All on the
    bundle engine, which records the PZ sizes the small-capacity kernels are chosen by."""
    if (name, variant) not in _planners:
        cs = Z.case(name)
        _, _, tables = B.robot_of(cs["robot"])
        O = 40 if name == WIDE else cs["O"]
        key, val = {"default": ("ARMOUR_PLANE_CACHE", "1"), "nocache": ("ARMOUR_PLANE_CACHE", "0"),
                    "full": ("ARMOUR_EVAL_FULL", "1")}[variant]
        with engine("lane"), env(key, val):
            _planners[name, variant] = A.Planner(T=cs["T"], max_obstacles=O, max_worlds=1, robot=tables)
    return _planners[name, variant]


def assert_variant_paths(name, variant):
    """the census of planner(name, variant) after it evaluated or planned: the bundle engine, and the
    evaluation kernels of its variant (the small-capacity ones only for the Kinova's at most 280 pairs)"""
    lane = engine_paths("lane")
    small = ("eval_small",) if Z.case(name)["robot"] == "kinova" else ()
    ran, not_ran = {"default": (("pc_builds", "eval_cached") + small, ("pc_fallbacks",) + (() if small else ("eval_small",))),
                    "nocache": (("eval_full_scan",), ("pc_builds", "eval_cached", "eval_small", "trials_small")),
                    "full": (("pc_builds", "eval_cached", "eval_f64"), ("eval_small", "trials_small"))}[variant]
    assert_paths(planner(name, variant).path_counts(), ran=lane["ran"] + ran, not_ran=lane["not_ran"] + not_ran)


def run(name):
    """the default planner on one fixture world: per point g, J, the link centres
    (armour_get_link_centers after armour_eval_constraints) and their central differences"""
    if name not in _runs:
        cs, P = Z.case(name), planner(name)
        P.reach([cs["world"]])

        def centres_at(y):
            P.eval_constraints(0, y, jac=False)
            return P.link_centers(0)

        pts = []
        for x in cs["points"]:
            dc = Z.central_differences(centres_at, x)
            g, J = P.eval_constraints(0, x)
            pts.append(dict(x=x, g=g, J=J, lc=P.link_centers(0), dc=dc))
        _runs[name] = dict(NJ=P.NJ, link_gens=P.link_generators(0), points=pts,
                           stats=P.plane_cache_stats(), occupancy=P.occupancy())
    assert_variant_paths(name, "default")
    return _runs[name]


@pytest.mark.parametrize("name", Z.names())
def test_against_oracle(name):
    cs, got, ref = Z.case(name), run(name), Z.reference(name)
    R = ref["R"]
    rows = B.collision_slice(cs["T"], R.NJ, cs["O"])
    assert got["NJ"] == R.NJ
    np.testing.assert_allclose(got["link_gens"], ref["link_gens"], rtol=0, atol=TOL)
    for k, (p, q) in enumerate(zip(got["points"], ref["points"])):
        dg, dJ = np.abs(p["g"] - q["g"]).max(), np.abs(p["J"] - q["J"]).max()
        print(f"{name} point {k}: |dg| {dg:.2e} |dJ| {dJ:.2e}")
        np.testing.assert_allclose(p["g"], q["g"], rtol=0, atol=TOL, err_msg=f"point {k}")
        np.testing.assert_allclose(p["J"], q["J"], rtol=0, atol=TOL, err_msg=f"point {k}")
        np.testing.assert_array_equal(p["g"][rows] > COL_THR, q["g"][rows] > COL_THR)
        assert R.feasible(p["g"]) == R.feasible(q["g"])
        np.testing.assert_allclose(p["lc"], q["lc"], rtol=0, atol=TOL)


@pytest.mark.parametrize("name", Z.names())
def test_against_model(name):
    cs, got = Z.case(name), run(name)
    fig = Z.compare_with_model(cs, got["NJ"], got["link_gens"], got["points"], f"gpu {name}")
    print(f"{name}: {fig}")


@pytest.mark.parametrize("name", Z.names())
def test_variants_bitwise(name):
    """plane cache against the full scan, small-capacity kernels against the full-capacity ones"""
    cs, got = Z.case(name), run(name)
    worlds = [cs["world"]]
    pairs = [("nocache", planner(name, "nocache"))]
    if cs["robot"] == "kinova":  # Fetch's 320 pairs are above the small kernels' 280: full-capacity in both
        pairs.append(("full", planner(name, "full")))
    for label, Q in pairs:
        P = planner(name)
        check_eval(P, Q, worlds, np.random.default_rng(3), n=2)
        for k, p in enumerate(got["points"]):
            g, J = Q.eval_constraints(0, p["x"])
            np.testing.assert_array_equal(g, p["g"], err_msg=f"{label} point {k}")
            np.testing.assert_array_equal(J, p["J"], err_msg=f"{label} point {k}")
        assert_variant_paths(name, label)
    NJ, st = got["NJ"], got["stats"]
    print(f"{name}: plane cache {st}, occupancy {got['occupancy']}")
    assert st["box_misses"] == 0 and planner(name).plane_cache_stats()["box_misses"] == 0
    assert st["pairs"] == cs["T"] * NJ * cs["O"] and st["blocks_cached"] == st["blocks"]
    assert st["planes_kept"] < 36 * st["pairs"] and 1 <= st["max_per_pair"] <= 36  # it really pruned
    if cs["robot"] == "kinova":  # the small-capacity kernels ran (planner.hip eval_small_fits)
        occ = got["occupancy"]
        assert occ["link_monomials"][0] <= 16 and occ["torque_monomials"][0] <= 64
        assert NJ * cs["O"] <= 280


@pytest.mark.parametrize("name", KINOVA)
def test_plans(name):
    """the plan against the oracle's (every world holds an obstacle containing the arm: the plans
    are infeasible, decided on the collision rows), and cached against uncached bitwise"""
    cs, ref = Z.case(name), Z.reference(name)
    P, Q = planner(name), planner(name, "nocache")
    res, _ = P.plan([cs["world"]])
    r, ro = res[0], ref["R"].plan()
    print(f"{name}: feasible={r['feasible']} status={r['status']} iterations={r['iterations']} "
          f"(oracle {ro['feasible']} {ro['status']} {ro['iterations']}) |dk_opt|={np.abs(r['k_opt'] - ro['k_opt']).max():.1e}")
    assert r["feasible"] == ro["feasible"] and r["status"] == ro["status"]
    assert r["iterations"] == ro["iterations"]
    tol = 1e-8 if (r["status"] == 0 or r["feasible"]) else 1e-3  # test_gpu_boundary.compare_set
    np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=tol)
    check_plan(P, Q, [cs["world"]])
    # the same world with the containing obstacle replaced by a second copy of obstacle 0: the
    # solver works against the other kinds' rows instead of stopping on a row no x can clear
    obs = cs["world"][4].copy()
    obs[cs["kinds"] == "contain"] = obs[0]
    world = cs["world"][:4] + (obs,)
    R = OraclePlanner(*world, T=cs["T"], threads=4)
    R.reach()
    res, _ = P.plan([world])
    r, ro = res[0], R.plan()
    print(f"{name} without the containing obstacle: feasible={r['feasible']} status={r['status']} "
          f"iterations={r['iterations']} (oracle {ro['feasible']} {ro['status']} {ro['iterations']}) "
          f"|dk_opt|={np.abs(r['k_opt'] - ro['k_opt']).max():.1e}")
    # an addition to the fixture's plans, held to test_gpu_boundary.compare_set's rules in full: a plan
    # that ends in local infeasibility (status 4) may differ by a few iterations, its k_opt is unused
    local_infeasible = r["status"] == 4 and not r["feasible"]
    assert r["feasible"] == ro["feasible"] and r["status"] == ro["status"]
    assert abs(r["iterations"] - ro["iterations"]) <= (5 if local_infeasible else 0)
    tol = 1e-8 if (r["status"] == 0 or r["feasible"]) else 1e-3
    if not local_infeasible:
        np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=tol)
    check_plan(P, Q, [world])
    assert_variant_paths(name, "default")
    assert_variant_paths(name, "nocache")
    _runs.pop(name, None)  # the planner has moved on; a later run() evaluates again


def test_armtd():
    """world 0 of tests/golden/armtd_T100_O10.npz with its obstacles replaced by ten of the kinds,
    at test_gpu_armtd.py's bar"""
    fx, zf = load_armtd(), Z.fixture()
    T = int(fx["T"])
    obs = zf["armtd_obstacles"]
    O = obs.shape[0]
    world = armtd_world(fx, 0)[:5] + (obs,)
    P = A.ArmtdPlanner(T=T, max_obstacles=O, max_worlds=1)
    P.reach([world])
    R = OracleArmtd(*world, T=T, threads=8)
    R.reach()
    np.testing.assert_allclose(P.link_generators(0), R.link_gens(), rtol=0, atol=TOL)
    cs = B.collision_slice(T, 7, O, nt=0)
    for x in (zf["armtd_x_star"], np.zeros(7), np.linspace(-0.8, 0.8, 7)):
        g, J = P.eval_constraints(0, x)
        go, Jo = R.eval(x)
        np.testing.assert_allclose(g, go, rtol=0, atol=TOL)
        np.testing.assert_allclose(J, Jo, rtol=0, atol=TOL)
        np.testing.assert_array_equal(g[cs] > COL_THR, go[cs] > COL_THR)
        assert R.feasible(g) == R.feasible(go)
    col = R.eval(zf["armtd_x_star"], jac=False)[cs].reshape(7, T, O)
    for o, (t, l, v) in enumerate(zf["armtd_targets"]):  # the placement holds on the oracle's rows
        assert abs(col[int(l), int(t), o] - v) < 1e-9
    res, _ = P.plan([world])
    r, ro = res[0], R.plan()
    assert r["feasible"] == ro["feasible"] and r["status"] == ro["status"] and r["iterations"] == ro["iterations"]
    tol = 1e-8 if (r["status"] == 0 or r["feasible"]) else 1e-3
    np.testing.assert_allclose(r["k_opt"], ro["k_opt"], rtol=0, atol=tol)
    np.testing.assert_allclose(P.constraints(0), R.eval(r["k_opt"], jac=False), rtol=0, atol=1e-7)
    assert_paths(P.path_counts(), ran=("eval_armtd_f64",), not_ran=("eval_f64", "eval_small", "eval_f32", "eval_armtd_f32"))


def test_fp32_study_path():
    """ARMOUR_EVAL_F32=1 on one Kinova world: finite everywhere; collision rows within
    test_gpu_fp32.py's 5e-6 of fp64 on every kind except the 1e3 m obstacle, which fp32 cannot
    resolve (its rows are only required to be finite)"""
    name = "kinova1"
    cs, got = Z.case(name), run(name)
    with engine("lane"), env("ARMOUR_EVAL_F32", "1"):
        F = A.Planner(T=cs["T"], max_obstacles=cs["O"], max_worlds=1)
    F.reach([cs["world"]])
    rows = B.collision_slice(cs["T"], got["NJ"], cs["O"])
    huge = cs["kinds"] == "huge"
    for k, p in enumerate(got["points"]):
        g32, J32 = F.eval_constraints(0, p["x"])
        assert np.all(np.isfinite(g32)) and np.all(np.isfinite(J32))
        d = np.abs(g32[rows] - p["g"][rows]).reshape(got["NJ"], cs["T"], cs["O"])
        print(f"fp32 point {k}: worst {d[..., ~huge].max():.2e}, on the 1e3 m obstacle {d[..., huge].max():.2e}")
        assert d[..., ~huge].max() < 5e-6
        assert not np.array_equal(g32, p["g"])  # it really ran in float
    assert_paths(F.path_counts(), ran=("eval_f32", "eval_full_scan") + engine_paths("lane")["ran"],
                 not_ran=("eval_f64", "eval_small", "eval_cached", "pc_builds") + engine_paths("lane")["not_ran"])
