"""The ARMTD comparison planner's oracle (oracle/src/armtd.cpp) against tests/armtd_model.py, a numpy
statement of what its rows and sets mean that shares no code with it, on the edge worlds of
tests/armtd_edges.py and on crafted tables. The HIP path runs the same checks (the same functions) in
tests/test_gpu_armtd_edges.py.

Point containment with the reference's own tables cannot see a wrong ARMTD planner: the reference scales
the JRS radius by 5 (ACMP/Trajectory.cu:43,56), and with that factor sets sliced at -x still contain the
curve of +x at |x| = 1 with 2 to 8 cm to spare (fixture world 1), and a q0 shift of 0.01 rad passes. So:

  * the reference's tables are held to their own radius WITHOUT the factor (test_reference_tables_*),
  * the extremum rows to the curve's exact extrema, 1e-12, at the x where their branches change,
  * the Jacobian and cost gradient to central differences of the model,
  * the link sets to the affine model with radius-free crafted tables, where nothing hides a sign,
    a swapped row or a wrong rotation by q0; and that check's own sensitivity is asserted.
"""
import numpy as np
import pytest

import armtd_edges as E
import armtd_model as M
import boundary_worlds as B
from armour_amd import robot_tables as RT
from oracle import OracleArmtd
from test_armtd import load as load_random, world as random_world
from test_domain_edges import IDENTITY, MARGIN
from test_oracle_containment import SLACK

EDGE_NAMES = ("rest", "rest_kzero", "tiny", "binedge", "fast", "branch_a", "branch_b", "branch_a_turns", "limit_0.05",
              "limit_0.001", "wrap", "none", "graze_rest")


class OracleEval:
    """the evaluator of tests/armtd_edges.py on the oracle"""

    def __init__(self, wd, threads=8):
        self.R = OracleArmtd(*wd, T=E.T, threads=threads)
        self.R.reach()

    def eval(self, x):
        return self.R.eval(x, centers=True)

    def gens(self):
        return self.R.link_gens()


@pytest.fixture(scope="module")
def fx():
    return E.load()


@pytest.fixture(scope="module")
def robot():
    return RT.builtin(0)   # the header's tables, the oracle's and the HIP path's robot 0


@pytest.fixture(scope="module")
def crafted():
    wd = E.crafted_world()
    return wd, OracleEval(wd)


def test_fixture_names(fx):
    assert tuple(E.names(fx)) == EDGE_NAMES


# ---- the fixture --------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_oracle_reproduces_edge_fixture(fx, name):
    w = E.names(fx).index(name)
    wd = E.world(fx, w)
    assert E.digest(wd) == str(fx["sha1"][w])
    R = OracleArmtd(*wd, T=E.T, threads=4)
    R.reach()
    r = R.plan()
    assert r["feasible"] == bool(fx["feasible"][w]) and r["status"] == fx["status"][w]
    assert r["iterations"] == fx["iterations"][w]
    np.testing.assert_allclose(r["k_opt"], fx["k_opt"][w], rtol=0, atol=1e-10)
    O = int(fx["n_obs"][w])
    if O:
        g0 = R.eval(np.zeros(7), jac=False)
        assert B.near_threshold_rows(g0, E.T, 7, O, nt=0) == fx["near_x0"][w]


def test_edge_fixture_holds_what_it_was_built_for(fx):
    n = E.names(fx)
    st = {k: (bool(f), int(s)) for k, f, s in zip(n, fx["feasible"], fx["status"])}
    assert st["fast"] == (False, 4) and st["limit_0.001"] == (False, 4) and st["limit_0.05"] == (True, 0)
    assert int(np.sum(fx["near_x0"] > 0)) >= 2                                  # rows within 1e-3 of the threshold
    assert fx["near_x0"][n.index("graze_rest")] > 0 and fx["near_x0"][n.index("tiny")] > 0
    for k in ("rest", "rest_kzero", "graze_rest"):
        assert not fx["qd0"][n.index(k)].any()
    # k_opt = 0 on two joints, to the solver's tolerance: 1e-7 on a gradient of 20 (k_range / 8)^2 k = 5e-3 k
    assert np.abs(fx["k_opt"][n.index("rest_kzero")][[2, 5]]).max() < 1e-4
    assert fx["n_obs"][n.index("none")] == 0
    # tiny: t_mm inside (0, 0.5), on 0.5 at x = -sign(qd0), next to 0
    wd = E.by_name(fx, "tiny")
    qd0, kr = wd[1], wd[4]
    assert np.all(np.abs(qd0[:4]) < 0.5 * kr[:4]) and np.all(np.abs(qd0[4:6]) == 0.5 * kr[4:6]) and qd0[6] == 1e-9
    # binedge: every speed as far from its table's own as the grid allows
    import offline_jrs as OJ
    b = E.by_name(fx, "binedge")[1]
    d = np.abs(b[:, None] - OJ.C_KVI[None, :]).min(axis=1)
    np.testing.assert_allclose(d, 0.5 * (OJ.C_KVI[1] - OJ.C_KVI[0]), rtol=1e-9)
    # the limit rows decide the limit worlds: the position row of a limited joint is the largest violation
    # (limit_0.001) or active at the plan (limit_0.05)
    for name, active in (("limit_0.001", False), ("limit_0.05", True)):
        wd = E.by_name(fx, name)
        R = OracleArmtd(*wd, T=E.T, threads=4)
        R.reach()
        gl, gu = R.bounds()
        g = R.eval(fx["k_opt"][n.index(name)], jac=False)
        over = np.maximum(g[-28:-14] - gu[-28:-14], gl[-28:-14] - g[-28:-14]).reshape(2, 7)
        assert g[:-28].max() < 0 and np.all(over[:, list(E.CONT)] < -1)
        if active:
            assert -1e-6 < over[:, list(E.LIMITED)].max() <= 1e-8
        else:
            assert over[:, list(E.LIMITED)].max() > 1e-3
    # wrap: the goal is pi from q_plan(0) on joint 0
    wd = E.by_name(fx, "wrap")
    assert wd[2][0] - (wd[0][0] + 0.5 * wd[1][0]) == np.pi


# ---- the reference's tables ---------------------------------------------------------------------
def _enclosure(wd, rng, n=20):
    _, qd0, _, tab, kr, _ = wd
    worst = 0.0
    s = np.arange(E.T)
    for rep in range(n):
        x = np.sign(rng.uniform(-1, 1, 7)) if rep < 2 else rng.uniform(-1, 1, 7)
        for t in ((s + rng.uniform(0, 1, E.T)) / E.T, s / E.T, (s + 1) / E.T):
            worst = max(worst, M.table_enclosure(tab, kr, qd0, x, t))
    return worst


def test_reference_tables_enclose_the_curve_within_their_own_radius(fx):
    """cos / sin of the relative angle lie in c + g x +- r WITHOUT the planner's factor 5: worst
    |error| / r <= 1 over the 8 random fixture worlds and the edge worlds, random t and the interval ends,
    20 x per world with corners. Measured: 0.9975 on the random worlds, 0.9993 on the edge worlds (binedge,
    the largest distance from a table's own velocity). Pins the table layout, the meaning of k_range x and
    the slicing of tests/offline_jrs.py to within 1 % of the reference's own radius."""
    rng = np.random.default_rng(0)
    fr = load_random()
    worst_r = max(_enclosure(random_world(fr, w), rng) for w in range(8))
    worst_e = {n: _enclosure(E.by_name(fx, n), rng) for n in EDGE_NAMES}
    print(f"worst |error| / r: random worlds {worst_r:.4f}, edge worlds " + " ".join(f"{k}={v:.4f}" for k, v in worst_e.items()))
    assert worst_r <= 1.0
    assert max(worst_e.values()) <= 1.0, worst_e
    # the check sees a slice with x negated, and cos / sin tables swapped
    wd = random_world(fr, 1)
    neg, swp = wd[3].copy(), wd[3][:, [3, 4, 5, 0, 1, 2]]
    neg[:, [1, 4]] *= -1
    tm = (np.arange(E.T) + 0.5) / E.T
    assert M.table_enclosure(neg, wd[4], wd[1], np.ones(7), tm) > 2.0
    assert M.table_enclosure(swp, wd[4], wd[1], np.ones(7), tm) > 2.0


# ---- extremum rows ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EDGE_NAMES)
def test_oracle_extremum_rows_are_the_exact_extrema(fx, name):
    """g[-28:] against the curve's critical points (1e-12) and a 20001-point sampling, at x in {0, +-1,
    random, -sign(qd0), -0.999 sign(qd0), the x of t_mm = 0.5 and its neighbouring doubles}; every row
    finite at qd0 = 0, x = 0. Measured on the oracle: exact within 1.2e-13 (one ulp of 1000 rad, branch_b;
    1.8e-15 elsewhere), sampling within 4.1e-11."""
    wd = E.by_name(fx, name)
    ev = OracleEval(wd, threads=4)
    worst = (0.0, 0.0)
    for label, x in E.eval_points(wd):
        d = E.check_extrema(ev, wd, x, f"{name} {label}")
        worst = (max(worst[0], d[0]), max(worst[1], d[1]))
    print(f"{name}: exact {worst[0]:.2e} sampling {worst[1]:.2e}")


def test_model_extrema_bracket_its_own_curve():
    """the model against itself: the critical-point extrema bracket a dense sampling of the model's curve
    for random starts (the definition of the rows does not rest on the reference's branch text)"""
    rng = np.random.default_rng(3)
    ts = np.linspace(0, 1, 20001)
    for _ in range(50):
        q0, qd0, kr, x = rng.uniform(-1, 1, 7), rng.uniform(-0.3, 0.3, 7), rng.uniform(0.1, 1.0, 7), rng.uniform(-1, 1, 7)
        ext = M.extrema(q0, qd0, kr, x)
        q, qd = M.curve(q0, qd0, kr, x, ts)
        samp = np.array([q.min(0), q.max(0), qd.min(0), qd.max(0)])
        assert np.all(ext[[0, 2]] <= samp[[0, 2]] + 1e-15) and np.all(ext[[1, 3]] >= samp[[1, 3]] - 1e-15)
        assert np.abs(ext - samp).max() < 1e-8
        # the curve is C1 at t = 0.5 and ends at rest
        (qa, va), (qb, vb) = (M.curve(q0, qd0, kr, x, [t]) for t in (0.5, np.nextafter(0.5, 1)))
        assert np.abs(qa - qb).max() < 1e-15 and np.abs(va - vb).max() < 1e-14
        assert np.abs(M.curve(q0, qd0, kr, x, [1.0])[1]).max() < 1e-15


# ---- Jacobian rows and the cost -----------------------------------------------------------------
def jacobian_points(wd):
    """evaluation points off the kinks: random, a half of it, and points that put the interior extremum
    inside (0, 0.5) where the start speed allows (x = -0.97 sign(qd0), and 1.5 times the x of t_mm = 0.5)"""
    rng = np.random.default_rng(5)
    xh = E.half_time_x(wd[1], wd[4])
    pts = [rng.uniform(-0.95, 0.95, 7), rng.uniform(-0.5, 0.5, 7), -0.97 * np.sign(wd[1]) + 0.05 * (wd[1] == 0),
           np.clip(1.5 * xh, -0.9, 0.9) + 0.03 * (xh == 0)]
    return pts


def check_jacobians(ev, wd, cost_fn, robot, label):
    """the three Jacobian checks of one world; cost_fn(x) -> (f, grad), or None. Returns the worst errors and the
    number of joints compared on the interior branch"""
    q0, qd0, q_des, _, kr, _ = wd
    we, wc, wf, n_in = 0.0, 0.0, 0.0, 0
    for k, x in enumerate(jacobian_points(wd)):
        e, n, ni = E.check_extremum_jacobian(ev, wd, x, f"{label} {k}")
        we, n_in = max(we, e), n_in + ni
        if k < 2:
            wc = max(wc, E.check_collision_jacobian(ev, wd, x, f"{label} {k}")[0])
        if cost_fn is None:     # the HIP path returns the cost at the plan only
            continue
        f, grad = cost_fn(x)
        assert abs(f - M.cost(q0, qd0, kr, q_des, x, robot["wrap"])) <= 1e-12 * max(1.0, abs(f)), (label, k)
        fd = np.array([(M.cost(q0, qd0, kr, q_des, x + d, robot["wrap"]) - M.cost(q0, qd0, kr, q_des, x - d, robot["wrap"]))
                       / (2 * E.FD_H) for d in np.eye(7) * E.FD_H])
        wf = max(wf, float(np.abs(grad - fd).max()))
        assert wf <= E.FD_TOL, (label, k, "cost gradient", grad, fd)
        np.testing.assert_allclose(grad, M.cost_gradient(q0, qd0, kr, q_des, x, robot["wrap"]), rtol=0, atol=1e-12)
    return we, wc, wf, n_in


@pytest.mark.parametrize("name", EDGE_NAMES)
def test_oracle_jacobians_against_the_model(fx, robot, name):
    """J[-28:, i] k_range[i] equals the central difference of the model's extrema in x_i away from the
    kinks. The factor k_range stays: the reference differentiates in k_actual = k_range x, not in x
    (ACMP/Trajectory.cu:229-383), and this project keeps that; the solver sees
    J[-28:] as it is. The collision rows' Jacobian equals central differences of g, the cost and its
    gradient the model's. h = 1e-6, held to 1e-7; measured on the oracle: extremum rows <= 4.0e-10,
    collision rows <= 2.4e-10, cost <= 2.7e-8 (branch_b, q0 = 1000 rad; <= 1.6e-8 elsewhere)."""
    wd = E.by_name(fx, name)
    ev = OracleEval(wd, threads=8)
    we, wc, wf, n_in = check_jacobians(ev, wd, ev.R.cost, robot, name)
    print(f"{name}: extremum {we:.2e} collision {wc:.2e} cost {wf:.2e}, interior-branch joints {n_in}")
    if name == "tiny":
        assert n_in >= 4      # the interior extremum's gradient 0.5 qd0^2 / k_actual^2 is really compared


# ---- radius-free tables -------------------------------------------------------------------------
def test_oracle_sets_are_the_affine_model_with_radius_free_tables(robot, crafted):
    """With crafted tables of zero radius (every entry distinct, generators +-0.05) every corner the affine
    model gives at x lies in the oracle's sliced link zonotope, over all 100 intervals, 7 links, 8 corners,
    at x in {0, random, +1, -1}. Measured excess on the oracle with the header's tables
    (robot_tables.builtin(0)): 1.7e-16 m, rounding only (with the URDF-derived tables it is 4.8e-7, those
    tables' 6-decimal rounding, which is why the header's are used): within SLACK =
    1e-9 of tests/test_oracle_containment.py, which is the bound used here and on the HIP path."""
    wd, ev = crafted
    worst = E.check_radius_free(ev, robot, wd, SLACK)
    print(f"radius-free excess {worst:.3e} m")


def test_radius_free_check_sees_a_negated_slice(robot, crafted):
    """the model evaluated at -x lies outside the sets sliced at x by more than 1 cm in more than half of
    the 700 (interval, link) samples at |x| = 1. Measured on the oracle: 436 (x = +1) and 429 (x = -1) of 700 out, largest excess 10.4 cm."""
    wd, ev = crafted
    out = E.check_sensitivity(ev, robot, wd)
    print("samples out of 700, largest excess [m]:", out)


# ---- whole turns --------------------------------------------------------------------------------
def shift_distances(base, other, n):
    """tests/test_domain_edges.identity_distances for an ARMTD evaluator pair (no torque radius)"""
    d = dict(gens=np.abs(other.gens() - base.gens()).max(), centres=0.0, rows=0.0, jac=0.0)
    for x in (np.zeros(7), np.linspace(-0.9, 0.9, 7)):
        g, J, lc = other.eval(x)
        g0, J0, lc0 = base.eval(x)
        g = g.copy()
        for off in (-28, -21):
            g[[off + j for j in E.CONT]] -= 2 * np.pi * n
        d["centres"] = max(d["centres"], np.abs(lc - lc0).max())
        d["rows"] = max(d["rows"], np.abs(g - g0).max())
        d["jac"] = max(d["jac"], np.abs(J - J0).max())
    return d


def check_shift(base, other, n, plan_base, plan_other):
    d = shift_distances(base, other, n)
    assert plan_base["feasible"] == plan_other["feasible"] and plan_base["status"] == plan_other["status"]
    assert plan_base["iterations"] == plan_other["iterations"]
    d["k"] = np.abs(plan_base["k_opt"] - plan_other["k_opt"]).max()
    print(f"shift({n}): " + " ".join(f"{k}={v:.2e}" for k, v in d.items()))
    for key, v in d.items():
        assert v <= MARGIN * IDENTITY[n][key], (key, v, MARGIN * IDENTITY[n][key])


def test_oracle_whole_turns_change_nothing(fx):
    """branch_a_turns is branch_a with its continuous joints 7 turns on: the sets, every row but those
    joints' position extrema (which move by 14 pi), the Jacobian and the plan agree within the table of
    tests/test_domain_edges.py (IDENTITY[7] times MARGIN), no new numbers"""
    n = int(fx["shift_turns"])
    a, b = OracleEval(E.by_name(fx, "branch_a")), OracleEval(E.by_name(fx, "branch_a_turns"))
    check_shift(a, b, n, a.R.plan(), b.R.plan())
