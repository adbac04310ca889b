"""The oracle and the host emulation on the edges of the input domain (tests/domain_edges.py): multi-turn
angles, starts on the branch points of cos / sin, starts on and beyond the position and speed limits,
far goals. T = 10, O = 3, the built-in Kinova. The HIP path runs the same cases in
tests/test_gpu_domain_edges.py, which imports the checks and the measured table from here.

  * containment: the point models of tests/point_model.py lie in the oracle's sets on every shift and
    straddle case (tests/test_oracle_containment.containment, SLACK);
  * emulation: jobs t = 0 and t = T - 1 of those cases against the oracle, as tests/test_emu.py;
  * shift identity: turning the continuous joints by whole turns changes nothing but their position
    extremum rows, which move by 2 pi n; shifting only the goal changes nothing at all;
  * the limit, speed and far-goal plans are pinned to tests/golden/domain_edges.npz.

The identities hold to rounding only: cos / sin of an angle of magnitude 2 pi n carry its ulp, and the
solve amplifies 1e-11 in a row to 1e-7 in k. IDENTITY is the oracle's own shifted-against-unshifted
distance per n; every identity check, on the oracle and on the HIP path, allows ten times that
(different orders of summation).
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import emu  # noqa: E402

import domain_edges as DE  # noqa: E402
from oracle import OraclePlanner  # noqa: E402
from test_oracle_containment import SLACK, containment, kinova, oracle_sets  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T, O = DE.T, DE.O
XS = (np.zeros(7), np.linspace(-0.9, 0.9, 7))
MARGIN = 10.0

# The oracle's distances between shift(n) and the base world: link centres [m] and generators [m], torque
# radius [N m], rows of g (torque, collision, extremum; the continuous joints' position rows moved back by
# 2 pi n) and of the Jacobian at XS, k_opt and cost of the plan. Measured 2026-10-20 on the build
# container (x86-64, g++ -O2, oracle/ at this commit), T = 10, O = 3.
IDENTITY = {
    1: dict(centres=2.33e-15, gens=1.76e-15, tr=5.68e-14, rows=5.51e-14, jac=4.72e-16, k=4.24e-10, cost=3.76e-15),
    -1: dict(centres=1.50e-15, gens=1.90e-15, tr=4.62e-14, rows=5.68e-14, jac=4.44e-16, k=4.24e-10, cost=3.74e-15),
    7: dict(centres=1.28e-14, gens=1.42e-14, tr=3.98e-13, rows=1.01e-13, jac=3.09e-15, k=2.97e-09, cost=2.66e-14),
    -40: dict(centres=7.03e-14, gens=7.93e-14, tr=1.51e-12, rows=5.04e-13, jac=1.72e-14, k=1.81e-08, cost=1.58e-13),
    150: dict(centres=2.70e-13, gens=2.50e-13, tr=9.29e-12, rows=1.84e-12, jac=5.80e-14, k=5.88e-07, cost=5.05e-12),
}
# the same for goal_shift(n): the reach sets and every row do not see q_des (exactly equal); the wrapped
# cost does, through wrap_to_pi's one subtraction of 2 pi per turn
GOAL_IDENTITY = {
    1: dict(k=1.72e-14, cost=4.34e-19), -1: dict(k=1.52e-14, cost=8.85e-17), 7: dict(k=1.63e-13, cost=6.14e-16),
    -40: dict(k=6.55e-12, cost=2.28e-14), 150: dict(k=6.48e-11, cost=2.18e-13),
}


class OracleSets:
    """the quantities of the identity checks from an oracle planner (the HIP path's adapter is in
    tests/test_gpu_domain_edges.py)"""

    def __init__(self, world):
        self.R = OraclePlanner(*world, T=T, threads=4)
        self.R.reach()

    def gens(self):
        return self.R.link_gens()

    def torque_radius(self):
        return self.R.torque_radius()

    def eval(self, x):
        return self.R.eval(x, centers=True)   # g, J, centres

    def plan(self):
        return self.R.plan()


def identity_distances(base, other, n, goal_only=False):
    """distances of the quantities that a shift by n turns must leave alone (IDENTITY's keys)"""
    d = dict(gens=np.abs(other.gens() - base.gens()).max(), tr=np.abs(other.torque_radius() - base.torque_radius()).max(),
             centres=0.0, rows=0.0, jac=0.0)
    for x in XS:
        g, J, lc = other.eval(x)
        g0, J0, lc0 = base.eval(x)
        g = g.copy()
        if not goal_only:
            for off in (-28, -21):                      # min q and max q of the continuous joints
                g[[off + j for j in DE.CONT]] -= DE.TWO_PI * n
        d["centres"] = max(d["centres"], np.abs(lc - lc0).max())
        d["rows"] = max(d["rows"], np.abs(g - g0).max())
        d["jac"] = max(d["jac"], np.abs(J - J0).max())
    p, p0 = other.plan(), base.plan()
    assert p["feasible"] == p0["feasible"] and p["status"] == p0["status"] and p["iterations"] == p0["iterations"]
    d["k"] = np.abs(p["k_opt"] - p0["k_opt"]).max()
    d["cost"] = abs(p["cost"] - p0["cost"])
    return d


def check_identity(base, other, n, goal_only=False, report=print):
    d = identity_distances(base, other, n, goal_only)
    report(f"{'goal_shift' if goal_only else 'shift'}({n}): " + " ".join(f"{k}={v:.2e}" for k, v in d.items()))
    table = GOAL_IDENTITY[n] if goal_only else IDENTITY[n]
    for key, v in d.items():
        # a goal shift cannot reach the reach sets or the rows at all
        tol = MARGIN * table[key] if key in table else 0.0
        assert v <= tol, (n, key, v, tol)


@pytest.fixture(scope="module")
def base():
    return OracleSets(DE.base_world())


@pytest.mark.parametrize("n", DE.SHIFTS)
def test_oracle_shift_identity(base, n):
    check_identity(base, OracleSets(DE.shift(n)), n)


@pytest.mark.parametrize("n", DE.SHIFTS)
def test_oracle_goal_shift_gives_the_base_plan(base, n):
    check_identity(base, OracleSets(DE.goal_shift(n)), n, goal_only=True)


def test_oracle_sets_contain_point_models_at_multi_turn_and_branch_angles():
    robot = kinova()
    rng = np.random.default_rng(17)
    worst = [-np.inf, -np.inf]
    for name, world in DE.identity_cases():
        R = OraclePlanner(*world, T=T, threads=4)
        R.reach()
        for x in XS:
            lw, tw, _ = containment(robot, world, T, x, *oracle_sets(R, x), rng, n_t=3)
            worst = [max(worst[0], lw), max(worst[1], tw)]
            assert lw <= SLACK, f"{name}: link point outside its zonotope by {lw:.3e} m"
            assert tw <= SLACK, f"{name}: torque outside centre +- radius by {tw:.3e} N m"
    print(f"worst link excess {worst[0]:.3e} m, worst torque excess {worst[1]:.3e} N m")


def test_emulated_program_matches_oracle_at_multi_turn_and_branch_angles():
    """the comparison of tests/test_emu.py (same structure, values to rounding) on jobs t = 0 and
    t = T - 1 of every shift and straddle case"""
    for name, world in DE.identity_cases():
        P = OraclePlanner(*world, T=T, threads=4)
        P.reach()
        lg_o = P.get(0).reshape(T, 7, 18)
        tr_o = P.torque_radius()
        for t in (0, T - 1):
            o = emu.reach_job(world, T, t)
            assert o["err"] == 0, name
            np.testing.assert_allclose(o["link_gens"], lg_o[t], rtol=0, atol=1e-14, err_msg=name)
            np.testing.assert_allclose(o["torque_radius"], tr_o[t], rtol=0, atol=1e-12, err_msg=name)
            for l in range(7):
                pz = P.pz(0, l * T + t)
                n = o["link_cnt"][l]
                assert n == len(pz["hashes"]), name
                np.testing.assert_array_equal(o["link_hash"][l, :n], pz["hashes"], err_msg=name)
                np.testing.assert_allclose(o["link_coef"][l, :n], pz["coeffs"], rtol=0, atol=1e-14, err_msg=name)
                np.testing.assert_allclose(o["link_center"][l], pz["center"], rtol=0, atol=1e-14, err_msg=name)
                np.testing.assert_allclose(o["link_rad"][l], pz["indep"], rtol=0, atol=1e-14, err_msg=name)
            for j in range(7):
                pz = P.pz(1, j * T + t)
                n = o["tq_cnt"][j]
                assert n == len(pz["hashes"]), name
                np.testing.assert_array_equal(o["tq_hash"][j, :n], pz["hashes"], err_msg=name)
                np.testing.assert_allclose(o["tq_coef"][j, :n], pz["coeffs"][:, 0], rtol=0, atol=1e-13, err_msg=name)
                np.testing.assert_allclose(o["tq_center"][j], pz["center"][0], rtol=0, atol=1e-12, err_msg=name)
                np.testing.assert_allclose(o["tq_rad"][j], pz["indep"][0], rtol=0, atol=1e-12, err_msg=name)


def load_plans():
    return dict(np.load(os.path.join(GOLD, "domain_edges.npz")))


def test_oracle_reproduces_the_limit_speed_and_far_goal_plans():
    fx = load_plans()
    cases = DE.plan_cases()
    assert [n for n, _ in cases] == list(fx["names"])
    for w, (name, world) in enumerate(cases):
        for k, v in zip(("q0", "qd0", "qdd0", "q_des", "obstacles"), world):
            np.testing.assert_array_equal(v, fx[k][w], err_msg=f"{name} {k}")
        R = OraclePlanner(*world, T=T, threads=4)
        R.reach()
        r = R.plan()
        assert r["feasible"] == bool(fx["feasible"][w]) and r["status"] == int(fx["status"][w]), name
        assert r["iterations"] == int(fx["iterations"][w]) and r["evaluations"] == int(fx["evaluations"][w]), name
        np.testing.assert_allclose(r["k_opt"], fx["k_opt"][w], rtol=0, atol=1e-10, err_msg=name)
        np.testing.assert_allclose(r["cost"], fx["cost"][w], rtol=1e-9, atol=1e-13, err_msg=name)


def test_fixture_holds_what_the_issue_describes():
    """the families really end where they were built to end: the state-limit and speed-limit rows are
    active or infeasible, and the far goals put every plan's largest |k| on the box"""
    fx = load_plans()
    names = list(fx["names"])
    st = dict(zip(names, zip(fx["feasible"], fx["status"])))
    for n in names:
        feasible_family = n.startswith("far_") or n.endswith("ub+0.05") or n == "speed+0.8"
        assert st[n] == ((True, 0) if feasible_family else (False, 4)), (n, st[n])
    far = [i for i, n in enumerate(names) if n.startswith("far_")]
    assert np.all(np.abs(fx["k_opt"][far]).max(axis=1) > 0.9999)
    assert int(np.sum(fx["status"] == 4)) == 20
