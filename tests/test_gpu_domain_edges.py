"""HIP path on the edges of the input domain (tests/domain_edges.py; T = 10, O = 3, the built-in
Kinova), on every reach engine: multi-turn angles and starts on the branch points of cos / sin against a
fresh oracle at the project's bars, the point models and the shift identity; starts on and beyond the
position and speed limits and far goals against tests/golden/domain_edges.npz; the same batch through
the mixed entry and the candidate evaluation; and the one bad value that may reach a device, a NaN goal
of an unwrapped joint, refused by every entry.

Bars: reach outputs, g and J within 1e-9 of the oracle, collision decisions at 1e-4 and the
feasibility re-check identical, status and iterations identical, k_opt within 1e-8 — except at shifts
of -40 and 150 turns, where k_opt is held to ten times the oracle's own shifted-against-unshifted
distance (tests/test_domain_edges.IDENTITY: the solve amplifies 1e-11 in a row to 1e-7 in k).
"""
import numpy as np
import pytest

import armour_amd as A
import domain_edges as DE
from conftest import engine
from oracle import OraclePlanner
from paths import assert_paths, engine_paths
from test_domain_edges import IDENTITY, MARGIN, XS, check_identity, load_plans
from test_oracle_containment import SLACK, containment, kinova

pytestmark = pytest.mark.gpu
TOL = 1e-9
COL_THR = 1e-4
T, O = DE.T, DE.O
ENGINES = ["lane", "job", "narrow"]
COLLISION = slice(7 * T, 7 * T + 7 * T * O)


def k_tolerance(name):
    for n in (-40, 150):
        if name == f"shift{n:+d}":
            return MARGIN * IDENTITY[n]["k"]
    return 1e-8


@pytest.mark.parametrize("eng", ENGINES)
def test_multi_turn_and_branch_angles_against_the_oracle(eng):
    cases = DE.identity_cases() + DE.goal_shift_cases()
    worlds = [w for _, w in cases]
    with engine(eng):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=len(worlds))
    P.reach(worlds)
    refs = []
    for w, (name, world) in enumerate(cases):
        R = OraclePlanner(*world, T=T, threads=4)
        R.reach()
        refs.append(R)
        np.testing.assert_allclose(P.torque_radius(w), R.torque_radius(), rtol=0, atol=TOL, err_msg=name)
        np.testing.assert_allclose(P.link_generators(w), R.link_gens(), rtol=0, atol=TOL, err_msg=name)
        for x in XS:
            g, J = P.eval_constraints(w, x)
            go, Jo = R.eval(x)
            np.testing.assert_allclose(g, go, rtol=0, atol=TOL, err_msg=name)
            np.testing.assert_allclose(J, Jo, rtol=0, atol=TOL, err_msg=name)
            np.testing.assert_array_equal(g[COLLISION] > COL_THR, go[COLLISION] > COL_THR, err_msg=name)
            assert R.feasible(g) == R.feasible(go), name
    res, _ = P.plan(worlds)
    robot = kinova()
    rng = np.random.default_rng(23)
    worst = [-np.inf, -np.inf]
    for w, (name, world) in enumerate(cases):
        r, ro = res[w], refs[w].plan()
        assert r["feasible"] == ro["feasible"] and r["status"] == ro["status"], name
        assert r["iterations"] == ro["iterations"], (name, r["iterations"], ro["iterations"])
        dk = np.abs(r["k_opt"] - ro["k_opt"]).max()
        print(f"{eng} {name}: iterations {r['iterations']} |dk_opt| {dk:.2e} (allowed {k_tolerance(name):.1e})")
        assert dk <= k_tolerance(name), (name, dk)
        # the point models inside the sets at k_opt (tests/test_gpu_containment._check)
        g = P.constraints(w)
        lw, tw, _ = containment(robot, world, T, r["k_opt"], P.link_centers(w), P.link_generators(w),
                                g[:7 * T].reshape(T, 7), P.torque_radius(w), rng, n_t=3)
        worst = [max(worst[0], lw), max(worst[1], tw)]
        assert lw <= SLACK, f"{name}: a link point lies {lw:.3e} m outside its set"
        assert tw <= SLACK, f"{name}: a torque lies {tw:.3e} N m outside centre +- radius"
    print(f"{eng}: worst link excess {worst[0]:.3e} m, worst torque excess {worst[1]:.3e} N m")
    assert_paths(P.path_counts(), **engine_paths(eng))


class DeviceSets:
    """the quantities of tests/test_domain_edges.identity_distances from a one-world batch of planner P
    (every world takes the same place in its batch, so the engines' orders of summation are the same
    and only the shift separates two worlds); everything is read at construction"""

    def __init__(self, P, world):
        P.reach([world])
        self._gens, self._tr = P.link_generators(0), P.torque_radius(0)
        self._ev = []
        for x in XS:
            g, J = P.eval_constraints(0, x)
            self._ev.append((g, J, P.link_centers(0)))
        res, _ = P.plan([world])
        self._plan = res[0]

    def gens(self):
        return self._gens

    def torque_radius(self):
        return self._tr

    def eval(self, x):
        return self._ev[[i for i, v in enumerate(XS) if v is x][0]]

    def plan(self):
        return self._plan


@pytest.mark.parametrize("eng", ENGINES)
def test_shift_identity_on_the_device(eng):
    """free of the oracle: whole turns of the continuous joints move nothing but their position
    extremum rows, and whole turns of the goal move nothing at all, within ten times the distances
    the oracle itself shows"""
    with engine(eng):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=1)
    base = DeviceSets(P, DE.base_world())
    for n in DE.SHIFTS:
        check_identity(base, DeviceSets(P, DE.shift(n)), n, report=lambda s: print(eng, s))
    for n in DE.SHIFTS:
        check_identity(base, DeviceSets(P, DE.goal_shift(n)), n, goal_only=True, report=lambda s: print(eng, s))
    assert_paths(P.path_counts(), **engine_paths(eng))


def _extremum_violation(P, g):
    jb = P.joint_bounds()   # per joint [L, U] of its position rows, then of its velocity rows
    Lx = np.concatenate([jb[0:14:2], jb[0:14:2], jb[14:28:2], jb[14:28:2]])
    Ux = np.concatenate([jb[1:14:2], jb[1:14:2], jb[15:28:2], jb[15:28:2]])
    return np.maximum(Lx - g[-28:], g[-28:] - Ux).max()


@pytest.mark.parametrize("eng", ENGINES)
def test_limits_speeds_and_far_goals(eng):
    """one mixed-status batch against the fixture. A world that ends in local infeasibility (status 4)
    follows the rule of tests/test_gpu_boundary.py: verdict and status equal, the iteration count within
    5 of the oracle's, k_opt (where the restoration phase stalled) not compared; and the oracle, given
    the device's last iterate, evaluates the same rows and reaches the same verdict."""
    fx = load_plans()
    cases = DE.plan_cases()
    names = [n for n, _ in cases]
    assert names == list(fx["names"])
    worlds = [w for _, w in cases]
    W = len(worlds)
    with engine(eng):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    res, _ = P.plan(worlds)
    g_opt = [P.constraints(w) for w in range(W)]
    stalled = 0
    for w, name in enumerate(names):
        r = res[w]
        assert r["error"] == 0, name
        assert r["feasible"] == bool(fx["feasible"][w]) and r["status"] == int(fx["status"][w]), \
            (name, r["feasible"], r["status"])
        dk = np.abs(r["k_opt"] - fx["k_opt"][w]).max()
        print(f"{eng} {name}: feasible={r['feasible']} status={r['status']} iterations={r['iterations']} "
              f"(fixture {int(fx['iterations'][w])}) |dk_opt|={dk:.1e}")
        if r["status"] == 4:
            stalled += 1
            assert not r["feasible"], name
            assert abs(r["iterations"] - int(fx["iterations"][w])) <= 5, (name, r["iterations"])
            R = OraclePlanner(*worlds[w], T=T, threads=4)
            R.reach()
            go = R.eval(r["k_opt"], jac=False)
            np.testing.assert_allclose(g_opt[w], go, rtol=0, atol=TOL, err_msg=name)
            assert not R.feasible(go) and not R.feasible(g_opt[w]), name
        else:
            assert r["iterations"] == int(fx["iterations"][w]), (name, r["iterations"])
            assert dk <= 1e-8, (name, dk)
            np.testing.assert_allclose(r["cost"], fx["cost"][w], rtol=1e-8, atol=1e-12, err_msg=name)
    assert stalled == int(np.sum(fx["status"] == 4)) and stalled >= 20

    # the same batch through the mixed entry: bitwise the uniform plan
    res_m, _ = P.plan_mixed(worlds)
    for w, name in enumerate(names):
        a, b = res[w], res_m[w]
        assert a["k_opt"].tobytes() == b["k_opt"].tobytes(), name
        assert (a["feasible"], a["status"], a["iterations"], a["evaluations"]) == \
               (b["feasible"], b["status"], b["iterations"], b["evaluations"]), name
        assert np.float64(a["cost"]).tobytes() == np.float64(b["cost"]).tobytes(), name
        assert P.constraints(w).tobytes() == g_opt[w].tobytes(), name

    # candidates: every world's k_opt and the corners x = +1 and x = -1
    X = np.stack([np.stack([res[w]["k_opt"], np.ones(7), -np.ones(7)]) for w in range(W)])
    out = P.eval_candidates(X)
    for w, name in enumerate(names):
        for c in range(3):
            g = P.eval_constraints(w, X[w, c], jac=False)
            want = _extremum_violation(P, g)
            assert np.float64(out["violation"][w, c, 2]).tobytes() == np.float64(want).tobytes(), (name, c)
            assert out["feasible"][w, c] == bool((out["violation"][w, c] <= 0).all()), (name, c)
            if out["feasible"][w, c]:
                assert want <= 0
        # a start inside the tracking error of a position limit, or at a speed the limit less the
        # tracking error forbids, violates an extremum row whatever k is (the row includes t = 0)
        forced = (name.startswith("limit") and not name.endswith("ub+0.05")) or \
                 (name.startswith("speed") and name not in ("speed+0.8", "speed+0.9"))
        if forced:
            assert (out["violation"][w, :, 2] > 0).all() and not out["feasible"][w].any(), name
        assert out["feasible"][w, 0] == res[w]["feasible"], name
    assert_paths(P.path_counts(), **engine_paths(eng))


def _armtd_world(q_des_1):
    b = DE.base_world()
    tab = np.zeros((7, 6, T))
    tab[:, 0] = 1.0
    q_des = b[3].copy()
    q_des[1] = q_des_1
    return (b[0], b[1], q_des, tab, np.full(7, np.pi / 72), b[4])


def test_nan_goal_refused_by_every_entry_and_the_planner_stays_clean():
    """q_des[1] = NaN: joint 1 is not wrapped and q_des enters the cost and its gradient only, so this
    value cannot loop even on a build without the check. Every entry refuses it with ARMOUR_E_ARG
    before anything is launched, and the planner then plans a clean batch bitwise as a fresh one."""
    b = DE.base_world()
    q_des = b[3].copy()
    q_des[1] = np.nan
    bad = (b[0], b[1], b[2], q_des, b[4])
    assert "q_des[1]" in A.check_world(bad, O)   # the host check first
    clean = [DE.base_world(), DE.shift(1), DE.straddle(0.5, False)]
    P = A.Planner(T=T, max_obstacles=O, max_worlds=3)
    batch = [clean[0], bad, clean[2]]
    for call in (lambda: P.plan(batch), lambda: P.plan_mixed(batch), lambda: P.reach(batch),
                 lambda: P.reach_mixed(batch), lambda: P.plan_one(bad)):
        with pytest.raises(A.ArmourError, match=r"armour error -1: q_des\[1\] is not finite"):
            call()
    Pa = A.ArmtdPlanner(T=T, max_obstacles=O, max_worlds=1)
    for call in (lambda: Pa.plan([_armtd_world(np.nan)]), lambda: Pa.reach([_armtd_world(np.nan)])):
        with pytest.raises(A.ArmourError, match=r"armour error -1: q_des\[1\] is not finite"):
            call()
    res, _ = P.plan(clean)
    F = A.Planner(T=T, max_obstacles=O, max_worlds=3)
    ref, _ = F.plan(clean)
    for w in range(3):
        assert res[w]["k_opt"].tobytes() == ref[w]["k_opt"].tobytes()
        assert (res[w]["feasible"], res[w]["status"], res[w]["iterations"]) == \
               (ref[w]["feasible"], ref[w]["status"], ref[w]["iterations"])
        assert P.constraints(w).tobytes() == F.constraints(w).tobytes()
