"""armour_check_motion on the GPU against the numpy model (tests/episode_model.py).

Setup: T = 20, saved worlds 0-7 in one mixed batch (5-10 obstacles), a uniform batch of the general
zonotope obstacles of tests/golden/zonotope_worlds.npz (flat, point, sheared, rotated, parallel,
1e3 m ... kinds; 20 and 40 obstacles), a world without obstacles, a reversed-axis and a 9-joint robot.
Trajectories: the plans' own k_opt, k = +-1, and trajectories found with the model to pass through
an obstacle (negative clearance).

The rounding bound. A separation is |n . (c - c_obs)| - sum_j |n . G_j| on unit normals n: about 40
operations on quantities bounded by |c - c_obs|_1 + sum_j |G_j|_1, for which
collision_model.rounding_bound takes 256 eps of that sum. Here c and the link's G_j also come from
forward kinematics on both sides (device: host-built RPY matrices, device sin / cos, products in
chain order; model: numpy), so episode_model.fk_bound adds a term of the same form over the arm's
offsets: 256 eps L for the chain of up to 9 rotations (L = sum |trans_i|_1 + the link box, about 1.5 m)
and 16 eps L sum_j (|q0| + |qd0| + |qdd0| + |k| k_range) for the joint angles of the Bezier curve.
Together about 1e-13 .. 3e-13 m on the saved worlds (1.7e-10 m against the 1e3 m obstacle, whose
generators enter the sum). The minimum of values that each agree within the bound agrees within the
largest bound of the window, which is what the test uses.

Assertions: |clearance - model| <= bound; the sign is the model's and no case lies within the bound
of 0; `where` is the model's wherever its runner-up is farther than the bound. One refinement: where
an obstacle generator and a link generator are parallel to rounding (the base link's z generator
against an upright box), their cross product is an arbitrary unit vector that depends on the last
bit of the forward kinematics; any unit vector is a valid axis, so there the device may lie above
the model's regular-plane value but never more than the bound below it. Cases whose minimiser is
such a pair are held to that floor and to the sign, and must stay under a tenth of all cases.
A rounding-level cross product with a single non-zero component is no such pair: it normalises to a
coordinate axis exactly (episode_model.separations).

Measured on the MI355X: 160 cases on the saved worlds, none on a fragile pair, the largest
|clearance - model| 1.1e-3 of the bound (about 3e-16 m), `where` equal in every case.
"""
import os

import numpy as np
import pytest

import armour_amd as A
import episode_model as E
import robot_variants as RV
import test_zonotope_obstacles as Z
from test_episode_model import saved

pytestmark = pytest.mark.gpu

T = 20
SAMPLES = 11


def colliding_trajectory(robot, world, rng, tries=400):
    """a trajectory from a random state whose model clearance against the world's obstacles is below -1 mm"""
    lb = np.where(robot["state_lb"] < -100, -np.pi, robot["state_lb"])
    ub = np.where(robot["state_ub"] > 100, np.pi, robot["state_ub"])
    for _ in range(tries):
        traj = (rng.uniform(lb, ub), rng.uniform(-0.5, 0.5, 7), rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7))
        q, _, _ = E.trajectory(traj, E.sample_times(0, 1, 3))
        c, G = E.link_boxes(robot, q)
        if E.separation(c[:, :, None, :], G[:, :, None], world[4][None, None]).min() < -1e-3:
            return traj
    raise RuntimeError("no colliding trajectory found")


def compare(P, robot, worlds, trajs, t0, t1, samples, tag):
    """the assertions of the module docstring for one call; returns (cases, fragile cases, worst error / bound)"""
    clear, where = P.check_motion(np.array([np.stack(t) for t in trajs]), t0, t1, samples)
    fragile = 0
    worst = 0.0
    for w, (world, traj) in enumerate(zip(worlds, trajs)):
        m = E.clearance(robot, traj, world[4], t0, t1, samples)
        if len(world[4]) == 0:
            assert clear[w] == np.inf and tuple(where[w]) == (-1, -1, -1), (tag, w)
            continue
        b = m["bound"]
        print(f"{tag} world {w}: device {clear[w]:+.6e} model {m['clearance']:+.6e} diff {clear[w] - m['clearance']:+.2e} "
              f"bound {b:.2e} where {tuple(where[w])} / {m['where']} fragile {m['fragile']}")
        assert abs(m["clearance"]) > b and abs(m["floor"]) > b, (tag, w, "a case inside the bound of 0")
        if m["fragile"]:
            fragile += 1
            assert clear[w] >= m["floor"] - b and (clear[w] > 0) == (m["floor"] > 0), (tag, w)
            continue
        assert abs(clear[w] - m["clearance"]) <= b, (tag, w, clear[w], m["clearance"], b)
        worst = max(worst, abs(clear[w] - m["clearance"]) / b)
        assert (clear[w] > 0) == (m["clearance"] > 0), (tag, w)
        if m["runner_up"] > b:
            assert tuple(where[w]) == m["where"], (tag, w, where[w], m["where"])
    return len(worlds), fragile, worst


@pytest.fixture(scope="module")
def batch():
    """saved worlds 0-7 planned in one mixed batch, once; the trajectories of every test on it"""
    robot = E.kinova()
    worlds = [saved(i)[0] for i in range(8)]
    counts = [len(w[4]) for w in worlds]
    assert min(counts) == 5 and max(counts) == 10
    P = A.Planner(T=T, max_obstacles=max(counts), max_worlds=8)
    res, _ = P.plan_mixed(worlds)
    rng = np.random.default_rng(7)
    z = np.zeros(7)
    trajs = dict(k_opt=[(w[0], z, z, r["k_opt"]) for w, r in zip(worlds, res)],
                 plus=[(w[0], z, z, np.ones(7)) for w in worlds], minus=[(w[0], z, z, -np.ones(7)) for w in worlds],
                 moving=[(w[0], rng.uniform(-0.5, 0.5, 7), rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7)) for w in worlds],
                 into=[colliding_trajectory(robot, w, rng) for w in worlds])
    yield dict(P=P, robot=robot, worlds=worlds, res=res, trajs=trajs)
    P.close()


def test_mixed_batch_against_model(batch):
    P, robot, worlds = batch["P"], batch["robot"], batch["worlds"]
    cases = fragile = 0
    worst = 0.0
    for name, trajs in batch["trajs"].items():
        for t0, t1, s in ((0.0, 1.0, SAMPLES), (0.0, 0.5, SAMPLES), (0.5, 1.0, 4), (0.25, 0.25, 1)):
            n, f, e = compare(P, robot, worlds, trajs, t0, t1, s, f"{name} [{t0}, {t1}] x {s}")
            cases, fragile, worst = cases + n, fragile + f, max(worst, e)
    clear, _ = P.check_motion(np.array([np.stack(t) for t in batch["trajs"]["into"]]), 0.0, 1.0, SAMPLES)
    assert np.all(clear < -1e-3 + 1e-9)   # (the model found them on 3 of these samples' times)
    clear, _ = P.check_motion(np.array([np.stack(t) for t in batch["trajs"]["k_opt"]]), 0.0, 1.0, SAMPLES)
    feas = np.array([r["feasible"] for r in batch["res"]])
    assert feas.any() and np.all(clear[feas] > 0)   # a feasible plan misses the obstacles
    print(f"{cases} cases, {fragile} on a fragile pair, worst error {worst:.3g} bounds")
    assert fragile <= cases // 10


def test_samples_chunking(batch):
    """[0, 0.5] with 11 samples is the minimum of the eleven 1-sample calls, first minimiser included"""
    P = batch["P"]
    for name in ("k_opt", "moving", "into"):
        traj = np.array([np.stack(t) for t in batch["trajs"][name]])
        clear, where = P.check_motion(traj, 0.0, 0.5, SAMPLES)
        singles = [P.check_motion(traj, t, t, 1) for t in np.linspace(0.0, 0.5, SAMPLES)]
        cs = np.array([c for c, _ in singles])             # [S, W]
        first = np.argmin(cs, axis=0)
        np.testing.assert_array_equal(clear, cs.min(axis=0))
        np.testing.assert_array_equal(where[:, 0], first)
        for w in range(len(clear)):
            assert np.all(singles[first[w]][1][w] == [0, where[w, 1], where[w, 2]])


@pytest.mark.parametrize("samples", [64, 65, 130])
def test_samples_chunking_past_one_wave(batch, samples):
    """the same identity with a full wave of samples, one more, and a third trip of the finish kernel's
    lane-strided loop: clearance and first minimiser are those of the single-sample calls, exactly"""
    P = batch["P"]
    traj = np.array([np.stack(t) for t in batch["trajs"]["moving"]])
    clear, where = P.check_motion(traj, 0.0, 1.0, samples)
    singles = [P.check_motion(traj, t, t, 1) for t in E.sample_times(0.0, 1.0, samples)]
    cs = np.array([c for c, _ in singles])                 # [S, W]
    first = np.argmin(cs, axis=0)
    print(samples, "first minimisers", first.tolist())
    np.testing.assert_array_equal(clear, cs.min(axis=0))
    np.testing.assert_array_equal(where[:, 0], first)
    for w in range(len(clear)):
        assert np.all(singles[first[w]][1][w] == [0, where[w, 1], where[w, 2]])


def test_a_trajectory_at_rest_ties_in_every_sample(batch):
    """qd0 = qdd0 = 0 and k = 0 at q0 = 0: all 130 samples are the same configuration bit for bit, a tie
    across the lanes and the trips of the finish kernel, which the lowest sample wins. (At another q0 the
    Bernstein sum of six equal control points rounds differently from sample to sample; at 0 every term
    is 0, so the tie is exact.)"""
    P = batch["P"]
    traj = np.zeros((len(batch["worlds"]), 4, 7))
    clear, where = P.check_motion(traj, 0.0, 1.0, 130)
    one, where1 = P.check_motion(traj, 0.0, 0.0, 1)
    assert np.all(where[:, 0] == 0)
    np.testing.assert_array_equal(clear, one)
    np.testing.assert_array_equal(where, where1)


def test_state_is_undisturbed(batch):
    """the getters and the next plan are bitwise what they were"""
    P, worlds = batch["P"], batch["worlds"]
    res, _ = P.plan_mixed(worlds)
    before = [(P.constraints(w), P.link_centers(w), P.torque_radius(w)) for w in (0, 5)]
    P.check_motion(np.array([np.stack(t) for t in batch["trajs"]["into"]]), 0.0, 1.0, 23)
    P.check_motion(np.array([np.stack(t) for t in batch["trajs"]["plus"]]), 0.2, 0.9, 5)
    after = [(P.constraints(w), P.link_centers(w), P.torque_radius(w)) for w in (0, 5)]
    for b, a in zip(before, after):
        for x, y in zip(b, a):
            assert np.array_equal(x, y)
    res2, _ = P.plan_mixed(worlds)
    for r, r2 in zip(res, res2):
        assert np.array_equal(r["k_opt"], r2["k_opt"]) and r["cost"] == r2["cost"] and r["iterations"] == r2["iterations"]
        assert r["feasible"] == r2["feasible"] and r["kkt"] == r2["kkt"]


@pytest.mark.parametrize("name", ["kinova0", "kinova_small"])
def test_general_zonotope_obstacles_uniform_batch(name):
    """flat, point, sheared ... obstacles (20 and 40 per world) in a uniform batch, after a reach entry only"""
    cs = Z.case(name)
    robot = E.kinova()
    kinds = set(cs["kinds"].tolist())
    assert {"plate", "floor", "point", "sheared"} <= kinds
    world = cs["world"]
    worlds = [world, (world[0] + 0.3, world[1], world[2], world[3], world[4])]
    P = A.Planner(T=cs["T"], max_obstacles=cs["O"], max_worlds=2)
    P.reach(worlds)
    rng = np.random.default_rng(11)
    cases = fragile = 0
    for k in range(3):
        trajs = [(w[0], rng.uniform(-0.5, 0.5, 7), rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7)) for w in worlds]
        n, f, _ = compare(P, robot, worlds, trajs, 0.0, 1.0, 7, f"{name} draw {k}")
        cases, fragile = cases + n, fragile + f
    assert fragile <= cases // 2   # (upright plates and boxes meet the base link here more often)
    P.close()


def test_obstacle_kinds_one_world_each():
    """the fixture's obstacles grouped by kind, one world per group (a mixed batch), so that each kind
    holds the minimum somewhere: flat (plate, floor), point, sheared, rotated and rod, the rest"""
    cs = Z.case("kinova0")
    robot = E.kinova()
    world, kinds = cs["world"], cs["kinds"]
    groups = [("plate", "floor"), ("point",), ("sheared",), ("rotated", "rod"), ("parallel", "near_parallel", "dup", "negperm", "tiny")]
    worlds = [(world[0], world[1], world[2], world[3], world[4][np.isin(kinds, g)]) for g in groups]
    assert all(len(w[4]) > 0 for w in worlds)
    P = A.Planner(T=cs["T"], max_obstacles=cs["O"], max_worlds=len(worlds))
    P.reach_mixed(worlds)
    rng = np.random.default_rng(13)
    cases = fragile = 0
    for k in range(3):
        trajs = [(w[0], rng.uniform(-0.5, 0.5, 7), rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7)) for w in worlds]
        n, f, _ = compare(P, robot, worlds, trajs, 0.0, 1.0, 7, f"kinds draw {k}")
        cases, fragile = cases + n, fragile + f
    assert fragile <= cases // 2
    P.close()


def test_world_without_obstacles():
    worlds = [A.make_world(3, 0), A.make_world(4, 2), A.make_world(5, 0)]
    P = A.Planner(T=10, max_obstacles=2, max_worlds=3)
    P.reach_mixed(worlds)
    z = np.zeros(7)
    trajs = [(w[0], w[1], w[2], z) for w in worlds]
    compare(P, E.kinova(), worlds, trajs, 0.0, 1.0, 5, "no obstacles")
    clear, where = P.check_motion(np.array([np.stack(t) for t in trajs]), 0.0, 1.0, 5)
    assert clear[0] == np.inf and clear[2] == np.inf and np.isfinite(clear[1])
    assert np.all(where[[0, 2]] == -1) and np.all(where[1] >= 0)
    P.close()
    # a uniform batch of worlds without obstacles
    P = A.Planner(T=10, max_obstacles=0, max_worlds=2)
    P.reach([worlds[0], worlds[2]])
    clear, where = P.check_motion(np.array([np.stack(t) for t in (trajs[0], trajs[2])]), 0.0, 1.0, 5)
    assert np.all(clear == np.inf) and np.all(where == -1)
    P.close()


@pytest.mark.parametrize("name", ["KINOVA_REV", "KINOVA_9"])
def test_robot_variants(name):
    """a reversed-axis robot and the 9-joint robot: the kernel reads the planner's tables"""
    tables = RV.variant(name)
    worlds = [A.make_world(s, 4) for s in (21, 22)]
    P = A.Planner(T=10, max_obstacles=4, max_worlds=2, robot=tables)
    P.reach(worlds)
    rng = np.random.default_rng(5)
    trajs = [(w[0], w[1], w[2], rng.uniform(-1, 1, 7)) for w in worlds]
    n, f, worst = compare(P, tables, worlds, trajs, 0.0, 1.0, 9, name)
    _, where = P.check_motion(np.array([np.stack(t) for t in trajs]), 0.0, 1.0, 9)
    assert np.all(where[:, 1] < int(tables["num_joints"]))
    if name == "KINOVA_REV":
        # the mirror identity: the reversed robot at the mirrored trajectory is the base robot
        S = RV.SPECS[name][2]
        s = RV.sigma(S)
        Pb = A.Planner(T=10, max_obstacles=4, max_worlds=2)
        Pb.reach([RV.mirror_world(w, S) for w in worlds])
        cb, wb = Pb.check_motion(np.array([np.stack([s * v for v in t]) for t in trajs]), 0.0, 1.0, 9)
        ca, wa = P.check_motion(np.array([np.stack(t) for t in trajs]), 0.0, 1.0, 9)
        np.testing.assert_allclose(ca, cb, rtol=0, atol=1e-12)
        Pb.close()
    P.close()


def test_errors(batch):
    P = batch["P"]
    traj = np.array([np.stack(t) for t in batch["trajs"]["k_opt"]])
    ok = lambda t=traj, a=0.0, b=1.0, s=3: A.lib().armour_check_motion(P.h, A._ptr(np.ascontiguousarray(t)), a, b, s, None, None)  # noqa: E731
    assert ok() == 0   # (both outputs are optional)
    assert A.lib().armour_check_motion(P.h, None, 0.0, 1.0, 3, None, None) == A.ARMOUR_E_ARG
    for bad in (np.nan, np.inf, -np.inf):
        for field in range(4):
            t = traj.copy()
            t[3, field, 2] = bad
            assert ok(t) == A.ARMOUR_E_ARG, (bad, field)
    for k in (1.0 + 1e-12, -1.5):
        t = traj.copy()
        t[7, 3, 6] = k
        assert ok(t) == A.ARMOUR_E_ARG
    t = traj.copy()
    t[0, 3, :] = [1, -1, 1, -1, 1, -1, 1]
    assert ok(t) == 0
    assert ok(s=0) == A.ARMOUR_E_ARG and ok(s=-3) == A.ARMOUR_E_ARG
    assert ok(a=0.6, b=0.5) == A.ARMOUR_E_ARG
    assert ok(a=-0.1) == A.ARMOUR_E_ARG and ok(b=1.0 + 1e-9) == A.ARMOUR_E_ARG
    assert ok(a=np.nan) == A.ARMOUR_E_ARG and ok(b=np.nan) == A.ARMOUR_E_ARG
    assert ok(a=0.5, b=0.5, s=4) == 0
    with pytest.raises(A.ArmourError, match="window"):
        P.check_motion(traj, 0.7, 0.2, 3)
    # before any batch
    Q = A.Planner(T=10, max_obstacles=2, max_worlds=8)
    assert A.lib().armour_check_motion(Q.h, A._ptr(traj), 0.0, 1.0, 3, None, None) == A.ARMOUR_E_STATE
    Q.close()


def test_fp32_study_refused():
    os.environ["ARMOUR_EVAL_F32"] = "1"
    try:
        P = A.Planner(T=10, max_obstacles=2, max_worlds=1)
    finally:
        os.environ.pop("ARMOUR_EVAL_F32", None)
    w = A.make_world(1, 2)
    P.reach([w])
    P._W = 1
    with pytest.raises(A.ArmourError, match="fp32"):
        P.check_motion(np.zeros((1, 4, 7)), 0.0, 1.0, 3)
    P.close()


def test_armtd_refused():
    P = A.ArmtdPlanner(T=10, max_obstacles=2, max_worlds=1)
    P._W = 1
    with pytest.raises(A.ArmourError, match="ARMTD"):
        P.check_motion(np.zeros((1, 4, 7)), 0.0, 1.0, 3)
    P.close()
