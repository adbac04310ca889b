"""The roadmap model (tests/roadmap_model.py) pinned from outside itself, on the CPU, on the fixture
tests/golden/roadmap_worlds.npz (tests/golden/make_roadmap_worlds.py):

  * togo against scipy.sparse.csgraph.dijkstra on the model's own adjacency and weights, relative 1e-12;
  * a subsample of the edges the model accepts, every interior sample recomputed through
    collision_model.intersects_lp: no link box meets an obstacle grown by margin / sqrt(3) per side (a box
    inside the obstacle's margin-neighbourhood, which a separation above the margin keeps clear);
  * next strictly decreases togo and follows an existing edge;
  * the walk's q_des lies on the polyline q -> entry -> next -> ... -> goal at arc length
    min(lookahead, path_left), 1e-12;
  * an oracle-driven episode of the blocked world (world 4: a slab across the straight joint-space line) at
    T = 20: with the straight-line waypoint it is still short of its goal at the step cap, parked in front
    of the slab; with the model's roadmap waypoint it reaches the goal with positive clearance. Measured
    here: straight line 1.20 rad from the goal after 70 steps; roadmap: status 1 after 40 steps (STEPS_ROADMAP), clearance 0.039 m.
"""
import os

import numpy as np
import pytest

import collision_model as C
import episode_model as E
import roadmap_model as R

HERE = os.path.dirname(os.path.abspath(__file__))
STEP_CAP = 70
STEPS_ROADMAP = 40  # the roadmap episode's steps to the goal, established on the CPU (test_blocked_world_episode)


@pytest.fixture(scope="module")
def fx():
    return np.load(os.path.join(HERE, "golden", "roadmap_worlds.npz"))


@pytest.fixture(scope="module")
def robot():
    return E.kinova()


_models = {}


def model(fx, robot, w):
    if w not in _models:
        radius, step, margin, _ = fx["config"]
        _models[w] = R.build(robot, fx["nodes"][w], fx["goals"][w], fx["obstacles"][w][:fx["counts"][w]], radius, step, margin)
    return _models[w]


def test_fixture_holds_what_the_tests_need(fx, robot):
    assert tuple(fx["counts"]) == (3, 0, 6, 2, 1) and fx["nodes"].shape == (5, 100, 7) and fx["big_nodes"].shape == (1023, 7)
    assert np.array_equal(fx["nodes"][0][3], fx["nodes"][0][7])
    rm = model(fx, robot, 0)
    assert not rm["is_free"][5] and rm["clearance"][5] < 0 and rm["weight"][3, 7] == np.inf
    rm = model(fx, robot, 3)
    assert not rm["is_free"][100] and np.all(np.isinf(rm["togo"])) and np.all(rm["next"] == -1)
    rm = model(fx, robot, 2)
    assert np.any(rm["is_free"] & np.isinf(rm["togo"])) and np.any(np.isfinite(rm["togo"][:-1]))


@pytest.mark.parametrize("w", [0, 2, 4])
def test_togo_is_the_shortest_path(fx, robot, w):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import dijkstra

    rm = model(fx, robot, w)
    V = rm["verts"].shape[0]
    Wt = np.where(np.isfinite(rm["weight"]), rm["weight"], 0.0)
    ref = dijkstra(csr_matrix(Wt), directed=False, indices=V - 1)
    assert np.array_equal(np.isinf(ref), np.isinf(rm["togo"]))
    fin = np.isfinite(ref)
    np.testing.assert_allclose(rm["togo"][fin], ref[fin], rtol=1e-12, atol=0)
    # next strictly decreases togo along an existing edge, and attains the minimum
    for i in np.flatnonzero(fin[:-1]):
        j = rm["next"][i]
        assert np.isfinite(rm["weight"][i, j]) and rm["togo"][j] < rm["togo"][i]
        assert rm["weight"][i, j] + rm["togo"][j] == rm["togo"][i]
    assert rm["next"][V - 1] == V - 1 and np.all(rm["next"][~fin] == -1)
    # the adjacency words say what the weights say
    bits = (rm["adjacency"][:, :, None] >> np.arange(32, dtype=np.uint32)) & 1
    assert np.array_equal(bits.reshape(V, -1)[:, :V].astype(bool), np.isfinite(rm["weight"]))


@pytest.mark.parametrize("w", [0, 4])
def test_accepted_edges_are_free_by_the_exact_test(fx, robot, w):
    rm = model(fx, robot, w)
    margin = rm["margin"]
    rng = np.random.default_rng(11)
    cand = rm["cand"]
    long_ones = np.flatnonzero(rm["exists"] & (cand["n"] > 2))
    tested = 0
    for e in rng.choice(long_ones, 6, replace=False):
        i, j, n = cand["i"][e], cand["j"][e], int(cand["n"][e])
        assert np.all(rm["sample_clearance"][e] > margin)
        dl, _ = R.delta(robot, rm["verts"][i], rm["verts"][j])
        pts = R.segment_samples(rm["verts"][i], dl, n)
        c, G = E.link_boxes(robot, pts[rng.choice(len(pts), min(3, len(pts)), replace=False)])
        for s in range(c.shape[0]):
            for l in range(c.shape[1]):
                for ob in rm["obstacles"]:
                    Gob = ob[3:].reshape(3, 3).copy()
                    Gob += np.sign(Gob) * (margin / np.sqrt(3.0)) * (np.abs(Gob) == np.abs(Gob).max(1, keepdims=True))
                    assert C.intersects_lp(c[s, l], ob[:3], np.concatenate([Gob, G[s, l]])) < -1e-8
                    tested += 1
    assert tested >= 50


def on_polyline(pts, s):
    """the point at arc length s along the polyline pts [K, 7] (clamped to its end)"""
    for a, b in zip(pts[:-1], pts[1:]):
        d = float(np.sqrt(np.sum((b - a) ** 2)))
        if s <= d:
            return a + (s / d) * (b - a) if d > 0 else a
        s -= d
    return pts[-1]


@pytest.mark.parametrize("w", [0, 1, 2, 4])
def test_waypoint_lies_on_the_path(fx, robot, w):
    rm = model(fx, robot, w)
    lookahead = float(fx["config"][3])
    V = rm["verts"].shape[0]
    entries = 0
    for q in fx["queries"][w]:
        q_des, entry, left = R.waypoint(rm, q, lookahead)
        if entry < 0:
            np.testing.assert_array_equal(q_des, E.waypoint(robot, q, rm["verts"][V - 1], lookahead))
            assert left == np.inf
            continue
        entries += 1
        # the polyline in unwrapped coordinates: q plus the legs' Deltas
        pts, a, cur = [q.copy()], q, entry
        while True:
            pts.append(pts[-1] + R.delta(robot, a, rm["verts"][cur])[0])
            if cur == V - 1:
                break
            a, cur = rm["verts"][cur], rm["next"][cur]
        length = sum(float(np.linalg.norm(b - a)) for a, b in zip(pts[:-1], pts[1:]))
        assert abs(length - left) <= 1e-12 * max(1.0, left)
        np.testing.assert_allclose(q_des, on_polyline(np.array(pts), min(lookahead, left)), rtol=0, atol=1e-12)
    assert entries >= 16


def test_blocked_world_episode(fx, robot):
    w = 4
    obs = fx["obstacles"][w][:fx["counts"][w]]
    world = (fx["q0"][w], np.zeros(7), np.zeros(7), fx["q0"][w].copy(), obs)
    goal = fx["goals"][w]
    line = R.clearance(robot, world[0] + np.linspace(0, 1, 41)[:, None] * (goal - world[0]), obs)
    assert line.min() < 0 < min(line[0], line[-1])   # the slab lies across the straight line
    st = R.oracle_episode(robot, world, goal, None, STEP_CAP)
    print(f"straight line: status {st['status']}, {st['steps']} steps, {st['goal_distance']:.3f} rad from the goal")
    assert st["status"] == 0 and st["steps"] == STEP_CAP and st["goal_distance"] > 1.0
    st = R.oracle_episode(robot, world, goal, model(fx, robot, w), STEP_CAP)
    print(f"roadmap: status {st['status']}, {st['steps']} steps, clearance {st['clearance']:.4f}")
    assert st["status"] == 1 and st["clearance"] > 0
    assert st["steps"] == STEPS_ROADMAP
