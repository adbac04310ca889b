"""The roadmap high-level planner on the GPU (armour_roadmap_*, armour_episode_roadmap) against the numpy model
(tests/roadmap_model.py) on the fixture tests/golden/roadmap_worlds.npz (its generator holds the guard bands
that make the decisions comparable exactly). T = 20, the five fixture worlds as one mixed batch (3, 0, 6, 2, 1
obstacles), N = 100, connect_radius 1.0, edge_step 0.05, margin 0.02.

Build: is_free, the adjacency words, next and the stats' counts equal the model's; node clearances within the
bound test_gpu_check_motion.py holds the device to (episode_model.clearance's rounding + FK bound); togo at
rtol 1e-13 with identical infinity patterns; node clearances bitwise armour_check_motion's for the constant
trajectories; two builds give bitwise the same getters; the N = 1023 set matches the model's recorded is_free
and counts; the plan's getters and the next plan are bitwise unchanged by a build; plan() after a build makes
the getters return ARMOUR_E_STATE; the argument errors name their fields.
Waypoint: 32 query points per world (on a node, mid-edge, out of reach: the fallback, bitwise episode_begin's
straight-line q_des; next to the goal: the clamp): the entry is the model's, q_des within
64 eps (|q| + lookahead) per joint, path_left at rtol 1e-13.
Episodes: with episode_roadmap each step's results are bitwise plan_mixed of the states read before the step on
a second planner and q_des is the model's waypoint at the new q; the blocked world (world 4) reaches its goal
within the CPU run's steps plus a quarter with positive clearance and does not without the call; an episode of
saved worlds 0-3 without the call is bitwise one on a planner that never saw a roadmap; tracking leaves the
planning results unchanged. (The issue's path counters roadmap_* are not in this library: an existing test pins
the last three counters' names, so the census stays as it is and the stats structure carries the counts.)
"""
import ctypes
import os

import numpy as np
import pytest

import armour_amd as A
import episode_model as E
import roadmap_model as R
from test_episode_model import saved
from test_gpu_episode import assert_bitwise, planning_worlds
from test_roadmap_model import STEPS_ROADMAP

pytestmark = pytest.mark.gpu

T = 20
EPS = 2.0 ** -52
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def ctx():
    """the fixture, its worlds at rest at their starts, the models (computed once) and a planner with the
    roadmap built after a reach of the mixed batch"""
    fx = np.load(os.path.join(HERE, "golden", "roadmap_worlds.npz"))
    robot = E.kinova()
    counts = fx["counts"]
    z = np.zeros(7)
    worlds = [(fx["q0"][w], z, z, E.waypoint(robot, fx["q0"][w], fx["goals"][w]), fx["obstacles"][w][:counts[w]]) for w in range(5)]
    radius, step, margin, lookahead = (float(v) for v in fx["config"])
    cfg = dict(connect_radius=radius, edge_step=step, margin=margin)
    models = [R.build(robot, fx["nodes"][w], fx["goals"][w], worlds[w][4], radius, step, margin) for w in range(5)]
    P = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    P.reach_mixed(worlds)
    stats = P.roadmap_build(fx["nodes"], fx["goals"], **cfg)
    yield dict(fx=fx, robot=robot, worlds=worlds, goals=fx["goals"], nodes=fx["nodes"], cfg=cfg, lookahead=lookahead, models=models,
               P=P, stats=stats)
    P.close()


def test_build_matches_the_model(ctx):
    P, models = ctx["P"], ctx["models"]
    for k in ("free_nodes", "candidate_edges", "edges", "edge_samples", "reachable"):
        assert ctx["stats"][k] == sum(m["stats"][k] for m in models), k
    assert ctx["stats"]["relax_rounds_max"] == max(m["stats"]["relax_rounds_max"] for m in models)
    assert np.all(ctx["stats"]["build_ms"] > 0)
    print("stats", ctx["stats"])
    z = np.zeros(7)
    for w, m in enumerate(models):
        g = P.roadmap(w)
        assert np.array_equal(g["is_free"] != 0, m["is_free"]), w
        assert np.array_equal(g["adjacency"], m["adjacency"]), w
        assert np.array_equal(g["next"], m["next"]), w
        assert np.array_equal(np.isinf(g["togo"]), np.isinf(m["togo"])), w
        fin = np.isfinite(m["togo"])
        np.testing.assert_allclose(g["togo"][fin], m["togo"][fin], rtol=1e-13, atol=0)
        assert np.array_equal(np.isinf(g["clearance"]), np.isinf(m["clearance"])), w
        worst = 0.0
        for v in range(0, len(m["verts"]), 7):   # (every 7th vertex: the bound is a model call each)
            if len(ctx["worlds"][w][4]) == 0:
                break
            c = E.clearance(ctx["robot"], (m["verts"][v], z, z, z), ctx["worlds"][w][4], 0.0, 0.0, 1)
            if c["fragile"]:
                assert g["clearance"][v] >= c["floor"] - c["bound"], (w, v)
            else:
                assert abs(g["clearance"][v] - c["clearance"]) <= c["bound"], (w, v, g["clearance"][v], c["clearance"])
                worst = max(worst, abs(g["clearance"][v] - c["clearance"]) / c["bound"])
        fin = np.isfinite(m["clearance"])
        print(f"world {w}: clearance error {np.abs(g['clearance'][fin] - m['clearance'][fin]).max() if fin.any() else 0:.2e}, {worst:.2e} of the bound")


def test_node_clearance_is_check_motion(ctx):
    P = ctx["P"]
    got = [P.roadmap(w)["clearance"] for w in range(5)]
    traj = np.zeros((5, 4, 7))
    for v in (0, 3, 5, 7, 42, 99, 100):
        for w in range(5):
            traj[w, 0] = ctx["models"][w]["verts"][v]
        clear, _ = P.check_motion(traj, 0.0, 0.0, 1)
        for w in range(5):
            assert clear[w] == got[w][v], (v, w, clear[w], got[w][v])
    assert got[0][5] < 0 and np.all(np.isinf(got[1]))


def test_build_twice_is_bitwise(ctx):
    P = ctx["P"]
    first = [P.roadmap(w) for w in range(5)]
    stats = P.roadmap_build(ctx["nodes"], ctx["goals"], **ctx["cfg"])
    for k, v in ctx["stats"].items():
        assert k == "build_ms" or stats[k] == v, k
    for w in range(5):
        g = P.roadmap(w)
        for k in g:
            assert np.array_equal(g[k], first[w][k], equal_nan=True), (w, k)


def test_waypoints_match_the_model(ctx):
    P, lookahead = ctx["P"], ctx["lookahead"]
    queries = ctx["fx"]["queries"]
    seen = dict(entry=0, fallback=0, clamp=0)
    for k in range(queries.shape[1]):
        q = queries[:, k]
        q_des, entry, left = P.roadmap_waypoint(q, lookahead)
        for w in range(5):
            m_des, m_entry, m_left = R.waypoint(ctx["models"][w], q[w], lookahead)
            assert entry[w] == m_entry, (k, w, entry[w], m_entry)
            tol = 64 * EPS * (np.abs(q[w]) + lookahead)
            assert np.all(np.abs(q_des[w] - m_des) <= tol), (k, w, q_des[w] - m_des)
            if m_entry < 0:
                assert left[w] == np.inf
                seen["fallback"] += 1
            else:
                assert abs(left[w] - m_left) <= 1e-13 * m_left, (k, w)
                seen["entry"] += 1
                seen["clamp"] += int(m_left < lookahead)
    assert seen["entry"] >= 60 and seen["fallback"] >= 40 and seen["clamp"] >= 12, seen
    # the fallback is the straight-line q_des of episode_begin, bit for bit
    far = queries[:, 16]
    q_des, entry, _ = P.roadmap_waypoint(far, lookahead)
    assert np.all(entry == -1)
    z = np.zeros(7)
    Q = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    st = Q.episode_begin([(far[w], z, z, far[w], ctx["worlds"][w][4]) for w in range(5)], ctx["goals"], lookahead=lookahead)
    Q.close()
    assert np.array_equal(q_des, st["q_des"])


def test_large_set(ctx):
    fx = ctx["fx"]
    P = A.Planner(T=T, max_obstacles=6, max_worlds=1)
    P.reach_mixed(ctx["worlds"][:1])
    stats = P.roadmap_build(fx["big_nodes"][None], ctx["goals"][:1], **ctx["cfg"])
    g = P.roadmap(0)
    P.close()
    print("N = 1023:", stats)
    assert np.array_equal(g["is_free"] != 0, fx["big_is_free"])
    got = [stats[k] for k in ("free_nodes", "candidate_edges", "edges", "edge_samples", "reachable")]
    assert got == [int(v) for v in fx["big_counts"]]
    bits = int(np.unpackbits(g["adjacency"].view(np.uint8)).sum())
    assert bits == 2 * stats["edges"]


def test_build_leaves_the_plan_alone(ctx):
    worlds = ctx["worlds"]
    P = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    Q = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    res, _ = P.plan_mixed(worlds)
    before = [(P.constraints(w), P.link_centers(w)) for w in range(5)]
    P.roadmap_build(ctx["nodes"], ctx["goals"], **ctx["cfg"])
    P.roadmap_waypoint(ctx["fx"]["queries"][:, 0], ctx["lookahead"])
    for w in range(5):
        assert np.array_equal(P.constraints(w), before[w][0]) and np.array_equal(P.link_centers(w), before[w][1])
    assert all(v == 0 for k, v in P.path_counts().items() if k.startswith("roadmap"))
    res2, _ = P.plan_mixed(worlds)
    Q.plan_mixed(worlds)
    want, _ = Q.plan_mixed(worlds)
    assert_bitwise(res2, want, "the plan after a build")
    # the plan invalidated the roadmap
    L = A.lib()
    assert L.armour_roadmap_get(P.h, 0, None, None, None, None, None) == A.ARMOUR_E_STATE
    assert b"roadmap" in L.armour_last_error()
    assert L.armour_roadmap_waypoint(P.h, A._ptr(np.zeros((5, 7))), 0.1, None, None, None) == A.ARMOUR_E_STATE
    P.close()
    Q.close()


def test_argument_errors_name_their_fields(ctx):
    P, L = ctx["P"], A.lib()
    nodes, goals = np.ascontiguousarray(ctx["nodes"]), np.ascontiguousarray(ctx["goals"])

    def build(N=100, radius=1.0, step=0.05, margin=0.02, n=nodes, g=goals):
        cfg = A.RoadmapConfig(N, radius, step, margin)
        rc = L.armour_roadmap_build(P.h, ctypes.byref(cfg), A._ptr(n), A._ptr(g), None)
        return rc, L.armour_last_error().decode()

    for kw, word in ((dict(N=1), "num_nodes"), (dict(N=1024), "num_nodes"), (dict(radius=np.nan), "connect_radius"),
                     (dict(radius=0.0), "connect_radius"), (dict(radius=100.5), "connect_radius"), (dict(step=0.0), "edge_step"),
                     (dict(step=np.inf), "edge_step"), (dict(radius=50.0, step=0.01), "connect_radius / edge_step"),
                     (dict(margin=-0.1), "margin"), (dict(margin=np.nan), "margin"), (dict(n=None), "null"), (dict(g=None), "null")):
        rc, msg = build(**kw)
        assert rc == A.ARMOUR_E_ARG and word in msg, (kw, rc, msg)
    bad = nodes.copy()
    bad[2, 17, 3] = np.nan
    rc, msg = build(n=bad)
    assert rc == A.ARMOUR_E_ARG and "nodes" in msg and "finite" in msg, msg
    bad[2, 17, 3] = 2e4
    rc, msg = build(n=bad)
    assert rc == A.ARMOUR_E_ARG and "nodes" in msg and "ARMOUR_MAX_ABS_ANGLE" in msg, msg
    badg = goals.copy()
    badg[1, 0] = np.inf
    rc, msg = build(g=badg)
    assert rc == A.ARMOUR_E_ARG and "goals" in msg, msg
    # none of them touched the roadmap
    assert L.armour_roadmap_get(P.h, 0, None, None, None, None, None) == 0
    assert L.armour_roadmap_waypoint(P.h, A._ptr(np.zeros((5, 7))), 0.0, None, None, None) == A.ARMOUR_E_ARG
    assert "lookahead" in L.armour_last_error().decode()
    qbad = np.zeros((5, 7))
    qbad[3, 2] = np.nan
    assert L.armour_roadmap_waypoint(P.h, A._ptr(qbad), 0.1, None, None, None) == A.ARMOUR_E_ARG
    # before any batch, on an ARMTD planner
    Q = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    cfg = A.RoadmapConfig(100, 1.0, 0.05, 0.02)
    assert L.armour_roadmap_build(Q.h, ctypes.byref(cfg), A._ptr(nodes), A._ptr(goals), None) == A.ARMOUR_E_STATE
    assert L.armour_episode_roadmap(Q.h, ctypes.byref(cfg), A._ptr(nodes)) == A.ARMOUR_E_STATE
    assert L.armour_episode_get_roadmap(Q.h, None, None) == A.ARMOUR_E_STATE
    Q.close()
    Z = A.ArmtdPlanner(T=T, max_obstacles=6, max_worlds=5)
    assert L.armour_roadmap_build(Z.h, ctypes.byref(cfg), A._ptr(nodes), A._ptr(goals), None) == A.ARMOUR_E_ARG
    assert "ARMTD" in L.armour_last_error().decode()
    Z.close()


def test_episode_steps_follow_plan_and_model(ctx):
    """each step's results are bitwise plan_mixed of the states read before it; q_des is the model's waypoint
    at the new q; the getter's entry and path left are the model's"""
    worlds, goals, lookahead = ctx["worlds"], ctx["goals"], ctx["lookahead"]
    P = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    P2 = A.Planner(T=T, max_obstacles=6, max_worlds=5)
    st0 = P.episode_begin(worlds, goals, lookahead=lookahead)
    st = P.episode_roadmap(ctx["nodes"], **ctx["cfg"])

    def check(st, moved, tag):
        entry, left = P.episode_roadmap_state()
        for w in moved:
            m_des, m_entry, m_left = R.waypoint(ctx["models"][w], st["q"][w], lookahead)
            assert entry[w] == m_entry, (tag, w, entry[w], m_entry)
            assert np.all(np.abs(st["q_des"][w] - m_des) <= 64 * EPS * (np.abs(st["q"][w]) + lookahead)), (tag, w)
            assert left[w] == m_left or abs(left[w] - m_left) <= 1e-13 * m_left, (tag, w)
        return entry

    entry = check(st, range(5), "begin")
    assert entry[3] == -1 and np.array_equal(st["q_des"][3], st0["q_des"][3])   # the goal is not free: the straight line
    assert np.all(entry[[0, 1, 4]] >= 0)
    for k in ("q", "qd", "qdd", "status", "mode", "steps"):
        assert np.array_equal(st[k], st0[k]), k
    for step in range(5):
        before = st
        running, res, _ = P.episode_step()
        st = P.episode_states()
        want, _ = P2.plan_mixed(planning_worlds(before, worlds))
        assert_bitwise(res, want, f"step {step}")
        moved = [w for w in range(5) if before["status"][w] == 0 and not np.array_equal(before["q"][w], st["q"][w])]
        assert len(moved) >= 3
        check(st, moved, f"step {step}")
    P.close()
    P2.close()


def test_blocked_world_needs_the_roadmap(ctx):
    w = 4
    worlds, goals = ctx["worlds"][w:w + 1], ctx["goals"][w:w + 1]
    cap = STEPS_ROADMAP + (STEPS_ROADMAP + 3) // 4
    P = A.Planner(T=T, max_obstacles=6, max_worlds=1)
    out = A.run_episodes(P, worlds, goals, cap, roadmap=dict(nodes=ctx["nodes"][w:w + 1], **ctx["cfg"]), lookahead=ctx["lookahead"])
    print("roadmap:", out)
    assert out["status"][0] == 1 and out["steps"][0] <= cap and out["clearance"][0] > 0
    line = A.run_episodes(P, worlds, goals, cap, lookahead=ctx["lookahead"])
    print("straight line:", line)
    assert line["status"][0] == 0 and line["steps"][0] == cap
    assert P.episode_states()["goal_distance"][0] > 1.0
    P.close()


def test_episodes_without_the_call_are_the_parents(ctx):
    """saved worlds 0-3: an episode on a planner that built and used a roadmap before is bitwise one on a planner
    that never saw a roadmap"""
    pairs = [saved(i) for i in range(4)]
    worlds, goals = [p[0] for p in pairs], np.array([p[1] for p in pairs])
    O = max(len(wd[4]) for wd in worlds)
    P = A.Planner(T=T, max_obstacles=O, max_worlds=4)
    Q = A.Planner(T=T, max_obstacles=O, max_worlds=4)
    rng = np.random.default_rng(1)
    nodes = np.array([A.roadmap_nodes(ctx["robot"], worlds[w][0], goals[w], 40, 0.2, rng) for w in range(4)])
    P.episode_begin(worlds, goals)
    P.episode_roadmap(nodes, **ctx["cfg"])
    P.episode_step()
    a, b = P.episode_begin(worlds, goals), Q.episode_begin(worlds, goals)
    assert A.lib().armour_episode_get_roadmap(P.h, None, None) == A.ARMOUR_E_STATE   # a new begin ended it
    for step in range(6):
        for k in a:
            assert np.array_equal(a[k], b[k], equal_nan=True), (step, k)
        ra, rb = P.episode_step()[1], Q.episode_step()[1]
        assert_bitwise(ra, rb, f"step {step}")
        a, b = P.episode_states(), Q.episode_states()
    P.close()
    Q.close()


def test_tracking_leaves_the_roadmap_episode_alone(ctx):
    w = 0
    worlds, goals = ctx["worlds"][w:w + 1], ctx["goals"][w:w + 1]
    roadmap = dict(nodes=ctx["nodes"][w:w + 1], **ctx["cfg"])
    P = A.Planner(T=T, max_obstacles=6, max_worlds=1)
    Q = A.Planner(T=T, max_obstacles=6, max_worlds=1)
    P.episode_begin(worlds, goals, lookahead=ctx["lookahead"])
    P.episode_roadmap(**roadmap)
    Q.episode_begin(worlds, goals, lookahead=ctx["lookahead"])
    Q.episode_track(num_samples=2, steps=250, stop_on_input=False, stop_on_bound=False, stop_on_limit=False)
    Q.episode_roadmap(**roadmap)
    for step in range(4):
        ra, rb = P.episode_step()[1], Q.episode_step()[1]
        assert_bitwise(ra, rb, f"step {step}")
        a, b = P.episode_states(), Q.episode_states()
        for k in ("q", "qd", "qdd", "q_des", "status", "steps"):
            assert np.array_equal(a[k], b[k]), (step, k)
    assert np.array_equal(P.episode_roadmap_state()[0], Q.episode_roadmap_state()[0])
    assert Q.episode_tracked()["max_pos_err"].max() > 0
    P.close()
    Q.close()
