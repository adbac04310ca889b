"""Generator of tests/golden/roadmap_worlds.npz: the worlds, node sets and query points of the roadmap tests
(tests/test_roadmap_model.py, tests/test_gpu_roadmap.py). Run from the repository root:

    python tests/golden/make_roadmap_worlds.py

Five Kinova worlds with 3, 0, 6, 2 and 1 box obstacles, their goals, a node set of N = 100 each
(armour_amd.roadmap_nodes; connect_radius 1.0, edge_step 0.05, margin 0.02), 32 query points each, and one
set of N = 1023 for world 0 with the model's is_free and edge counts:

  world 0   nodes 3 and 7 bitwise identical (an exact tie with no edge between them), node 5 inside an obstacle
  world 1   no obstacles
  world 2   the nodes in two clusters farther apart than connect_radius: two components
  world 3   the goal inside an obstacle: every togo is +infinity and every waypoint falls back
  world 4   the blocked world: a slab across the straight joint-space line from start to goal; the node set is one
            with which the oracle-driven episode (roadmap_model.oracle_episode) reaches the goal within 70 steps

The query points: 8 on a node, 8 in the middle of an edge, 4 out of reach of every vertex, 4 next to the
goal, 8 near a node. The guard bands are asserted on the model (tests/roadmap_model.py), seeds are tried until
they hold: no vertex, edge-sample or entry-sample clearance within 1e-9 of the margin; no distance within
1e-9 of connect_radius or ARMOUR_ROADMAP_MIN_EDGE; no d / edge_step of a candidate edge or an entry segment
within 1e-9 of an integer (d = 0 exactly, the query on a node and the identical pair, is exact on both
sides: b - a = 0); no runner-up within 1e-9 of a next or entry winner other than between bitwise identical
vertices.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "armour-dev_amd")]

import armour_amd as A  # noqa: E402
import episode_model as E  # noqa: E402
import roadmap_model as R  # noqa: E402

RADIUS, STEP, MARGIN, LOOKAHEAD, BAND = 1.0, 0.05, 0.02, 0.1, 1e-9
COUNTS = (3, 0, 6, 2, 1)
N, NQ, OMAX = 100, 32, 6
STEP_CAP = 70   # of the oracle-driven episodes (tests/test_roadmap_model.py)
START4 = np.array([-0.9, 0.9, 0.0, 1.0, 0.0, 0.6, 0.0])
SLAB = np.array([0.7, 0.0, 0.3, 0.2, 0, 0, 0, 0.03, 0, 0, 0, 0.3])


class Retry(Exception):
    pass


def need(cond, what):
    if not cond:
        raise Retry(what)


def near_integer(x):
    return np.abs(x - np.round(x)) < BAND


def band_build(rm):
    """the guard bands of a built roadmap"""
    sc = np.concatenate([rm["clearance"]] + list(rm["sample_clearance"]))
    need(not np.any(np.abs(sc[np.isfinite(sc)] - MARGIN) < BAND), "a clearance at the margin")
    V = rm["verts"].shape[0]
    ii, jj = np.triu_indices(V, 1)
    _, d = R.delta(rm["robot"], rm["verts"][ii], rm["verts"][jj])
    need(not np.any(np.abs(d - RADIUS) < BAND) and not np.any(np.abs(d - R.MIN_EDGE) < BAND), "a distance at a threshold")
    need(not np.any(near_integer(rm["cand"]["d"] / STEP)), "an edge length at a multiple of edge_step")
    same = (rm["verts"][:, None, :] == rm["verts"][None, :, :]).all(-1)
    for i in np.flatnonzero(np.isfinite(rm["togo"])[:-1]):
        c = rm["weight"][i] + rm["togo"]
        c[same[rm["next"][i]]] = np.inf
        need(c.min() - rm["togo"][i] >= BAND, "a runner-up at a next winner")


def band_query(rm, q):
    """the guard bands of one waypoint query; returns the model's (q_des, entry, path_left)"""
    q_des, entry, left, info = R.waypoint(rm, q, LOOKAHEAD, detail=True)
    d = info["d"]
    need(not np.any(np.abs(d - RADIUS) < BAND), "a query distance at connect_radius")
    for i, sc in info["segments"].items():
        need(d[i] == 0.0 or not near_integer(d[i] / STEP), "an entry segment at a multiple of edge_step")
        need(not np.any(np.abs(sc - MARGIN) < BAND), "an entry sample at the margin")
    if entry >= 0:
        c = info["cost"].copy()
        c[(rm["verts"] == rm["verts"][entry]).all(-1)] = np.inf
        if d[entry] == 0.0 and entry < rm["next"][entry]:
            # the query on node i: the way through next[i] costs d(v_i, v_next) + togo[next] = togo[i], the same
            # operations on the same operands (lower index first): an exact tie, to the lower index
            c[rm["next"][entry]] = np.inf
        need(c.min() - left >= BAND, "a runner-up at an entry winner")
    return q_des, entry, left


def colliding(robot, rng, centre, obstacles, spread):
    q = centre + spread * rng.standard_normal((3000, 7))
    hit = np.flatnonzero(R.clearance(robot, q, obstacles) < -0.01)
    need(len(hit) > 0, "no configuration inside an obstacle")
    return q[hit[0]]


def queries(robot, rng, rm, goal, w):
    verts, N_ = rm["verts"], rm["verts"].shape[0] - 1
    good = np.flatnonzero(rm["is_free"][:-1] & np.isfinite(rm["togo"][:-1]))
    good = good[good < rm["next"][good]]   # (band_query: the exact tie of a query on a node)
    pool = good if len(good) >= 8 else np.arange(N_)
    on = verts[rng.choice(pool, 8, replace=False)]
    e = np.flatnonzero(rm["exists"])
    if len(e) >= 8:
        pick = rng.choice(e, 8, replace=False)
        a, b = verts[rm["cand"]["i"][pick]], verts[rm["cand"]["j"][pick]]
        mid = a + 0.5 * R.delta(robot, a, b)[0]
    else:
        mid = verts[rng.choice(N_, 8, replace=False)] + 0.05 * rng.standard_normal((8, 7))
    far = goal + np.array([0.0, 2.2, 0.0, -2.4, 0.0, 2.0, 0.0]) * rng.choice([-1.0, 1.0], (4, 7)) + 0.05 * rng.standard_normal((4, 7))
    for f in far:
        need(R.delta(robot, np.broadcast_to(f, verts.shape), verts)[1].min() > RADIUS + 0.1, "a far query within reach")
    close = goal + 0.02 * rng.standard_normal((4, 7))
    near = verts[rng.choice(N_, 8, replace=False)] + 0.1 * rng.standard_normal((8, 7))
    qs = np.concatenate([on, mid, far, close, near])
    res = [band_query(rm, q) for q in qs]
    entries = np.array([r[1] for r in res])
    if w == 3:
        need(np.all(entries == -1), "world 3 must fall back everywhere")
    else:
        need(np.all(entries[16:20] == -1), "the far queries must fall back")
        if np.isfinite(rm["togo"]).any():
            need(np.all(entries[:8] >= 0) and np.all(entries[20:24] >= 0), "on-node and goal queries have an entry")
            for r, q in zip(res[20:24], qs[20:24]):   # the clamp: the walk ends at the goal, short of lookahead
                need(r[2] < LOOKAHEAD, "a goal query farther than lookahead")
    return qs


def world(robot, w, seed):
    rng = np.random.default_rng(1000 * w + seed)
    O = COUNTS[w]
    if w == 4:
        q0, obs = START4.copy(), SLAB[None].copy()
        goal = q0.copy()
        goal[0] = 0.9
        nodes = A.roadmap_nodes(robot, q0, goal, N, SPREAD4, rng)
    else:
        wd = A.make_world(50 + 10 * w + seed, max(O, 1))
        q0 = np.asarray(wd[0], dtype=np.float64)
        obs = np.asarray(wd[4], dtype=np.float64).reshape(-1, 12)[:O]
        off = rng.standard_normal(7)
        goal = q0 + (3.0 if w == 2 else 1.5) * off / np.linalg.norm(off)
        if w == 3:
            goal = colliding(robot, rng, q0 + 1.0 * off / np.linalg.norm(off), obs, 0.7)
        if w == 2:
            nodes = np.concatenate([A.roadmap_nodes(robot, q0, q0, N // 2, 0.15, rng), A.roadmap_nodes(robot, goal, goal, N // 2, 0.15, rng)])
        else:
            nodes = A.roadmap_nodes(robot, q0, goal, N, 0.3, rng)
        if w == 0:
            nodes[5] = colliding(robot, rng, nodes[5], obs, 0.7)
            nodes[7] = nodes[3]
    for v in np.concatenate([nodes, goal[None]]).reshape(-1):
        need(abs(v) < 1e4, "an angle outside the input domain")
    rm = R.build(robot, nodes, goal, obs, RADIUS, STEP, MARGIN)
    band_build(rm)
    free, togo = rm["is_free"], rm["togo"]
    if w == 0:
        need(not free[5] and free[3] and free[7] and np.isfinite(togo[3]) and rm["weight"][3, 7] == np.inf, "world 0's special nodes")
    if w == 2:
        need(np.any(free & np.isinf(togo)) and np.isfinite(togo[:-1]).sum() >= 20, "world 2 needs two components")
    if w == 3:
        need(not free[N] and np.all(np.isinf(togo)), "world 3's goal must not be free")
    if w in (0, 1, 4):
        need(np.isfinite(togo).sum() >= 60, "too few reachable vertices")
    if w == 4:
        need(R.waypoint(rm, q0, LOOKAHEAD)[1] >= 0, "the blocked world's start has no entry")
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        st = R.oracle_episode(robot, (q0, np.zeros(7), np.zeros(7), q0.copy(), obs), goal, rm, STEP_CAP)
        need(st["status"] == 1 and st["clearance"] > 0, f"the blocked world's episode ended with status {st['status']}")
        print(f"world 4: the roadmap episode reaches the goal in {st['steps']} steps, clearance {st['clearance']:.4f}")
    qs = queries(robot, rng, rm, goal, w)
    pad = np.zeros((OMAX, 12))
    pad[:O] = obs
    return dict(q0=q0, goal=goal, obstacles=pad, nodes=nodes, queries=qs, rm=rm)


SPREAD4 = 0.35


def main():
    robot = E.kinova()
    out = []
    for w in range(len(COUNTS)):
        for seed in range(50):
            try:
                out.append(world(robot, w, seed))
                print(f"world {w}: seed {seed}", out[-1]["rm"]["stats"], flush=True)
                break
            except Retry as r:
                print(f"world {w}: seed {seed} refused: {r}", flush=True)
        else:
            raise SystemExit(f"world {w}: no seed holds the guard bands")
    # the large set: world 0, N = 1023, a wider tube so that the graph stays sparse
    w0 = out[0]
    for seed in range(20):
        try:
            big = A.roadmap_nodes(robot, w0["q0"], w0["goal"], R.MAX_NODES, 0.5, np.random.default_rng(7000 + seed))
            rmb = R.build(robot, big, w0["goal"], w0["obstacles"][:COUNTS[0]], RADIUS, STEP, MARGIN)
            band_build(rmb)
            break
        except Retry as r:
            print(f"large set: seed {seed} refused: {r}", flush=True)
    else:
        raise SystemExit("large set: no seed holds the guard bands")
    print("large set", rmb["stats"], flush=True)
    st = rmb["stats"]
    np.savez(os.path.join(HERE, "roadmap_worlds.npz"), counts=np.array(COUNTS), q0=np.array([o["q0"] for o in out]),
             goals=np.array([o["goal"] for o in out]), obstacles=np.array([o["obstacles"] for o in out]),
             nodes=np.array([o["nodes"] for o in out]), queries=np.array([o["queries"] for o in out]),
             config=np.array([RADIUS, STEP, MARGIN, LOOKAHEAD]), big_nodes=big, big_is_free=rmb["is_free"],
             big_counts=np.array([st["free_nodes"], st["candidate_edges"], st["edges"], st["edge_samples"], st["reachable"]]))


if __name__ == "__main__":
    main()
