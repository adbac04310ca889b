"""Model of the roadmap high-level planner — TEST INFRASTRUCTURE, independent of the HIP path (numpy only).

What armour_roadmap_build and armour_roadmap_waypoint (include/armour_hip.h) compute, restated from the
contract on episode_model.link_boxes / separation / wrap, with the contract's sequence of IEEE operations:
the sequential 7-term sum of squares, sqrt, fmod (numpy's %), one division per sample fraction and per
partial leg, and a Dijkstra that adds togo[j] + w. The library is built with -ffp-contract=off, so
distances, togo and path_left are expected to agree to rounding and the decisions exactly (away from the
guard bands the fixture's generator asserts).

One world at a time: `build` returns a dict, `waypoint` reads it.
"""
from __future__ import annotations

import heapq

import numpy as np

import episode_model as EM

MAX_NODES = 1023     # ARMOUR_ROADMAP_MAX_NODES
MIN_EDGE = 1e-6      # ARMOUR_ROADMAP_MIN_EDGE
WORDS = 32


def continuous(robot):
    return np.asarray(robot["state_lb"], dtype=np.float64)[:7] <= -1000.0


def delta(robot, a, b):
    """Delta(a -> b) [..., 7] and d(a, b) [...]: wrapped on continuous joints, squares summed in joint order"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = b - a
    cont = continuous(robot)
    d[..., cont] = EM.wrap(d[..., cont])
    s = np.zeros(d.shape[:-1])
    for j in range(7):
        s = s + d[..., j] * d[..., j]
    return d, np.sqrt(s)


def clearance(robot, q, obstacles, chunk=4096):
    """clr(q) [N] of the configurations q [N, 7]: the minimum over (link, obstacle) of the separation"""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 7)
    obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 12)
    out = np.full(q.shape[0], np.inf)
    if obstacles.shape[0] == 0:
        return out
    for lo in range(0, q.shape[0], chunk):
        c, G = EM.link_boxes(robot, q[lo:lo + chunk])
        sep = EM.separation(c[:, :, None, :], G[:, :, None, :, :], obstacles[None, None, :, :])
        out[lo:lo + chunk] = sep.reshape(sep.shape[0], -1).min(-1)
    return out


def pieces(d, step):
    return np.ceil(np.asarray(d) / step).astype(np.int64)


def segment_samples(a, dl, n):
    """the interior samples a + (s / n) dl, s = 1 .. n - 1: [n - 1, 7]"""
    s = np.arange(1, n, dtype=np.float64)
    return a + (s / float(n))[:, None] * dl


def build(robot, nodes, goal, obstacles, connect_radius, edge_step, margin):
    """The roadmap of one world. dict: verts [V, 7] (the goal last), clearance [V], is_free [V], cand: the
    candidate edges in (i, j) order as arrays i, j, d, n, sample_clearance: a list of [n - 1] arrays per
    candidate, exists [E], adjacency [V, 32] uint32, weight [V, V] (inf: no edge), togo, next [V], stats."""
    verts = np.concatenate([np.asarray(nodes, dtype=np.float64).reshape(-1, 7), np.asarray(goal, dtype=np.float64).reshape(1, 7)])
    V = verts.shape[0]
    N = V - 1
    clr = clearance(robot, verts, obstacles)
    free = clr > margin
    ii, jj = np.triu_indices(V, 1)
    both = free[ii] & free[jj]
    ii, jj = ii[both], jj[both]
    dl, d = delta(robot, verts[ii], verts[jj])
    keep = (d >= MIN_EDGE) & (d <= connect_radius)
    ii, jj, dl, d = ii[keep], jj[keep], dl[keep], d[keep]
    n = pieces(d, edge_step)
    # every interior sample of every candidate, in one clearance call
    off = np.concatenate([[0], np.cumsum(n - 1)])
    e_of = np.repeat(np.arange(len(n)), n - 1)
    s_of = np.arange(off[-1]) - off[e_of] + 1
    pts = verts[ii[e_of]] + (s_of / n[e_of].astype(np.float64))[:, None] * dl[e_of]
    sc = clearance(robot, pts, obstacles)
    blocked = np.zeros(len(n), dtype=bool)
    np.logical_or.at(blocked, e_of, ~(sc > margin))
    exists = ~blocked
    weight = np.full((V, V), np.inf)
    weight[ii[exists], jj[exists]] = d[exists]
    weight[jj[exists], ii[exists]] = d[exists]
    adj = np.zeros((V, WORDS), dtype=np.uint32)
    for a, b in ((ii[exists], jj[exists]), (jj[exists], ii[exists])):
        np.bitwise_or.at(adj, (a, b >> 5), (np.uint32(1) << (b & 31).astype(np.uint32)))
    togo, rounds = relax(weight, N, bool(free[N]))
    nxt = np.full(V, -1, dtype=np.int64)
    for i in range(V):
        if np.isfinite(togo[i]):
            nxt[i] = N if i == N else int(np.flatnonzero(weight[i] + togo == togo[i])[0])
    stats = dict(free_nodes=int(free.sum()), candidate_edges=int(len(n)), edges=int(exists.sum()),
                 edge_samples=int(off[-1]), reachable=int(np.isfinite(togo).sum()), relax_rounds_max=rounds)
    return dict(verts=verts, clearance=clr, is_free=free, cand=dict(i=ii, j=jj, d=d, n=n), sample_clearance=np.split(sc, off[1:-1]),
                exists=exists, adjacency=adj, weight=weight, togo=togo, next=nxt, stats=stats, robot=robot,
                obstacles=np.asarray(obstacles, dtype=np.float64).reshape(-1, 12), connect_radius=connect_radius,
                edge_step=edge_step, margin=margin)


def dijkstra(weight, goal):
    """togo by Dijkstra from `goal` with the additions togo[j] + w"""
    V = weight.shape[0]
    togo = np.full(V, np.inf)
    togo[goal] = 0.0
    heap, done = [(0.0, goal)], np.zeros(V, dtype=bool)
    while heap:
        t, j = heapq.heappop(heap)
        if done[j]:
            continue
        done[j] = True
        for i in np.flatnonzero(np.isfinite(weight[j]) & ~done):
            c = togo[j] + weight[i, j]
            if c < togo[i]:
                togo[i] = c
                heapq.heappush(heap, (c, i))
    return togo


def relax(weight, goal, goal_free):
    """(togo, rounds): Dijkstra's togo (every togo +infinity when the goal is not free) and the number of
    Jacobi rounds from +infinity that change a value (every vertex takes min(own, min_j w + togo[j]) from
    the previous round's values), whose fixed point is the same"""
    V = weight.shape[0]
    if not goal_free:
        return np.full(V, np.inf), 0
    togo = np.full(V, np.inf)
    togo[goal] = 0.0
    rounds = 0
    while True:
        new = np.minimum(togo, (weight + togo[None, :]).min(1))
        new[goal] = 0.0
        if np.array_equal(new, togo):
            break
        togo, rounds = new, rounds + 1
    d = dijkstra(weight, goal)
    assert np.array_equal(d, togo), "the Jacobi fixed point is Dijkstra's"
    return togo, rounds


def waypoint(rm, q, lookahead, detail=False):
    """(q_des [7], entry, path_left) at q; detail: also a dict with the candidates' costs (inf: no candidate),
    the entry segments' sample clearances and the walk's polyline"""
    robot, verts = rm["robot"], rm["verts"]
    V = verts.shape[0]
    N = V - 1
    q = np.asarray(q, dtype=np.float64)
    dl, d = delta(robot, np.broadcast_to(q, verts.shape), verts)
    cost = np.full(V, np.inf)
    seg = {}
    near = np.flatnonzero(rm["is_free"] & np.isfinite(rm["togo"]) & (d <= rm["connect_radius"]))
    pts = [segment_samples(q, dl[i], int(pieces(d[i], rm["edge_step"]))) for i in near]
    every = clearance(robot, np.concatenate(pts), rm["obstacles"]) if pts else np.zeros(0)   # (one call for all segments)
    for i, sc in zip(near, np.split(every, np.cumsum([len(p) for p in pts])[:-1]) if pts else []):
        seg[int(i)] = sc
        if np.all(sc > rm["margin"]):
            cost[i] = d[i] + rm["togo"][i]
    info = dict(cost=cost, d=d, segments=seg, polyline=[q.copy()])
    if not np.isfinite(cost).any():
        out = (EM.waypoint(robot, q, verts[N], lookahead), -1, np.inf)
        return out + (info,) if detail else out
    entry = int(np.argmin(cost))
    pos, a, r, cur = q.copy(), q, float(lookahead), entry
    for _ in range(N + 2):
        dl1, d1 = delta(robot, a, verts[cur])
        if r > d1:
            pos = pos + dl1
            r -= float(d1)
            info["polyline"].append(pos.copy())
        else:
            pos = pos + (r / d1) * dl1
            break
        if cur == N:
            break
        a, cur = verts[cur], int(rm["next"][cur])
    out = (pos, entry, float(cost[entry]))
    return out + (info,) if detail else out


def oracle_episode(robot, world, goal, rm, cap, lookahead=0.1):
    """the state after an episode of one world driven by the oracle's plans at T = 20 (episode_model.begin / step),
    for at most `cap` steps: the straight-line waypoint (rm None) or the roadmap's"""
    from oracle import OraclePlanner

    st = EM.begin(robot, world, goal, lookahead)
    if rm is not None:
        st["q_des"] = waypoint(rm, st["q"], lookahead)[0]
    for _ in range(cap):
        if st["status"] != 0:
            break
        P = OraclePlanner(st["q"], st["qd"], st["qdd"], st["q_des"], world[4], T=20, threads=8)
        P.reach()
        r = P.plan()
        st = EM.step(robot, st, r["k_opt"], bool(r["feasible"]), world[4], goal, lookahead)
        if rm is not None and st["status"] == 0:
            st["q_des"] = waypoint(rm, st["q"], lookahead)[0]
    return st
