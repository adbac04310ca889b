"""Generate tests/golden/zonotope_worlds.npz (build container, repo root):

    python tests/golden/make_zonotope_worlds.py

Worlds whose obstacles are general zonotopes with three generators, not only axis-aligned boxes
(include/armour_hip.h: "center + 3 generators"). The reach sets do not depend on the obstacles, so
per world the oracle's reach() runs once, the link generators and the link centres at a stored x*
are taken from it, and every obstacle is placed with tests/collision_model.py (not with the
oracle): its centre is bisected along a random direction from a link centre until the model's row
of one (link, time step) at x* takes a target value. The targets put rows on both sides of 0 and of
COL_THR = 1e-4, none closer than 1e-6 to either: +-1e-2, 1e-4 +- 1e-6, -1e-4 +- 1e-6, +-1e-6.

Obstacle kinds (one or more of each per world): see KINDS below. The fixture stores inputs only
(the worlds, the kinds and targets, x* and the evaluation points, and ten placed obstacles for
world 0 of tests/golden/armtd_T100_O10.npz); expected values come from the oracle at test time
and from the model.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("armour-dev_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import boundary_worlds as B  # noqa: E402
import collision_model as M  # noqa: E402
from armour_amd.worlds import make_world  # noqa: E402
from oracle import OracleArmtd, OraclePlanner  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
COL_THR = B.COL_THR
TARGETS = [1e-2, -1e-2, 1e-4 + 1e-6, 1e-4 - 1e-6, -1e-4 + 1e-6, -1e-4 - 1e-6, 1e-6, -1e-6]
# no decision closer than this to 0 or COL_THR at any stored point (the targets sit at 1e-6 up to
# the bisection's resolution)
CLEAR = 1e-6 * (1 - 1e-3)

# every world carries these, in this order, then cycles through REPEAT up to its O
KINDS = ["box", "rotated", "sheared", "plate", "rod", "point", "parallel", "near_parallel", "negperm", "dup",
         "tiny", "floor", "huge", "contain", "rotated", "sheared", "rotated", "sheared", "plate", "rod"]
REPEAT = ["rotated", "sheared", "box", "plate", "rod", "point", "parallel", "near_parallel", "negperm", "tiny"]
# name -> (robot, make_world seed, T, O)
WORLDS = {"kinova0": ("kinova", 4100, 8, 20), "kinova1": ("kinova", 4101, 8, 20), "kinova_small": ("kinova", 4102, 4, 40),
          "fetch": ("fetch", 4103, 4, 40)}
ARMTD_KINDS = ["box", "rotated", "sheared", "plate", "rod", "point", "parallel", "near_parallel", "negperm", "tiny"]


def rotation(rng):
    """uniform on SO(3) (QR of a Gaussian matrix, signs fixed)"""
    q, r = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.diag(r))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q


def generators(kind, rng):
    """[3, 3] obstacle generators, one per row"""
    half = rng.uniform(0.02, 0.15, 3)
    Rm = rotation(rng)
    if kind == "box":
        return np.diag(half)
    if kind == "rotated":
        return half[:, None] * Rm.T
    if kind == "sheared":
        S = np.eye(3) + np.triu(rng.uniform(-0.8, 0.8, (3, 3)), 1)
        return half[:, None] * (Rm @ S).T
    if kind in ("plate", "rod"):
        G = half[:, None] * Rm.T
        G[rng.permutation(3)[:1 if kind == "plate" else 2]] = 0.0
        return G
    if kind == "point":
        return np.zeros((3, 3))
    if kind in ("parallel", "near_parallel"):
        g1, g3 = half[0] * Rm[:, 0], half[2] * Rm[:, 2]
        g2 = 0.7 * g1
        if kind == "near_parallel":
            g2 = g2 + 1e-12 * Rm[:, 1]
        return np.array([g1, g2, g3])
    if kind == "negperm":  # negated and permuted: -0.0 components
        return -np.diag(half)[[2, 0, 1]]
    if kind == "tiny":
        return 1e-6 * Rm.T
    if kind == "floor":
        return np.diag([5.0, 5.0, 0.0025])
    if kind == "huge":
        return np.diag([1e3, 1e3, 1e3])
    if kind == "contain":
        return np.diag([3.0, 3.0, 3.0])
    raise ValueError(kind)


def place(G3, base, u, LG, target, reach):
    """obstacle centre base + s u at which the model's row of the link (centre base, generators LG
    [3, 6]) takes `target`: bisection on s (the row is the negated maximum of functions affine in
    the centre, so it falls through every level once along the ray)"""
    G = M.buffered(G3, LG)

    def f(s):
        return float(M.row(base, base + s * u, G)["g"])

    lo, hi = 0.0, reach
    if not (f(lo) > target > f(hi)):
        return None
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if f(mid) > target:
            lo = mid
        else:
            hi = mid
    s = lo if abs(f(lo) - target) <= abs(f(hi) - target) else hi
    return base + s * u


def place_kinds(kinds, rng, lc, LG, k0=0):
    """obstacles [O, 12], targets [O, 3] = (t, l, value) (NaN where the kind is not placed on a row)"""
    T, NJ = lc.shape[:2]
    obs, tg = [], []
    k = k0
    for kind in kinds:
        if kind == "dup":  # the same obstacle listed twice
            obs.append(obs[1].copy())
            tg.append(tg[1].copy())
            continue
        if kind == "contain":
            obs.append(np.concatenate([lc.reshape(-1, 3).mean(0), generators(kind, rng).reshape(-1)]))
            tg.append(np.full(3, np.nan))
            continue
        for _ in range(50):
            G3 = generators(kind, rng)
            t, l = int(rng.integers(0, T)), int(rng.integers(1, NJ))
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            reach = 3.0
            if kind == "floor":  # below the base: pushed down from the lowest link centre
                t, l = np.unravel_index(np.argmin(lc[:, :, 2]), lc.shape[:2])
                u = np.array([0.0, 0.0, -1.0])
            if kind == "huge":  # 1e3 m away, one face passing near the arm
                u = np.eye(3)[int(rng.integers(0, 3))] * rng.choice([-1.0, 1.0])
                reach = 1e3 + 3.0
            target = TARGETS[k % len(TARGETS)]
            c = place(G3, lc[t, l], u, LG[t, l], target, reach)
            if c is not None:
                break
        else:
            raise RuntimeError(f"could not place {kind}")
        k += 1
        obs.append(np.concatenate([c, G3.reshape(-1)]))
        tg.append(np.array([t, l, target], dtype=np.float64))
    return np.array(obs), np.array(tg)


def model_rows(obstacles, lc, LG):
    """[NJ, T, O] model rows, the order of g's collision block"""
    G = M.buffered(obstacles[None, None, :, 3:].reshape(1, 1, -1, 3, 3), LG[:, :, None])
    g = M.row(lc[:, :, None, :], obstacles[None, None, :, :3], G)["g"]
    return g.transpose(1, 0, 2)


def eval_points(rng, x_star):
    alt = np.array([1, -1, 1, -1, 1, -1, 1.0])
    outside = rng.uniform(-1, 1, 7) * 1.5
    outside[int(rng.integers(0, 7))] = 1.4  # surely outside the certified box: the full scan
    return np.array([x_star, np.zeros(7), np.ones(7), -np.ones(7), alt, rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7),
                     outside])


def make(name, robot, seed, T, O):
    geo, rs, _ = B.robot_of(robot)
    q0, qd0, qdd0, q_des, _ = make_world(seed, 0, robot=geo, profile="survey")
    R = OraclePlanner(q0, qd0, qdd0, q_des, np.zeros((0, 12)), T=T, threads=8, robot=rs)
    R.reach()
    LG = R.link_gens()
    kinds = (KINDS + REPEAT * 4)[:O]
    for attempt in range(20):
        rng = np.random.default_rng(seed * 100 + attempt)
        x_star = rng.uniform(-0.6, 0.6, 7)
        pts = eval_points(rng, x_star)
        _, _, lc = R.eval(x_star, centers=True)
        obs, tg = place_kinds(kinds, rng, lc, LG, k0=3 * list(WORLDS).index(name))
        worst = np.inf
        for x in pts:
            _, _, c = R.eval(x, centers=True)
            g = model_rows(obs, c, LG)
            worst = min(worst, np.abs(g).min(), np.abs(g - COL_THR).min())
        if worst >= CLEAR:
            break
        print(f"{name}: a decision {worst:.2e} from a threshold, next draw", flush=True)
    else:
        raise RuntimeError("no draw keeps every decision clear of the thresholds")
    g = model_rows(obs, lc, LG)
    hit = [g[int(l), int(t), o] - v for o, (t, l, v) in enumerate(tg) if np.isfinite(v)]
    assert np.abs(hit).max() < 1e-9, np.abs(hit).max()
    print(f"{name}: T={T} O={O} NJ={R.NJ} closest decision {worst:.3e}, targets hit within {np.abs(hit).max():.1e}, "
          f"rows > 0: {(g > 0).mean():.2f}", flush=True)
    return {"q0": q0, "qd0": qd0, "qdd0": qdd0, "q_des": q_des, "obstacles": obs, "kinds": np.array(kinds),
            "targets": tg, "x_star": x_star, "points": pts, "T": np.int64(T), "robot": np.array(robot)}


def make_armtd():
    """ten kinds for world 0 of armtd_T100_O10.npz, placed on the OracleArmtd centres at x*"""
    fx = dict(np.load(os.path.join(OUT, "armtd_T100_O10.npz")))
    T = int(fx["T"])
    w = (fx["q0"][0], fx["qd0"][0], fx["q_des"][0], fx["tables"][0], fx["k_range"][0], fx["obstacles"][0])
    R = OracleArmtd(*w, T=T, threads=8)
    R.reach()
    rng = np.random.default_rng(4200)
    x_star = rng.uniform(-0.6, 0.6, 7)
    _, _, lc = R.eval(x_star, centers=True)
    obs, tg = place_kinds(ARMTD_KINDS, rng, lc, R.link_gens())
    return {"armtd_obstacles": obs, "armtd_kinds": np.array(ARMTD_KINDS), "armtd_targets": tg, "armtd_x_star": x_star}


def main():
    out = {"names": np.array(list(WORLDS))}
    for name, (robot, seed, T, O) in WORLDS.items():
        for k, v in make(name, robot, seed, T, O).items():
            out[f"{name}_{k}"] = v
    out.update(make_armtd())
    path = os.path.join(OUT, "zonotope_worlds.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
