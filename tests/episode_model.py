"""Model of plan execution — TEST INFRASTRUCTURE, independent of the oracle and of the HIP path (numpy only).

What armour_check_motion and armour_episode_step (include/armour_hip.h) compute, restated from the
definitions with tests/point_model.py (the Bezier trajectory, point forward kinematics of the link
boxes) and tests/collision_model.py (`row`, the plane test of KPR/CollisionChecking.cu):

  * separation of a link box from an obstacle zonotope: -row(c, c_obs, G)["g"] with G = [obstacle 3,
    link 3, three zero rows] (the zero rows span no plane, so 15 axes remain);
  * clearance of a trajectory over a sampled window: the minimum over samples, links and obstacles,
    with its first minimiser in the order (sample, link, obstacle);
  * the episode step: which segment a world executes, the advance to the segment's end, the
    straight-line waypoint (armour_amd.worlds.straight_line_waypoint), the goal distance and the
    status / mode / counter bookkeeping.

A state is a dict with the fields of armour_episode_state plus "pending" (the last accepted plan
(q0, qd0, qdd0, k) or None) for one world.
"""
from __future__ import annotations

import numpy as np

import collision_model as C
import point_model as PM

EPS = 2.0 ** -52
K_RANGE = np.pi / 48          # KPR/Parameters.h, planner_defaults
T_PLAN = 0.5
MAX_ABS_ANGLE = 1e4           # ARMOUR_MAX_ABS_ANGLE


def kinova():
    """the built-in Kinova tables as point_model wants them (host-side call into the product library)"""
    from armour_amd import robot_tables as RT

    return RT._shaped(RT.builtin(0))


# ---- trajectory ---------------------------------------------------------------------------------
def sample_times(t0, t1, samples):
    return np.linspace(t0, t1, samples) if samples > 1 else np.array([float(t0)])


def trajectory(traj, t):
    """(q, qd, qdd) [N, 7] of traj = (q0, qd0, qdd0, k normalised) at the times t [N]"""
    q0, qd0, qdd0, k = (np.asarray(v, dtype=np.float64) for v in traj)
    beta = PM.control_points(q0, qd0, qdd0, k * K_RANGE)          # [7, 6]
    q, qd, qdd = PM.bezier(beta[None], np.asarray(t, dtype=np.float64)[:, None])
    return q, qd, qdd


# ---- link boxes and separation --------------------------------------------------------------------
def link_boxes(robot, q):
    """(centres [N, NJ, 3], generators [N, NJ, 3, 3], one generator per row) of the link boxes at q [N, 7]"""
    coords = np.concatenate([np.zeros((1, 3)), np.eye(3)])
    P = PM.link_points(robot, q, box_coords=coords)               # [NJ, N, 4, 3]
    c = P[:, :, 0]
    G = P[:, :, 1:] - c[:, :, None, :]
    return np.swapaxes(c, 0, 1), np.swapaxes(G, 0, 1)


def separation(c_link, G_link, obstacle):
    """max_n (|n . (c - c_obs)| - sum_j |n . G_j|) over the 15 axes; obstacle [..., 12], c_link [..., 3],
    G_link [..., 3, 3] (rows)"""
    obstacle = np.asarray(obstacle, dtype=np.float64)
    Gob = obstacle[..., 3:].reshape(obstacle.shape[:-1] + (3, 3))
    lead = np.broadcast_shapes(Gob.shape[:-2], np.shape(G_link)[:-2])
    G = np.concatenate([np.broadcast_to(Gob, lead + (3, 3)), np.broadcast_to(G_link, lead + (3, 3)),
                        np.zeros(lead + (3, 3))], axis=-2)
    return -C.row(c_link, obstacle[..., :3], G)["g"]


def separations(robot, traj, obstacles, t0, t1, samples):
    """dict over every (sample, link, obstacle), each [S, NJ, O]:
      sep      the separation;
      regular  the separation without the rounding-level planes (collision_model.degenerate);
      fragile  an obstacle generator and a link generator are parallel to rounding and their cross product
               has two or more non-zero components: its direction is an arbitrary unit vector that depends
               on the last bit of the forward kinematics, so two restatements agree on `regular` from
               below only (any unit vector is a valid axis). A rounding-level cross product with a single
               non-zero component (the base link's z generator (0, -sin(pi), -1) g against an upright box)
               normalises to a coordinate axis exactly, whatever its size: not fragile;
      bound    within which two double-precision restatements agree elsewhere (rounding_bound + fk_bound)"""
    obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 12)
    q, _, _ = trajectory(traj, sample_times(t0, t1, samples))
    c, G = link_boxes(robot, q)                                    # [S, NJ, 3], [S, NJ, 3, 3]
    shape = (q.shape[0], G.shape[1], obstacles.shape[0])
    Gob = obstacles[:, 3:].reshape(-1, 3, 3)
    G9 = np.concatenate([np.broadcast_to(Gob[None, None], shape + (3, 3)), np.broadcast_to(G[:, :, None], shape + (3, 3)),
                         np.zeros(shape + (3, 3))], axis=-2)
    cl, co = c[:, :, None, :], obstacles[None, None, :, :3]
    deg = C.degenerate(G9)
    length = np.sqrt((G9 * G9).sum(-1))
    mixed = np.array([a < 3 <= b < 6 for a, b in C.PAIRS])
    live = (length[..., C._IA] > 0) & (length[..., C._IB] > 0) & ((C._cross(G9)[0] != 0).sum(-1) > 1)
    return dict(sep=-C.row(cl, co, G9)["g"], regular=-C.row(cl, co, G9, drop=deg)["g"],
                fragile=(deg & live & mixed).any(-1), bound=C.rounding_bound(cl, co, G9) + fk_bound(robot, traj))


def fk_bound(robot, traj):
    """Rounding of the forward kinematics between two double-precision restatements, in metres.
    L = sum_i |trans_i|_1 + max_l (|link_center_l|_1 + |link_generators_l|_1) bounds every lever arm of
    the chain. (1) Each of the up to 9 chain rotations is a product of three 3x3 matrices whose entries
    carry a few eps (trigonometric functions to 1-2 ulp, 5 operations per product entry): at most
    about 11 eps per joint, 100 eps at the ninth, per restatement: 256 eps L covers two restatements
    with the margin collision_model.rounding_bound takes. (2) A joint angle comes from 6 Bernstein
    terms of about 4 operations each on quantities bounded by A_j = |q0| + |qd0| + |qdd0| + |k| k_range:
    16 eps A_j covers two restatements; the error of joint j moves every later link by at most that
    angle times L."""
    nj = int(robot["num_joints"])
    L = np.abs(robot["trans"][:nj]).sum() + (np.abs(robot["link_center"][:nj]).sum(-1) +
                                               np.abs(robot["link_generators"][:nj]).sum(-1)).max()
    q0, qd0, qdd0, k = (np.abs(np.asarray(v, dtype=np.float64)) for v in traj)
    A = (q0 + qd0 + qdd0 + k * K_RANGE).sum()
    return 256 * EPS * L + 16 * EPS * A * L


def clearance(robot, traj, obstacles, t0, t1, samples):
    """dict(clearance, where (sample, link, obstacle): the first minimum in that order, runner_up: the
    smallest separation at another (sample, link, obstacle) minus the minimum, bound: the largest
    rounding bound of the window, fragile: the minimiser is a fragile pair (separations),
    floor: the minimum of the regular separations (a restatement is never below floor - bound))"""
    obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 12)
    if obstacles.shape[0] == 0:
        return dict(clearance=np.inf, where=(-1, -1, -1), runner_up=np.inf, bound=0.0, fragile=False, floor=np.inf)
    m = separations(robot, traj, obstacles, t0, t1, samples)
    flat = m["sep"].reshape(-1)
    i = int(np.argmin(flat))
    rest = np.delete(flat, i)
    return dict(clearance=float(flat[i]), where=tuple(int(v) for v in np.unravel_index(i, m["sep"].shape)),
                runner_up=float(rest.min() - flat[i]) if rest.size else np.inf, bound=float(m["bound"].max()),
                fragile=bool(m["fragile"].reshape(-1)[i] or m["fragile"].reshape(-1)[int(np.argmin(m["regular"]))]),
                floor=float(m["regular"].min()))


# ---- episodes -------------------------------------------------------------------------------------
def wrap(d):
    return (np.asarray(d, dtype=np.float64) + np.pi) % (2 * np.pi) - np.pi


def goal_distance(q, goal):
    return float(np.sqrt(np.sum(wrap(np.asarray(goal) - np.asarray(q)) ** 2)))


def waypoint(robot, q, goal, lookahead=0.1):
    """armour_amd.worlds.straight_line_waypoint for a robot-table dict (d = 0: the state itself)"""
    q = np.asarray(q, dtype=np.float64)
    d = np.asarray(goal, dtype=np.float64) - q
    cont = np.asarray(robot["state_lb"]) <= -1000.0
    d[cont] = wrap(d[cont])
    n = np.sqrt(np.sum(d * d))
    return q + lookahead * d / n if n > 0 else q.copy()


def begin(robot, world, goal, lookahead=0.1, goal_radius=np.pi / 30):
    q0, qd0, qdd0 = (np.array(v, dtype=np.float64) for v in world[:3])
    dist = goal_distance(q0, goal)
    return dict(q=q0, qd=qd0, qdd=qdd0, q_des=waypoint(robot, q0, goal, lookahead), status=1 if dist <= goal_radius else 0,
                mode=int(np.any(qd0 != 0) or np.any(qdd0 != 0)), steps=0, failed_plans=0, failed_streak=0,
                clearance=np.inf, clearance_at=(-1, -1, -1), goal_distance=dist, pending=None)


def step(robot, state, k_opt, accept, obstacles, goal, lookahead=0.1, goal_radius=np.pi / 30, check_samples=11):
    """the state after one armour_episode_step of one world whose plan from `state` ended at k_opt
    (normalised) and was accepted (feasible and not vetoed) or not"""
    s = dict(state)
    if s["status"] != 0:
        return s
    if accept:
        traj, win = (s["q"], s["qd"], s["qdd"], np.asarray(k_opt, dtype=np.float64)), (0.0, T_PLAN)
        s["failed_streak"] = 0
    else:
        s["failed_plans"] += 1
        s["failed_streak"] += 1
        if s["mode"] == 1 and s["pending"] is not None:
            traj, win = s["pending"], (T_PLAN, 1.0)
        elif s["mode"] == 1:
            s["status"] = 3
            return s
        else:
            s["steps"] += 1
            return s
    step_no = s["steps"]
    s["steps"] += 1
    t = sample_times(win[0], win[1], check_samples)
    q, qd, qdd = trajectory(traj, t)
    if not (np.all(np.isfinite(q[-1])) and np.all(np.isfinite(qd[-1])) and np.all(np.isfinite(qdd[-1])) and
            np.all(np.abs(q[-1]) <= MAX_ABS_ANGLE)):
        s["status"] = 4
        return s
    c = clearance(robot, traj, obstacles, win[0], win[1], check_samples)
    if c["clearance"] < s["clearance"]:
        s["clearance"] = c["clearance"]
        s["clearance_at"] = (step_no, c["where"][1], c["where"][2])
    reached = any(goal_distance(qs, goal) <= goal_radius for qs in q)
    s["q"], s["qd"], s["qdd"] = q[-1].copy(), qd[-1].copy(), qdd[-1].copy()
    s["goal_distance"] = goal_distance(s["q"], goal)
    s["q_des"] = waypoint(robot, s["q"], goal, lookahead)
    if accept:
        s["mode"], s["pending"] = 1, tuple(np.array(v, dtype=np.float64) for v in traj)
    else:
        s["mode"], s["pending"] = 0, None
    if not c["clearance"] > 0:
        s["status"] = 2
    elif reached:
        s["status"] = 1
    return s
