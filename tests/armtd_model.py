"""Model of the ARMTD comparison planner's definitions — TEST INFRASTRUCTURE, independent of the oracle.

oracle/src/armtd.cpp and the HIP path (jrs_armtd_kernel, armtd_extrema_cost, the ARMTD instantiations of
the evaluation kernel) restate the same reference lines; a shared misreading passes a comparison of the
two. This module states in numpy, with no oracle code and no PZ code, what those lines MEAN:

  * the curve: ACMP/Trajectory.cu:83-93 read as a trajectory. With ka = k_range x the joint accelerates
    at ka for t <= 0.5, q = q0 + qd0 t + ka t^2 / 2, then brakes at constant deceleration to rest at
    t = 1 (q_ddot_to_stop = -q_dot_peak / 0.5);
  * its exact extrema over [0, 1] from the curve's critical points (not from the reference's branch
    text): q at t in {0, 0.5, 1} and at -qd0 / ka when that lies strictly inside (0, 0.5); qd is
    piecewise linear, so its extrema are among {qd0, qd0 + ka / 2, 0};
  * cost and gradient (ACMP/NLPclass.cu:186-246): q_plan = q0 + qd0 / 2 + k_range x / 8, the squared
    distance from the goal, wrapped to (-pi, pi] on the robot's wrap mask, times
    COST_FUNCTION_OPTIMALITY_SCALE (ACMP/Parameters.h:39);
  * the table enclosure: cos and sin of the relative angle q(t) - q0 lie in c + g x +- r per interval
    (the offline JRS, ACMP/offline_jrs/create_orig_offline_jrs.m, sliced as KSI/uarmtd_planner.m:288-314);
  * affine forward kinematics: with the tables fixed and the radius zero, the ARMTD link sets are the
    link boxes under joint rotations C I + (1 - C) u u^T + S [u]x whose C, S are affine in x
    (ACMP/Trajectory.cu:38-54: the table entries rotated by q0), chained as point_model.link_points.
"""
from __future__ import annotations

import numpy as np

import point_model as PM

T_MOVE = 0.5
COST_SCALE = 10.0   # ACMP/Parameters.h:39


# ---- curve --------------------------------------------------------------------------------------
def relative(qd0, ka, t):
    """(q(t) - q0, qd(t)) of the constant-acceleration curve; qd0, ka, t broadcast"""
    qd0, ka, t = (np.asarray(v, dtype=np.float64) for v in (qd0, ka, t))
    vp = qd0 + ka * T_MOVE                              # speed at t = 0.5
    rp = qd0 * T_MOVE + 0.5 * ka * T_MOVE ** 2          # position at t = 0.5
    s = t - T_MOVE
    dec = -vp / (1.0 - T_MOVE)
    move = t <= T_MOVE
    q = np.where(move, qd0 * t + 0.5 * ka * t * t, rp + vp * s + 0.5 * dec * s * s)
    qd = np.where(move, qd0 + ka * t, vp + dec * s)
    return q, qd


def curve(q0, qd0, k_range, x, t):
    """(q [N, 7], qd [N, 7]) at the times t [N]"""
    t = np.asarray(t, dtype=np.float64).reshape(-1, 1)
    r, v = relative(np.asarray(qd0)[None, :], (np.asarray(k_range) * np.asarray(x))[None, :], t)
    return np.asarray(q0)[None, :] + r, v


def extrema(q0, qd0, k_range, x):
    """[4, 7] = min q, max q, min qd, max qd over t in [0, 1], from the critical points"""
    q0, qd0, ka = (np.asarray(v, dtype=np.float64) for v in (q0, qd0, np.asarray(k_range) * np.asarray(x)))
    out = np.zeros((4, q0.size))
    for i in range(q0.size):
        ts = [0.0, T_MOVE, 1.0]
        if ka[i] != 0.0:
            with np.errstate(over="ignore"):
                tc = -qd0[i] / ka[i]
            if 0.0 < tc < T_MOVE:
                ts.append(tc)
        r, _ = relative(qd0[i], ka[i], np.array(ts))
        cand = q0[i] + r
        vel = np.array([qd0[i], qd0[i] + ka[i] * T_MOVE, 0.0])
        out[:, i] = cand.min(), cand.max(), vel.min(), vel.max()
    return out


# ---- cost ---------------------------------------------------------------------------------------
def wrap_to_pi(a):
    """the representative of a in [-pi, pi] reached by whole turns (ACMP/NLPclass.cu:6-15 leaves +-pi)"""
    a = np.asarray(a, dtype=np.float64)
    w = a - 2 * np.pi * np.round(a / (2 * np.pi))
    return w


def cost(q0, qd0, k_range, q_des, x, wrap):
    """f(x) of ACMP/NLPclass.cu:186-216 (scaled)"""
    qp = np.asarray(q0) + 0.5 * np.asarray(qd0) + np.asarray(k_range) * np.asarray(x) / 8.0
    d = np.asarray(q_des) - qp
    d = np.where(np.asarray(wrap) != 0, wrap_to_pi(d), d)
    return COST_SCALE * float(np.sum(d * d))


def cost_gradient(q0, qd0, k_range, q_des, x, wrap):
    """df/dx of ACMP/NLPclass.cu:221-246"""
    kr = np.asarray(k_range, dtype=np.float64)
    qp = np.asarray(q0) + 0.5 * np.asarray(qd0) + kr * np.asarray(x) / 8.0
    d = qp - np.asarray(q_des)
    d = np.where(np.asarray(wrap) != 0, wrap_to_pi(d), d)
    return COST_SCALE * 2.0 * d * kr / 8.0


# ---- tables -------------------------------------------------------------------------------------
def table_enclosure(tables, k_range, qd0, x, t):
    """worst |error| / r of cos / sin of the relative angle against c + g x, over the joints and the
    times t [T] (t[s] inside interval s). tables [7][6][T] = c_cos, g_cos, r_cos, c_sin, g_sin, r_sin"""
    tables = np.asarray(tables, dtype=np.float64)
    worst = 0.0
    for i in range(tables.shape[0]):
        a, _ = relative(qd0[i], k_range[i] * x[i], t)
        ec = np.abs(np.cos(a) - (tables[i, 0] + tables[i, 1] * x[i])) / tables[i, 2]
        es = np.abs(np.sin(a) - (tables[i, 3] + tables[i, 4] * x[i])) / tables[i, 5]
        worst = max(worst, float(ec.max()), float(es.max()))
    return worst


def sliced_cos_sin(tables, q0, x):
    """(C, S) [T, 7]: the table centres and k-generators rotated by q0 and sliced at x
    (ACMP/Trajectory.cu:38-54 without the radius)"""
    tables = np.asarray(tables, dtype=np.float64)
    cq, sq = np.cos(q0), np.sin(q0)
    cc, gc, cs, gs = tables[:, 0].T, tables[:, 1].T, tables[:, 3].T, tables[:, 4].T    # [T, 7]
    x = np.asarray(x, dtype=np.float64)
    C = cq * cc - sq * cs + (cq * gc - sq * gs) * x
    S = cq * cs + sq * cc + (cq * gs + sq * gc) * x
    return C, S


# ---- affine forward kinematics ------------------------------------------------------------------
def affine_link_points(robot, C, S, box_coords=PM.BOX_CORNERS):
    """[NJ, N, P, 3] world points of every link box under joint rotations RPY_i (C_i I + (1 - C_i) u u^T
    + S_i [u]x) with C, S [N, 7] given (not required to satisfy C^2 + S^2 = 1), chained as
    point_model.link_points"""
    N = C.shape[0]
    R = np.broadcast_to(np.eye(3), (N, 3, 3))
    p = np.zeros((N, 3))
    out = []
    for i in range(int(robot["num_joints"])):
        p = p + R @ robot["trans"][i]
        Ri = np.broadcast_to(PM.rpy(*robot["rots"][i]), (N, 3, 3))
        ax = int(robot["axes"][i])
        if ax != 0 and i < C.shape[1]:
            u = PM.axis_vector(ax)
            K = np.array([[0.0, -u[2], u[1]], [u[2], 0.0, -u[0]], [-u[1], u[0], 0.0]])
            c, s = C[:, i, None, None], S[:, i, None, None]
            Ri = Ri @ (c * np.eye(3) + (1 - c) * np.outer(u, u) + s * K)
        R = R @ Ri
        local = robot["link_center"][i] + box_coords * robot["link_generators"][i]
        out.append(p[:, None, :] + np.einsum("nij,pj->npi", R, local))
    return np.array(out)
