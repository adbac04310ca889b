"""Point model of armour_track — TEST INFRASTRUCTURE: numpy, no oracle, no product code.

The definition in include/armour_hip.h (armour_track), vectorised over rollouts: the true arm
`M qdd = u - b` with scaled masses and inertias under the reference's ARMOUR robust controller
(robust_controller.cpp:63-168), integrated by classical RK4 with a fixed number of steps. The Bezier
curve and the joint rotations come from point_model; the RNEA with its midpoint-radius uncertainty
bound and the unpivoted Cholesky are this file's own. Sums run left to right in index order, as the
definition says, so that the model's rounding stays close to the product's.
"""
from __future__ import annotations

import numpy as np

import point_model as pm

NF = 7
K_RANGE = np.pi / 48


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], axis=1)


def _abscross(a, b):
    a, b = np.abs(a), np.abs(b)
    return np.stack([a[:, 1] * b[:, 2] + a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] + a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] + a[:, 1] * b[:, 0]], axis=1)


def _mv(A, x):
    """[R, 3, 3] x [R, 3], each row summed left to right"""
    return A[:, :, 0] * x[:, None, 0] + A[:, :, 1] * x[:, None, 1] + A[:, :, 2] * x[:, None, 2]


def _mtv(A, x):
    return A[:, 0, :] * x[:, None, 0] + A[:, 1, :] * x[:, None, 1] + A[:, 2, :] * x[:, None, 2]


def rnea_radius(robot, q, qd, qa, qdda, mass=None, inertia=None, gravity=True, damping=True, Rs=None):
    """(u, rho) [R, 7]: the point RNEA R(q, qd, qa, qdda) with masses `mass` [R, NJ] and inertias
    `inertia` [R, NJ, 3, 3] (default: nominal), and its radius for mass (1 +- dm), inertia (1 +- dI)"""
    q, qd, qa, qdda = (np.atleast_2d(np.asarray(v, dtype=np.float64)) for v in (q, qd, qa, qdda))
    R_, NJ = q.shape[0], int(robot["num_joints"])
    m = np.broadcast_to(robot["mass"], (R_, NJ)) if mass is None else mass
    I = np.broadcast_to(robot["inertia"], (R_, NJ, 3, 3)) if inertia is None else inertia
    dm, dI = float(robot["mass_uncertainty"]), float(robot["inertia_uncertainty"])
    Rs = pm.joint_rotations(robot, q) if Rs is None else Rs
    trans, com = robot["trans"], robot["com"]
    z3 = np.zeros((R_, 3))
    w, wa, wd, acc = z3.copy(), z3.copy(), z3.copy(), z3.copy()
    acc[:, pm.GRAVITY_AXIS] = robot["gravity"] * np.asarray(gravity, dtype=np.float64)   # (a flag, or one per row)
    F, N, rF, rN = [], [], [], []
    for i in range(NJ):
        p = np.broadcast_to(trans[i], (R_, 3))
        acc = _mtv(Rs[i], acc + _cross(wd, p) + _cross(w, _cross(wa, p)))
        w, wa, wd = _mtv(Rs[i], w), _mtv(Rs[i], wa), _mtv(Rs[i], wd)
        ax = int(robot["axes"][i])
        if ax != 0 and i < NF:
            z = pm.axis_vector(ax)[None, :]
            zq = qd[:, i, None] * z
            cr = _cross(wa, zq)
            w = w + zq
            wd = wd + cr + qdda[:, i, None] * z
            wa = wa + qa[:, i, None] * z
        c = np.broadcast_to(com[i], (R_, 3))
        ac = acc + _cross(wd, c) + _cross(w, _cross(wa, c))
        F.append(m[:, i, None] * ac)
        rF.append(dm * np.abs(m[:, i, None]) * np.abs(ac))
        Ii = I[:, i]
        N.append(_mv(Ii, wd) + _cross(wa, _mv(Ii, w)))
        rN.append(dI * (_mv(np.abs(Ii), np.abs(wd)) + _abscross(wa, _mv(np.abs(Ii), np.abs(w)))))
    f, n, rf, rn = z3.copy(), z3.copy(), z3.copy(), z3.copy()
    u = np.zeros((R_, NF))
    rho = np.zeros((R_, NF))
    eye = np.broadcast_to(np.eye(3), (R_, 3, 3))
    for i in range(NJ - 1, -1, -1):
        R1 = Rs[i + 1] if i + 1 < NJ else eye
        c = np.broadcast_to(com[i], (R_, 3))
        p1 = np.broadcast_to(trans[i + 1], (R_, 3))
        Rf, Rn = _mv(R1, f), _mv(R1, n)
        n = N[i] + Rn + _cross(c, F[i]) + _cross(p1, Rf)
        f = Rf + F[i]
        rRf, rRn = _mv(np.abs(R1), rf), _mv(np.abs(R1), rn)
        rn = rN[i] + rRn + _abscross(c, rF[i]) + _abscross(p1, rRf)
        rf = rRf + rF[i]
        ax = int(robot["axes"][i])
        if ax != 0 and i < NF:
            z = pm.axis_vector(ax)
            v = n[:, 0] * z[0] + n[:, 1] * z[1] + n[:, 2] * z[2] + robot["armature"][i] * qdda[:, i]
            v = np.where(np.asarray(damping, dtype=bool), v + robot["damping"][i] * qd[:, i], v)
            u[:, i] = v
            rho[:, i] = rn[:, 0] * abs(z[0]) + rn[:, 1] * abs(z[1]) + rn[:, 2] * abs(z[2])
    return u, rho


def wrap_diff(d):
    m = np.fmod(d + np.pi, 2 * np.pi)
    m = np.where(m < 0, m + 2 * np.pi, m)
    return m - np.pi


def _seqsum(x):
    """sum over the last axis in index order"""
    s = np.zeros(x.shape[:-1])
    for j in range(x.shape[-1]):
        s = s + x[..., j]
    return s


def cholesky_solve(M, rhs):
    """(x, ok): M x = rhs by the unpivoted Cholesky on the entries i >= j, column by column"""
    R_ = M.shape[0]
    L = np.zeros((R_, NF, NF))
    ok = np.ones(R_, dtype=bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for j in range(NF):
            s = M[:, j, j].copy()
            for k in range(j):
                s = s - L[:, j, k] * L[:, j, k]
            ok &= (s > 0) & np.isfinite(s)
            d = np.sqrt(s)
            L[:, j, j] = d
            for i in range(j + 1, NF):
                v = M[:, i, j].copy()
                for k in range(j):
                    v = v - L[:, i, k] * L[:, j, k]
                L[:, i, j] = v / d
        y = np.zeros((R_, NF))
        for i in range(NF):
            v = rhs[:, i].copy()
            for k in range(i):
                v = v - L[:, i, k] * y[:, k]
            y[:, i] = v / L[:, i, i]
        x = np.zeros((R_, NF))
        for i in range(NF - 1, -1, -1):
            v = y[:, i].copy()
            for k in range(i + 1, NF):
                v = v - L[:, k, i] * x[:, k]
            x[:, i] = v / L[:, i, i]
    return x, ok


class Rollouts:
    """R rollouts: traj [R, 4, 7] (one per rollout), scale [R, 2, NJ] or None, err0 [R, 2, 7] or None"""

    def __init__(self, robot, traj, scale=None, err0=None):
        self.robot = robot
        self.traj = np.asarray(traj, dtype=np.float64)
        R_, NJ = self.traj.shape[0], int(robot["num_joints"])
        self.R = R_
        scale = np.ones((R_, 2, NJ)) if scale is None else np.asarray(scale, dtype=np.float64)
        self.mass = robot["mass"][None, :] * scale[:, 0]
        self.inertia = robot["inertia"][None] * scale[:, 1, :, None, None]
        self.err0 = np.zeros((R_, 2, NF)) if err0 is None else np.asarray(err0, dtype=np.float64)
        self.beta = pm.control_points(self.traj[:, 0], self.traj[:, 1], self.traj[:, 2], self.traj[:, 3] * K_RANGE)
        self.cont = np.asarray(robot["state_lb"]) <= -1000.0

    def desired(self, t):
        return pm.bezier(self.beta, t)

    def stage(self, t, q, qd):
        """dict: u, qdd [R, 7], V, lam [R], ok [R], q_des, qd_des"""
        rb = self.robot
        K, alpha, V_m = float(rb["K"]), float(rb["alpha"]), float(rb["V_m"])
        q_des, qd_des, qdd_des = self.desired(t)
        e = q_des - q
        e = np.where(self.cont[None, :], wrap_diff(e), e)
        de = qd_des - qd
        qa_d, qa_dd, r = qd_des + K * e, qdd_des + K * de, de + K * e
        # the ten RNEAs of the stage as one stacked call (rows role * R + rollout): columns of M and b
        # with the true parameters, tau and Mr with the nominal ones; gravity and damping for b and tau
        R_ = self.R
        zero = np.zeros_like(q)
        units = [np.where(np.arange(NF)[None, :] == j, 1.0, zero) for j in range(NF)]
        nom_m = np.broadcast_to(rb["mass"], self.mass.shape)
        nom_I = np.broadcast_to(rb["inertia"], self.inertia.shape)
        full = np.repeat(np.array([0.0] * NF + [1.0, 1.0, 0.0]), R_)
        Rs = [np.tile(Rj, (10, 1, 1)) for Rj in pm.joint_rotations(rb, q)]
        U, RAD = rnea_radius(rb, np.tile(q, (10, 1)), np.concatenate([zero] * NF + [qd, qd, zero]),
                             np.concatenate([zero] * NF + [qd, qa_d, zero]), np.concatenate(units + [zero, qa_dd, r]),
                             np.concatenate([self.mass] * 8 + [nom_m] * 2), np.concatenate([self.inertia] * 8 + [nom_I] * 2),
                             gravity=full, damping=full, Rs=Rs)
        U, RAD = U.reshape(10, R_, NF), RAD.reshape(10, R_, NF)
        M = np.stack([U[j] for j in range(NF)], axis=2)
        b, tau, rho, Mr, rMr = U[7], U[8], RAD[8], U[9], RAD[9]
        V_sup = 0.5 * (_seqsum(r * Mr) + _seqsum(np.abs(r) * rMr))
        h = V_m - V_sup
        nr, nrho = np.sqrt(_seqsum(r * r)), np.sqrt(_seqsum(rho * rho))
        with np.errstate(invalid="ignore", divide="ignore"):
            lam = np.where(nr > 0, np.fmax(0.0, -alpha * h / nr + nrho), 0.0)
            u = np.where(nr[:, None] > 0, tau + lam[:, None] * r / nr[:, None], tau)
        qdd, ok = cholesky_solve(M, u - b)
        Mr_true = np.zeros_like(q)
        for j in range(NF):
            Mr_true = Mr_true + M[:, :, j] * r[:, j, None]
        V = 0.5 * _seqsum(r * Mr_true)
        ok = ok & np.all(np.isfinite(qdd), axis=1) & np.all(np.isfinite(u), axis=1) & np.isfinite(V) & np.isfinite(lam)
        return dict(u=u, qdd=qdd, V=V, lam=lam, ok=ok, q_des=q_des, qd_des=qd_des)

    def run(self, t0=0.0, t1=0.5, steps=250):
        """the outputs of armour_track as arrays over the rollouts"""
        q_des, qd_des, _ = self.desired(t0)
        q, qd = q_des + self.err0[:, 0], qd_des + self.err0[:, 1]
        R_ = self.R
        out = dict(max_pos_err=np.zeros((R_, NF)), max_vel_err=np.zeros((R_, NF)), max_torque=np.zeros((R_, NF)),
                   max_V=np.zeros(R_), max_robust=np.zeros(R_))
        alive = np.ones(R_, dtype=bool)

        def record(S, q, qd):
            nonlocal alive
            alive = alive & S["ok"]
            a = alive
            for name, val in (("max_pos_err", np.abs(q - S["q_des"])), ("max_vel_err", np.abs(qd - S["qd_des"])),
                              ("max_torque", np.abs(S["u"])), ("max_V", S["V"]), ("max_robust", S["lam"])):
                out[name][a] = np.fmax(out[name][a], val[a])

        h = (t1 - t0) / steps
        hh = 0.5 * h
        with np.errstate(all="ignore"):
            for s in range(steps):
                t = t0 + s * h
                S1 = self.stage(t, q, qd)
                record(S1, q, qd)
                q2, v2 = q + hh * qd, qd + hh * S1["qdd"]
                S2 = self.stage(t + hh, q2, v2)
                q3, v3 = q + hh * v2, qd + hh * S2["qdd"]
                S3 = self.stage(t + hh, q3, v3)
                q4, v4 = q + h * v3, qd + h * S3["qdd"]
                S4 = self.stage(t + h, q4, v4)
                qn = q + (h / 6) * (qd + 2 * v2 + 2 * v3 + v4)
                vn = qd + (h / 6) * (S1["qdd"] + 2 * S2["qdd"] + 2 * S3["qdd"] + S4["qdd"])
                good = S1["ok"] & S2["ok"] & S3["ok"] & S4["ok"] & np.all(np.isfinite(qn), axis=1) & np.all(np.isfinite(vn), axis=1)
                alive = alive & good
                q = np.where(alive[:, None], qn, q)
                qd = np.where(alive[:, None], vn, qd)
            record(self.stage(t1, q, qd), q, qd)
        out["end_state"] = np.stack([q, qd], axis=1)
        out["status"] = (~alive).astype(np.int32)
        return out


def track(robot, traj, scale=None, err0=None, t0=0.0, t1=0.5, steps=250):
    """armour_track's outputs for traj [N, 4, 7], scale [N, S, 2, NJ] / None, err0 [N, S, 2, 7] / None, shaped
    [N, S, ...]"""
    traj = np.asarray(traj, dtype=np.float64)
    N = traj.shape[0]
    S = 1 if scale is None and err0 is None else (np.shape(scale)[1] if scale is not None else np.shape(err0)[1])
    flat = np.repeat(traj, S, axis=0)
    sc = None if scale is None else np.asarray(scale, dtype=np.float64).reshape(N * S, 2, -1)
    e0 = None if err0 is None else np.asarray(err0, dtype=np.float64).reshape(N * S, 2, NF)
    out = Rollouts(robot, flat, sc, e0).run(t0, t1, steps)
    return {k: v.reshape((N, S) + v.shape[1:]) for k, v in out.items()}
