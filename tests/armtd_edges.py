"""Edge worlds of the ARMTD comparison planner and the model checks run on them — TEST INFRASTRUCTURE.

tests/golden/armtd_edges.npz (tests/golden/make_armtd_edges.py) holds worlds the random fixture never
enters: starts at rest (t_mm = -0/k, and 0/0 at x = 0), start speeds that put the interior extremum
-qd0 / k_actual inside (0, 0.5), on 0.5 and next to 0, speeds half-way between two offline-JRS bins and in
the largest bins, q0 on the branch points of cos / sin and many turns out, limited joints next to a
position limit, a goal on the wrap tie, no obstacles, obstacles on the collision threshold. The offline JRS
tables are stored once per velocity bin (jrs_tables [NB, 6, T], jrs_k_range [NB]) and each world names its
seven bins (bins [W, 7]).

The checks compare an evaluator (the oracle in tests/test_armtd_model.py, the HIP path in
tests/test_gpu_armtd_edges.py) with tests/armtd_model.py, which shares no code with either. An evaluator
has eval(x) -> (g, J, centres [T, 7, 3]) and gens() -> [T, 7, 3, 6].
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

import armtd_model as M
import point_model as PM

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
T = 100
CONT = (0, 2, 4, 6)
LIMITED = (1, 3, 5)
FD_H = 1e-6
FD_TOL = 1e-7          # the issue's bar (measured <= 3e-10 extremum rows, <= 1e-9 collision rows and cost)
EXT_TOL = 1e-12        # extremum rows against the exact extrema
CRAFTED_Q0 = np.array([0.3, np.pi / 2, 1000.0, -1.2, 3 * np.pi, 1.0, -7.0])


def load():
    return dict(np.load(os.path.join(GOLD, "armtd_edges.npz")))


def names(fx):
    return [str(n) for n in fx["names"]]


def world(fx, w):
    """(q0, qd0, q_des, tables [7, 6, T], k_range [7], obstacles [O_w, 12]) of fixture world w"""
    b = fx["bins"][w]
    return (fx["q0"][w], fx["qd0"][w], fx["q_des"][w], np.ascontiguousarray(fx["jrs_tables"][b]),
            np.ascontiguousarray(fx["jrs_k_range"][b]), np.ascontiguousarray(fx["obstacles"][w][:int(fx["n_obs"][w])]))


def by_name(fx, name):
    return world(fx, names(fx).index(name))


def digest(wd):
    """SHA-1 of a world's inputs"""
    h = hashlib.sha1()
    for a in wd:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def crafted_world(seed=0, obstacles=None):
    """a world whose tables share nothing with a trajectory: c = (cos a, sin a) of angles drawn
    independently per joint and interval (every entry distinct), generators uniform in +-0.05, radius
    zero. The link sets are then exactly the affine model's boxes (armtd_model.affine_link_points)."""
    rng = np.random.default_rng(71_000 + seed)
    a = rng.uniform(-1.5, 1.5, (7, T))
    tab = np.zeros((7, 6, T))
    tab[:, 0], tab[:, 3] = np.cos(a), np.sin(a)
    tab[:, 1] = rng.uniform(-0.05, 0.05, (7, T))
    tab[:, 4] = rng.uniform(-0.05, 0.05, (7, T))
    kr = rng.uniform(0.1, 0.4, 7)
    qd0 = rng.uniform(-0.5, 0.5, 7)
    q0 = CRAFTED_Q0.copy()
    obs = np.zeros((0, 12)) if obstacles is None else np.asarray(obstacles, dtype=np.float64).reshape(-1, 12)
    return q0, qd0, q0 + 0.1, tab, kr, obs


def half_time_x(qd0, k_range):
    """per joint the x that makes t_mm = -qd0 / (k_range x) equal 0.5 (0 where it lies outside [-1, 1])"""
    with np.errstate(divide="ignore", invalid="ignore"):
        x = -2.0 * np.asarray(qd0) / np.asarray(k_range)
    return np.where(np.isfinite(x) & (np.abs(x) <= 1.0), x, 0.0)


def eval_points(wd, seed=0):
    """[(label, x)] of the issue: 0, +-1, random, -sign(qd0), -0.999 sign(qd0), the x of t_mm = 0.5 and
    its two neighbouring doubles"""
    qd0, kr = np.asarray(wd[1]), np.asarray(wd[4])
    rng = np.random.default_rng(900 + seed)
    xh = half_time_x(qd0, kr)
    s = np.sign(qd0)
    return [("zero", np.zeros(7)), ("plus", np.ones(7)), ("minus", -np.ones(7)), ("random", rng.uniform(-1, 1, 7)),
            ("against", -s), ("against.999", -0.999 * s), ("half", xh),
            ("half-", np.clip(np.nextafter(xh, -np.inf), -1, 1)), ("half+", np.clip(np.nextafter(xh, np.inf), -1, 1))]


# ---- extremum rows ------------------------------------------------------------------------------
_TS = np.linspace(0.0, 1.0, 20001)


def check_extrema(ev, wd, x, label=""):
    """rows g[-28:] are the exact extrema (EXT_TOL) and bracket a 20001-point sampling of the curve within
    the bars of test_oracle_extremum_rows_bracket_the_trajectory. Returns the worst distances."""
    q0, qd0, _, _, kr, _ = wd
    g = ev.eval(x)[0]
    ext = g[-28:].reshape(4, 7)
    assert np.all(np.isfinite(g)), (label, "a row is not finite")
    exact = M.extrema(q0, qd0, kr, x)
    d_exact = float(np.abs(ext - exact).max())
    assert d_exact <= EXT_TOL, (label, "extremum rows miss the exact extrema", ext - exact)
    q, qd = M.curve(q0, qd0, kr, x, _TS)
    d_samp = 0.0
    for row, v, fn in ((0, q, np.min), (1, q, np.max), (2, qd, np.min), (3, qd, np.max)):
        sampled = fn(v, axis=0)
        slack = 1e-12
        if fn is np.min:
            assert np.all(ext[row] <= sampled + slack), (label, row, ext[row] - sampled)
        else:
            assert np.all(ext[row] >= sampled - slack), (label, row, ext[row] - sampled)
        d_samp = max(d_samp, float(np.abs(ext[row] - sampled).max()))
    assert d_samp < 1e-6, (label, d_samp)
    return d_exact, d_samp


# ---- Jacobian rows ------------------------------------------------------------------------------
def _signature(q0, qd0, ka):
    """which candidate attains each extremum and whether the interior critical point exists"""
    ts = [0.0, M.T_MOVE, 1.0]
    inside = ka != 0.0 and 0.0 < -qd0 / ka < M.T_MOVE
    if inside:
        ts.append(-qd0 / ka)
    r, _ = M.relative(qd0, ka, np.array(ts))
    vel = np.array([qd0, qd0 + ka * M.T_MOVE, 0.0])
    # a tie counts as a kink unless the tied candidates are equal for every ka (qd0 = 0 against rest)
    def arg(v, fn):
        k = int(fn(v))
        ties = [j for j in range(len(v)) if j != k and abs(v[j] - v[k]) < 1e-9]
        return (k, tuple(ties))
    return (np.sign(ka), inside, arg(r, np.argmin), arg(r, np.argmax), arg(vel, np.argmin), arg(vel, np.argmax))


def smooth_joints(wd, x, h=FD_H):
    """joints whose four extrema are differentiable in x_i on [x_i - 2h, x_i + 2h] (away from the kinks
    x = 0, t_mm in {0, 0.5}, q_peak = q0, q_stop = q_peak, q_dot_peak in {0, qd0}), with a flag: the
    interior extremum -qd0 / k_actual is active there"""
    q0, qd0, _, _, kr, _ = wd
    out = []
    for i in range(7):
        if abs(x[i]) <= 4 * h or abs(x[i]) > 1 - 2 * h:
            continue
        sig = [_signature(q0[i], qd0[i], kr[i] * (x[i] + d)) for d in (-2 * h, -h, 0.0, h, 2 * h)]
        if any(s != sig[0] for s in sig):
            continue
        # ties between candidates that move differently with ka are kinks; a start at rest ties qd0 with the
        # final 0 for every ka, which is none
        tie = False
        for k, ties in sig[0][2:]:
            tie |= len(ties) > 0 and not (qd0[i] == 0.0)
        if tie:
            continue
        out.append((i, bool(sig[0][1])))
    return out


def check_extremum_jacobian(ev, wd, x, label=""):
    """J[-28:, i] k_range[i] against the central difference of the MODEL's extrema in x_i. The factor
    stays: the reference differentiates in k_actual = k_range x, not in x (ACMP/Trajectory.cu:229-383),
    and this project keeps that. Returns (worst error, joints compared, of which on the interior branch)."""
    q0, qd0, _, _, kr, _ = wd
    J = ev.eval(x)[1]
    worst, n, n_in = 0.0, 0, 0
    for i, interior in smooth_joints(wd, x):
        e = np.zeros(7)
        e[i] = FD_H
        # the derivative does not depend on q0: difference the extrema of q - q0, which do not carry the
        # ulp of a start many turns out
        z = np.zeros(7)
        fd = (M.extrema(z, qd0, kr, x + e) - M.extrema(z, qd0, kr, x - e)) / (2 * FD_H)      # [4, 7]
        Ji = J[-28:, i].reshape(4, 7) * kr[i]
        err = float(np.abs(Ji - fd).max())
        assert err <= FD_TOL, (label, i, "extremum Jacobian", Ji[:, i], fd[:, i])
        worst, n, n_in = max(worst, err), n + 1, n_in + int(interior)
    return worst, n, n_in


def check_collision_jacobian(ev, wd, x, label=""):
    """the collision rows' Jacobian against central differences of g itself, where no row changes its
    winning plane between x - h and x + h (rows whose two one-sided differences agree)"""
    g, J = ev.eval(x)[:2]
    if g.size == 28:
        return 0.0, 0
    worst, n = 0.0, 0
    for i in range(7):
        if abs(x[i]) > 1 - 2 * FD_H:
            continue
        e = np.zeros(7)
        e[i] = FD_H
        gp, gm = ev.eval(x + e)[0][:-28], ev.eval(x - e)[0][:-28]
        fwd, bwd = (gp - g[:-28]) / FD_H, (g[:-28] - gm) / FD_H
        ok = np.abs(fwd - bwd) < 1e-4      # a max over planes: one-sided slopes differ where the winner changes
        err = np.abs((gp - gm) / (2 * FD_H) - J[:-28, i])[ok]
        assert ok.mean() > 0.9, (label, i, ok.mean())
        assert err.max() <= FD_TOL, (label, i, "collision Jacobian", err.max())
        worst, n = max(worst, float(err.max())), n + int(ok.sum())
    return worst, n


# ---- radius-free containment --------------------------------------------------------------------
def radius_free_excess(ev, robot, wd, x, sign=1.0):
    """[7, T] worst excess over the 8 corners of the affine model's link boxes, evaluated at sign * x,
    over the evaluator's link zonotopes sliced at x (crafted tables: radius 0)"""
    q0, _, _, tab, _, _ = wd
    lc = ev.eval(x)[2]
    gens = ev.gens()
    C, S = M.sliced_cos_sin(tab, q0, sign * np.asarray(x))
    pts = M.affine_link_points(robot, C, S)                                   # [7, T, 8, 3]
    exc = PM.zonotope_excess(lc.transpose(1, 0, 2), gens.transpose(1, 0, 2, 3), pts)
    return np.asarray(exc).max(axis=-1)


def crafted_points(seed=0):
    rng = np.random.default_rng(77 + seed)
    return [np.zeros(7), rng.uniform(-1, 1, 7), np.ones(7), -np.ones(7)]


def check_radius_free(ev, robot, wd, slack):
    """every corner of the affine model lies in the sliced link zonotope; returns the worst excess"""
    worst = -np.inf
    for x in crafted_points():
        e = float(radius_free_excess(ev, robot, wd, x).max())
        assert e <= slack, ("affine model outside the link zonotope", e, x)
        worst = max(worst, e)
    return worst


def check_sensitivity(ev, robot, wd):
    """the model at -x lies outside by more than 1 cm in more than half of the (interval, link) samples at
    |x| = 1, so the radius-free check cannot go blind; returns [(samples out, largest excess)]"""
    out = []
    for x in (np.ones(7), -np.ones(7)):
        e = radius_free_excess(ev, robot, wd, x, sign=-1.0)                   # [7, T]
        n = int((e > 0.01).sum())
        assert n > e.size // 2, ("the containment check would pass a negated slice", n, e.size)
        out.append((n, float(e.max())))
    return out
