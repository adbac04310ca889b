"""Generator of tests/golden/degenerate_roots.npz: start states and trajectory parameters on and next to
the surface 6 T qd0 + T^2 qdd0 = 12 k, where the quadratic whose roots are the interior critical points
of the desired trajectory loses its leading coefficient (reach.h q_roots / qd_roots / qdd_roots_k0), with
exact values from mpmath at 100 digits stored as (hi, lo) pairs (value = hi + lo) so that the tests
(tests/degenerate_roots.py) need no mpmath.

    python tests/golden/make_degenerate_roots.py        # rewrites the fixture (needs mpmath)

The trajectory is the degree-5 Bernstein curve on the control points of tests/point_model.control_points
(KPR/Trajectory.cu:554-559) with the built-in Kinova's duration and k_range; every input is taken as the
exact value of its double.

Start-state cases (k-independent part, jrs_joint): q0 x qd0 x delta with qdd0 D = -6 qd0 (1 + delta), at
(T, step) pairs whose interval holds a critical time (on the surface these are 1/4, 1/2 and 3/4 for q, qd
and qdd). Samples of a (case, step): the critical times of q, qd and qdd at k = 0 inside the interval
(roots of the derivative polynomials, rounded to double), the interval's ends and its midpoint, each at
khat in {-1, 0, 1}. The exact values are cos and sin of q + e qe for e = -1, +1 and the bare rates qd,
qdd: the tests form qd + e qde and qdd + e qddae in long double (one rounding at 2^-64, the constants
being doubles).

Row cases (extremum rows of g): start states with x on its own surface k_range x = (6 T qd0 + T^2 qdd0)
/ 12 (1 + delta), and controls away from it. Per case and kind (position, velocity): the exact minimum
and maximum over t in [0, 1], where each is attained and its derivative with respect to x (envelope
theorem: k_range B345(t*) for position, k_range 30 t*^2 (1 - t*)^2 / D for velocity). Two flags per
(case, kind) for the gradient check only: the two interior critical points within 1e-3 of each other;
the best two candidates of the minimum or of the maximum within 1e-12 in value with an interior point
among them (which of them wins is then decided by rounding, and their derivatives differ). A tie of the
two end points t = 0 and t = 1 is no flag: row_alt and row_alt_time hold the other end's derivative and
time, and a test accepts either. At most 15 % of the row cases carry a flag (asserted below).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
PATH = os.path.join(HERE, "degenerate_roots.npz")

from make_jrs_samples import JOINT, K_RANGE, QDAE, QDDAE, QDE, QE  # noqa: E402  (the built-in Kinova's constants)

D = 1.0   # armour-dev_amd/csrc/robots.cpp: duration
DELTAS = [0.0] + [s * d for d in (2.0 ** -50, 2.0 ** -44, 2.0 ** -36, 2.0 ** -28, 2.0 ** -16, 1e-3) for s in (1.0, -1.0)]
# ---- start states ----
Q0S = [0.3, np.pi / 2 - 0.04, -2.9]
QD0S = [0.6, 0.25, -1.0, 1e-3]
T_STEPS = [(7, 1), (7, 3), (7, 5), (10, 2), (10, 7)]
KHATS = (-1.0, 0.0, 1.0)
ES = (-1.0, 1.0)
NS = 6    # sample times per (case, step): up to three critical times, two ends, the midpoint
# ---- rows ----
ROW_STATES = [(0.3, 0.25, 0.0), (-1.1, 0.6, -0.8), (2.0, -1.0, 1.0), (0.5, 0.0, 0.7)]
CONTROL_XS = [0.0, 0.37, -0.37, 1.0, -1.0]
CLOSE_ROOTS = 1e-3
CLOSE_VALUES = 1e-12
FLAG_CAP = 0.15


def start_cases():
    """[n, 5] (q0, qd0, qdd0, T, step)"""
    out = []
    for q0 in Q0S:
        for qd0 in QD0S:
            for d in DELTAS:
                qdd0 = -6.0 * qd0 * (1.0 + d) / D
                for T, s in T_STEPS:
                    out.append((q0, qd0, qdd0, T, s))
    return np.array(out, dtype=np.float64)


def scaled_state(q0, qd0, qdd0):
    """qd0 halved until the surface's x lies in [-1, 1]"""
    while abs((6 * qd0 * D + qdd0 * D * D) / 12 / K_RANGE) > 1.0:
        qd0 *= 0.5
    return q0, qd0, qdd0


def row_cases():
    """([m, 4] (q0, qd0, qdd0, x), [m] kind of case: 0 surface family, 1 control)"""
    out, kind = [], []
    for st in ROW_STATES:
        q0, qd0, qdd0 = scaled_state(*st)
        ks = (6 * qd0 * D + qdd0 * D * D) / 12
        assert abs(ks / K_RANGE) <= 1.0
        for d in DELTAS:
            x = ks * (1.0 + d) / K_RANGE
            if abs(x) > 1.0:   # a delta that steps over the box's edge keeps its size on the inner side
                x = ks * (1.0 - d) / K_RANGE
            assert abs(x) <= 1.0
            out.append((q0, qd0, qdd0, x))
            kind.append(0)
        for x in CONTROL_XS:
            out.append((q0, qd0, qdd0, x))
            kind.append(1)
    for x in (0.0, 0.5):      # at rest
        out.append((0.3, 0.0, 0.0, x))
        kind.append(1)
    # a double root of dq/dt: 64 a^2 + 14 a b - 120 k a + b^2 = 0 at a = T qd0 = 0.05, b = T^2 qdd0 = 0.1
    a, b = 0.05, 0.1
    k = (64 * a * a + 14 * a * b + b * b) / (120 * a)
    out.append((0.4, a / D, b / D / D, k / K_RANGE))
    kind.append(1)
    assert abs(out[-1][3]) <= 1.0
    return np.array(out, dtype=np.float64), np.array(kind, dtype=np.int32)


def _pair(x):
    hi = float(x)
    return hi, float(x - hi)


def generate():
    import mpmath as mp

    mp.mp.dps = 100
    f = mp.mpf

    def curve(q0, qd0, qdd0, k):
        """control points and the Bernstein coefficients of the first three derivatives (in t, duration 1
        scale: a = qd0 D, b = qdd0 D^2)"""
        a, b = f(qd0) * f(D), f(qdd0) * f(D) * f(D)
        p = [f(q0), f(q0) + a / 5, f(q0) + 2 * a / 5 + b / 20, f(q0) + k, f(q0) + k, f(q0) + k]
        d1 = [5 * (p[n + 1] - p[n]) for n in range(5)]
        d2 = [4 * (d1[n + 1] - d1[n]) for n in range(4)]
        d3 = [3 * (d2[n + 1] - d2[n]) for n in range(3)]
        return p, d1, d2, d3

    def bern(c, t):
        n = len(c) - 1
        return mp.fsum(mp.binomial(n, m) * t ** m * (1 - t) ** (n - m) * c[m] for m in range(n + 1))

    def power_basis(c):
        """coefficients by rising power of t of the Bernstein polynomial with coefficients c"""
        n = len(c) - 1
        out = [f(0)] * (n + 1)
        for m in range(n + 1):
            for j in range(n - m + 1):
                out[m + j] += mp.binomial(n, m) * c[m] * mp.binomial(n - m, j) * (-1) ** j
        return out

    def critical_times(c, lo, hi, strict):
        """real roots of the Bernstein polynomial c inside (lo, hi) (strict) or [lo, hi], besides the
        roots at t = 1 that the trailing zero coefficients are: mpmath's polyroots on the deflated
        polynomial at the working precision"""
        c = list(c)
        while c and c[-1] == 0:
            c = c[:-1]   # a zero last Bernstein coefficient is a factor (1 - t): c(t) = (1 - t) c'(t)
            n = len(c)
            c = [c[m] * mp.binomial(n, m) / mp.binomial(n - 1, m) for m in range(n)] if n else []
        if not c:
            return []
        pw = power_basis(c)
        while pw and pw[-1] == 0:
            pw = pw[:-1]
        if len(pw) < 2:
            return []
        scale = max(abs(v) for v in pw)
        roots = mp.polyroots([v / scale for v in reversed(pw)], maxsteps=2000, extraprec=2000)
        out = []
        for r in roots:
            if abs(mp.im(r)) > mp.mpf(10) ** -40 * (1 + abs(r)):
                continue
            r = mp.re(r)
            inside = (lo < r < hi) if strict else (lo <= r <= hi)
            if inside:
                out.append(r)
        return sorted(out)

    # ---- start states ----
    sc = start_cases()
    times = np.zeros((len(sc), NS))
    exact = np.zeros((len(sc), NS, len(KHATS), 6, 2))   # cos(e=-1), cos(e=+1), sin(e=-1), sin(e=+1), qd, qdd
    ncrit = np.zeros(len(sc), dtype=np.int32)
    for i, (q0, qd0, qdd0, T, s) in enumerate(sc):
        ds = 1.0 / T                       # as jrs_joint forms the interval's ends
        lo, hi = s * ds, (s + 1) * ds
        _, d1, d2, d3 = curve(q0, qd0, qdd0, f(0))
        ts = []
        for c in (d1, d2, d3):
            ts += [float(r) for r in critical_times(c, f(lo), f(hi), True)]
        ts = [t for t in ts if lo < t < hi]
        ncrit[i] = len(ts)
        assert len(ts) <= 3, (sc[i], ts)
        ts = ts + [lo, hi, 0.5 * (lo + hi)]
        ts = ts + [lo] * (NS - len(ts))    # unused slots repeat the lower end
        times[i] = ts
        for j, t in enumerate(ts):
            for n, kh in enumerate(KHATS):
                p, e1, e2, _ = curve(q0, qd0, qdd0, f(kh) * f(K_RANGE))
                q = bern(p, f(t))
                vals = [mp.cos(q - f(QE)), mp.cos(q + f(QE)), mp.sin(q - f(QE)), mp.sin(q + f(QE)),
                        bern(e1, f(t)) / f(D), bern(e2, f(t)) / f(D) / f(D)]
                for m, v in enumerate(vals):
                    exact[i, j, n, m] = _pair(v)
    # every surface case holds its critical time
    on = np.array([abs(c[2] * D + 6 * c[1]) <= 2e-3 * abs(6 * c[1]) for c in sc])
    assert np.all(ncrit[on] >= 1), sc[on][ncrit[on] < 1]

    # ---- rows ----
    rc, rkind = row_cases()
    rex = np.zeros((len(rc), 2, 2, 3, 2))      # [case, kind, min/max, (value, time, d/dx), (hi, lo)]
    alt = np.zeros((len(rc), 2, 2))            # the tying end point's derivative (else the same)
    alt_t = np.zeros((len(rc), 2, 2))          # and its time (else the same)
    flags = np.zeros((len(rc), 2, 2), dtype=bool)   # [case, kind, (close roots, close values)]
    scale = np.zeros((len(rc), 2))             # S of the value tolerance
    for i, (q0, qd0, qdd0, x) in enumerate(rc):
        k = f(K_RANGE) * f(x)
        p, d1, d2, _ = curve(q0, qd0, qdd0, k)
        scale[i, 0] = max(1.0, float(mp.fsum(abs(v) for v in p)))
        scale[i, 1] = max(1.0, float(mp.fsum(abs(v) for v in d1))) / D    # d1 = 5 x the control differences
        for kind, (val, der) in enumerate(((p, d1), (d1, d2))):
            inner = critical_times(der, f(0), f(1), True)
            # a double root shows as two roots a rounding apart: they are close, and flagged as such
            flags[i, kind, 0] = any(abs(inner[n + 1] - inner[n]) <= CLOSE_ROOTS for n in range(len(inner) - 1))
            cand = [f(0), f(1)] + inner
            v = [bern(val, t) / (f(D) if kind else 1) for t in cand]
            if kind == 0:
                dv = [f(K_RANGE) * t ** 3 * (6 * t * t - 15 * t + 10) for t in cand]
            else:
                dv = [f(K_RANGE) * 30 * t * t * (1 - t) ** 2 / f(D) for t in cand]
            for mm, pick in enumerate((min, max)):
                order = sorted(range(len(cand)), key=lambda n: v[n], reverse=(pick is max))
                b0 = order[0]
                rex[i, kind, mm, 0] = _pair(v[b0])
                rex[i, kind, mm, 1] = _pair(cand[b0])
                rex[i, kind, mm, 2] = _pair(dv[b0])
                alt[i, kind, mm] = float(dv[b0])
                alt_t[i, kind, mm] = float(cand[b0])
                if len(order) > 1 and abs(v[order[1]] - v[b0]) <= CLOSE_VALUES:
                    if b0 < 2 and order[1] < 2 and not any(abs(v[n] - v[b0]) <= CLOSE_VALUES for n in order[2:]):
                        alt[i, kind, mm] = float(dv[order[1]])
                        alt_t[i, kind, mm] = float(cand[order[1]])
                    else:
                        flags[i, kind, 1] = True
    flagged = flags.any(axis=(1, 2))
    assert flagged.mean() <= FLAG_CAP, (int(flagged.sum()), len(rc), rc[flagged])
    return dict(start_cases=sc, start_times=times, start_exact=exact, start_ncrit=ncrit,
                row_cases=rc, row_kind=rkind, row_exact=rex, row_alt=alt, row_alt_time=alt_t, row_flags=flags, row_scale=scale,
                consts=np.array([JOINT, K_RANGE, D, QE, QDE, QDAE, QDDAE]), khats=np.array(KHATS), es=np.array(ES),
                deltas=np.array(DELTAS))


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
