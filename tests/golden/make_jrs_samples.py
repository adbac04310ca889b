"""Generator of tests/golden/jrs_samples.npz: the sample points of tests/test_jrs_enclosure.py and
tests/test_interval_ops.py (icos / isin) with their exact values from mpmath at 50 digits, stored as
(hi, lo) double pairs (value = hi + lo to about 1e-32 relative) so that the tests need no mpmath.

    python tests/golden/make_jrs_samples.py        # rewrites the fixture (needs mpmath)

The trajectory is the degree-5 Bernstein curve on the control points of tests/point_model.control_points
(KPR/Trajectory.cu:554-559), duration 1; every input is taken as the exact value of its double.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
PATH = os.path.join(HERE, "jrs_samples.npz")

T = 10
JOINT = 0
PI = np.pi
Q0S = [0.0, PI / 2, -PI / 2, PI, -PI, 2 * PI, 3.5 * PI, 1 + 14 * PI, -2.5 - 80 * PI, 0.3 + 300 * PI, 999.0, -999.9]
RATES = [(0.0, 0.0), (0.6, -0.8), (-1.39, 1.0), (1e-9, 0.0), (0.0, 1e-9)]
STEPS = [0, 4, 5, 9]
# (position in the interval, k / k_range, e): the eight corners, then interior points
SAMPLES = [(a, b, c) for a in (0.0, 1.0) for b in (-1.0, 1.0) for c in (-1.0, 1.0)] + \
          [(0.5, 0.0, 0.0), (0.3, 0.7, -0.4), (0.8, -0.35, 0.9), (0.13, 0.99, 0.5)]
ICOS_WIDTHS = [1e-3, 1e-2, 0.05, 0.2]

# the built-in Kinova's constants as armour-dev_amd/csrc/robots.cpp computes them, in doubles
EPS = float(np.sqrt(2 * 1e-2 / 5.095620491878957))
K_GAIN = 5.0
QE, QDE, QDAE, QDDAE = EPS / K_GAIN, 2 * EPS, EPS, 2 * K_GAIN * EPS
K_RANGE = PI / 48


def cases():
    """[n, 4] (q0, qd0, qdd0, s) in the fixture's order"""
    return np.array([(q, r[0], r[1], s) for q in Q0S for r in RATES for s in STEPS], dtype=np.float64)


def sample_points(c):
    """[n, 12, 3] (t, khat, e) of every case: t inside [s / T, (s + 1) / T] as jrs_joint forms its ends"""
    ds = 1.0 / T
    out = np.zeros((len(c), len(SAMPLES), 3))
    for i, (_, _, _, s) in enumerate(c):
        lo, hi = s * ds, (s + 1) * ds
        for j, (a, kh, e) in enumerate(SAMPLES):
            out[i, j] = (min(hi, lo + a * (hi - lo)), kh, e)
    return out


def icos_intervals():
    """[m, 2] intervals around every q0: the widths of ICOS_WIDTHS and q0 +- 1e-15"""
    iv = []
    for q in Q0S:
        for w in ICOS_WIDTHS:
            iv.append((q - w / 2, q + w / 2))
        iv.append((q - 1e-15, q + 1e-15))
    return np.array(iv, dtype=np.float64)


def _pair(x):
    hi = float(x)
    return hi, float(x - hi)


def generate():
    import mpmath as mp

    mp.mp.dps = 50
    f = mp.mpf
    c = cases()
    pts = sample_points(c)
    exact = np.zeros(pts.shape[:2] + (4, 2))   # cos, sin, qd + e qde, qdd + e qddae as (hi, lo)
    for i, (q0, qd0, qdd0, _) in enumerate(c):
        for j, (t, kh, e) in enumerate(pts[i]):
            t, k = f(t), f(kh) * f(K_RANGE)
            b = [f(q0), f(q0) + f(qd0) / 5, f(q0) + 2 * f(qd0) / 5 + f(qdd0) / 20, f(q0) + k, f(q0) + k, f(q0) + k]
            d1 = [5 * (b[n + 1] - b[n]) for n in range(5)]
            d2 = [4 * (d1[n + 1] - d1[n]) for n in range(4)]
            bern = lambda n: [mp.binomial(n, m) * t ** m * (1 - t) ** (n - m) for m in range(n + 1)]
            q = mp.fsum(w * v for w, v in zip(bern(5), b))
            qd = mp.fsum(w * v for w, v in zip(bern(4), d1))
            qdd = mp.fsum(w * v for w, v in zip(bern(3), d2))
            a = q + f(e) * f(QE)
            for n, v in enumerate((mp.cos(a), mp.sin(a), qd + f(e) * f(QDE), qdd + f(e) * f(QDDAE))):
                exact[i, j, n] = _pair(v)
    iv = icos_intervals()
    rng = np.zeros((len(iv), 4, 2))             # cos min, cos max, sin min, sin max as (hi, lo)
    for i, (lo, hi) in enumerate(iv):
        for n, (fn, shift) in enumerate(((mp.cos, f(0)), (mp.sin, mp.pi / 2))):
            vals = [fn(f(lo)), fn(f(hi))]
            # extrema of cos(x - shift) at shift + m pi
            m = mp.ceil((f(lo) - shift) / mp.pi)
            while shift + m * mp.pi <= f(hi):
                vals.append(f(1) if int(m) % 2 == 0 else f(-1))
                m += 1
            rng[i, 2 * n] = _pair(min(vals))
            rng[i, 2 * n + 1] = _pair(max(vals))
    return dict(cases=c, points=pts, exact=exact, icos_intervals=iv, icos_range=rng,
                consts=np.array([T, JOINT, K_RANGE, QE, QDE, QDAE, QDDAE]))


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate())
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
