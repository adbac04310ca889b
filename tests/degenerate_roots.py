"""The degenerate quadratic of the extremum roots — TEST INFRASTRUCTURE: the fixture
tests/golden/degenerate_roots.npz (written by tests/golden/make_degenerate_roots.py, which describes its
cases) unpacked for the host tests (tests/test_degenerate_roots.py) and the device tests
(tests/test_gpu_degenerate_roots.py), so that both assert the same things.

On 6 T qd0 + T^2 qdd0 = 12 k the quadratic whose roots are the interior critical points of the desired
trajectory loses its leading coefficient (reach.h q_roots / qd_roots / qdd_roots_k0, restated in
oracle/src/traj.cpp): one root leaves through infinity, and the other was a cancelled numerator over a
vanishing denominator. The start-state cases put jrs_joint (k = 0) there, the row cases the extremum rows
of g and their Jacobian (k = k_range x).
"""
import os

import numpy as np

import domain_edges as DE
import jrs_unit as U

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "degenerate_roots.npz")
LD = np.longdouble
T, O = DE.T, DE.O
NF = 7
ULP = 2.0 ** -52
ROW_TOL = 16 * ULP      # times S (row_scale): |row - exact|
JAC_TOL = 1e-9          # the project's bar on a Jacobian entry
_FX = None


def fixture():
    global _FX
    if _FX is None:
        _FX = dict(np.load(FIXTURE))
    return _FX


def consts():
    c = fixture()["consts"]
    return dict(joint=int(c[0]), k_range=c[1], D=c[2], qe=c[3], qde=c[4], qdae=c[5], qddae=c[6])


# ---- start states: jrs_joint -----------------------------------------------------------------------
def start_samples():
    """(cases [n, 5] = q0, qd0, qdd0, T, step; khat [n, p]; exact [n, p, 4] long double = cos and sin of
    q + e qe, qd + e qde, qdd + e qddae), p = 6 times x 3 khat x 2 e, the quantities of
    jrs_unit.excess_of"""
    fx, c = fixture(), consts()
    ex = U._ld(fx["start_exact"])                     # [n, times, khat, 6]
    n, nt, nk, _ = ex.shape
    es = fx["es"]
    kh = np.broadcast_to(fx["khats"][None, None, :, None], (n, nt, nk, len(es)))
    out = np.zeros((n, nt, nk, len(es), 4), dtype=LD)
    for m, e in enumerate(es):
        out[..., m, 0] = ex[..., 0 + m]
        out[..., m, 1] = ex[..., 2 + m]
        out[..., m, 2] = ex[..., 4] + LD(e) * LD(c["qde"])
        out[..., m, 3] = ex[..., 5] + LD(e) * LD(c["qddae"])
    return fx["start_cases"], kh.reshape(n, -1), out.reshape(n, -1, 4)


def start_outputs(lib):
    """[n, 13]: the library's JRS scalars of every start-state case (one call per T)"""
    sc = fixture()["start_cases"]
    out = np.full((len(sc), 13), np.nan)
    for Tv in np.unique(sc[:, 3]):
        m = sc[:, 3] == Tv
        out[m] = lib.jrs(int(Tv), consts()["joint"], sc[m, 0], sc[m, 1], sc[m, 2], sc[m, 4].astype(np.int32))
    return out


def start_delta(cases=None):
    """[n] the relative distance |qdd0 D + 6 qd0| / |6 qd0| of every start-state case from the surface"""
    c = fixture()["start_cases"] if cases is None else cases
    return np.abs(c[:, 2] * consts()["D"] + 6 * c[:, 1]) / np.abs(6 * c[:, 1])


def check_start_enclosure(out, report):
    """jrs_unit.check_enclosure on the start-state cases; returns the worst excess [n, 4]"""
    cases, kh, ex = start_samples()
    return U.check_enclosure(out, cases, kh, ex, report)


def surface_world():
    """one world with every joint on the start-state surface: qd0 = +-0.25 alternating,
    qdd0 = -6 qd0 / D; position, goal and obstacles those of the base world"""
    q0, _, _, q_des, obs = DE.base_world()
    qd0 = 0.25 * np.array([1.0, -1.0, 1.0, -1.0, 1.0, -1.0, 1.0])
    return q0, qd0, -6.0 * qd0 / consts()["D"], q_des, obs


# ---- rows: extremum() and its gradient -------------------------------------------------------------
def row_worlds():
    """(worlds, X [W, 7], index [W, 7]): the row cases seven to a world, case index[w, j] on joint j (the
    extremum rows of a joint depend on that joint's state and x alone; the last world repeats cases), its
    x component on X[w, j]; goal 0.03 rad from the start, obstacles those of the base world"""
    rc = fixture()["row_cases"]
    W = -(-len(rc) // NF)
    index = (np.arange(W * NF) % len(rc)).reshape(W, NF)
    obs = DE.base_world()[4]
    worlds = [(rc[index[w], 0].copy(), rc[index[w], 1].copy(), rc[index[w], 2].copy(), rc[index[w], 0] + 0.03, obs.copy())
              for w in range(W)]
    return worlds, rc[index, 3].copy(), index


def row_slices(m):
    """the extremum rows of g [m]: position minima, position maxima, velocity minima, velocity maxima"""
    return [slice(m - 28 + 7 * n, m - 21 + 7 * n) for n in range(4)]


def row_expected(index_w):
    """for one world (index_w [7]): exact [4, 7] long double row values in the order of row_slices,
    tolerance [4, 7], and acc [4, 7, 2]: the derivatives with respect to x a row may report.

    The rows keep one convention of the reference: an extremum attained at t = 1 reports dq/dk = 1 for
    the velocity as for the position (nlp_kernels.hip extremum_grad, traj.cpp grad: id 4), though the
    velocity at t = 1 is 0 for every k. Such a row is never active (0 lies inside the speed limits). The
    fixture stores the true derivative, 0; at t = 1 this returns k_range / D for a velocity row."""
    fx, c = fixture(), consts()
    ex = U._ld(fx["row_exact"])[index_w]              # [7, kind, min/max, 3]
    val = np.zeros((4, NF), dtype=LD)
    tol = np.zeros((4, NF))
    acc = np.zeros((4, NF, 2))
    for kind in range(2):
        for mm in range(2):
            r = 2 * kind + mm
            val[r] = ex[:, kind, mm, 0]
            tol[r] = ROW_TOL * fx["row_scale"][index_w, kind]
            d = ex[:, kind, mm, 2].astype(np.float64)
            a = fx["row_alt"][index_w, kind, mm].copy()
            if kind == 1:
                d = np.where(ex[:, kind, mm, 1] == 1, c["k_range"] / c["D"], d)
                a = np.where(fx["row_alt_time"][index_w, kind, mm] == 1, c["k_range"] / c["D"], a)
            acc[r, :, 0], acc[r, :, 1] = d, a
    return val, tol, acc


def row_flagged(index_w):
    """[4, 7] bool: rows left out of the gradient check (fixture flags, per case and kind)"""
    f = fixture()["row_flags"][index_w].any(axis=2)   # [7, kind]
    return np.repeat(f.T, 2, axis=0)


def check_rows(g, J, index_w):
    """the extremum rows of g [m] and, if not None, of J [m, 7] of a world of row_worlds() evaluated at its
    row of X, against the fixture at the bars ROW_TOL * S and JAC_TOL (flagged cases left out of the
    gradient check; where the end points tie, either derivative). Returns (worst value error, the same in
    units of its tolerance, worst Jacobian error, misses): a miss is (what, case, row class, error, bar),
    a non-finite entry an infinite error."""
    val, tol, acc = row_expected(index_w)
    flagged = row_flagged(index_w)
    worst_v, worst_u, worst_j = 0.0, 0.0, 0.0
    bad = []
    for r, sl in enumerate(row_slices(len(g))):
        err = np.abs(LD(g[sl]) - val[r]).astype(np.float64)
        err = np.where(np.isfinite(err), err, np.inf)
        worst_v, worst_u = max(worst_v, err.max()), max(worst_u, (err / tol[r]).max())
        bad += [("value", int(index_w[j]), r, float(err[j]), float(tol[r, j])) for j in np.flatnonzero(err > tol[r])]
        if J is None:
            continue
        Jr = J[sl]
        off = Jr - np.diag(np.diag(Jr))
        bad += [("off-diagonal", int(index_w[j]), r, float(np.abs(off[j]).max()), 0.0)
                for j in np.flatnonzero(~(off == 0).all(axis=1))]
        jerr = np.abs(np.diag(Jr)[:, None] - acc[r]).min(axis=1)
        jerr = np.where(np.isfinite(jerr), jerr, np.inf)
        jerr = np.where(flagged[r], 0.0, jerr)
        worst_j = max(worst_j, jerr.max())
        bad += [("jacobian", int(index_w[j]), r, float(jerr[j]), JAC_TOL) for j in np.flatnonzero(jerr > JAC_TOL)]
    return worst_v, worst_u, worst_j, bad


def rows_violation(index_w, bounds):
    """the largest excess of the exact extremum rows of one world over the joint bounds
    (Planner.joint_bounds(): per joint [L, U] of its position rows, then of its velocity rows), and the
    tolerance that goes with it"""
    val, tol, _ = row_expected(index_w)
    L = np.stack([bounds[0:14:2], bounds[0:14:2], bounds[14:28:2], bounds[14:28:2]])
    Uu = np.stack([bounds[1:14:2], bounds[1:14:2], bounds[15:28:2], bounds[15:28:2]])
    v = np.maximum(LD(L) - val, val - LD(Uu))
    return float(v.max()), float(tol.max())
