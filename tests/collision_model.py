"""Model of the collision rows — TEST INFRASTRUCTURE, independent of the oracle (numpy only).

tests/point_model.py pins the link and torque sets to their definitions; this module does the same
for the collision rows of g. A row belongs to one (link, time step, obstacle): the link's sliced
zonotope c + sum_j b_j L_j (6 generators) against the obstacle c_obs + sum_i b_i O_i (3
generators). The reference buffers the obstacle by the link's generators (9 generators G: the
obstacle's 3, then the link's 6) and tests the point c against the 36 planes whose normals are the
normalised cross products of generator pairs (KPR/CollisionChecking.cu:136-299):

    g = -max_p max(+-n_p . (c - c_obs) - sum_j |n_p . G_j|)

A pair with a cross product of norm exactly 0 spans no plane: it is skipped and counts as -1e8.
g < 0 certifies separation (every unit n is a valid separating direction), and for 3-D zonotopes
the cross products hold every facet normal of the buffered obstacle, so g > 0 means the two sets
intersect. `intersects_lp` states that meaning without any plane: a linear program over the
generator coefficients. tests/test_zonotope_obstacles.py holds the model to it and the oracle to
the model; tests/test_gpu_zonotope_obstacles.py holds the HIP path to the model directly.

Shapes broadcast over leading dimensions: G [..., 9, 3], c and c_obs [..., 3].
"""
from __future__ import annotations

import numpy as np

EPS = 2.0 ** -52
SKIPPED = -1e8  # a skipped plane's candidates, and the scan's start value (CollisionChecking.cu:261-282)
SAME_NORMAL = 1e-9  # signed normals this close (max norm) are one plane: see row()
PAIRS = [(a, b) for a in range(9) for b in range(a + 1, 9)]  # a < b over the 9 buffered generators
_IA = np.array([a for a, _ in PAIRS])
_IB = np.array([b for _, b in PAIRS])


def buffered(obstacle_gens, link_gens):
    """[..., 9, 3] buffered generators from the obstacle's [..., 3, 3] (one generator per row) and
    the link's [..., 3, 6] (one generator per column, the layout of armour_get_link_generators)"""
    obstacle_gens, link_gens = np.asarray(obstacle_gens, dtype=np.float64), np.asarray(link_gens, dtype=np.float64)
    lead = np.broadcast_shapes(obstacle_gens.shape[:-2], link_gens.shape[:-2])
    return np.concatenate([np.broadcast_to(obstacle_gens, lead + (3, 3)),
                           np.broadcast_to(np.swapaxes(link_gens, -1, -2), lead + (6, 3))], axis=-2)


def _cross(G):
    a, b = G[..., _IA, :], G[..., _IB, :]
    x = a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1]
    y = a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2]
    z = a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]
    return np.stack([x, y, z], axis=-1), np.sqrt(x * x + y * y + z * z)


def planes(G):
    """[..., 36, 3] normalised cross products of the generator pairs a < b; a zero normal where the
    cross product's norm is exactly 0"""
    G = np.asarray(G, dtype=np.float64)
    cr, nrm = _cross(G)
    ok = nrm > 0
    return np.where(ok[..., None], cr / np.where(ok, nrm, 1.0)[..., None], 0.0)


def degenerate(G, factor=64.0):
    """[..., 36] pairs whose cross product is zero or rounding-level: |a x b| <= factor eps |a| |b|.
    Such a pair is parallel in exact arithmetic; its computed normal is an arbitrary unit vector
    (still a valid separating direction, but not one a restatement has to reproduce)."""
    G = np.asarray(G, dtype=np.float64)
    _, nrm = _cross(G)
    la = np.sqrt((G * G).sum(-1))
    return nrm <= factor * EPS * la[..., _IA] * la[..., _IB]


def row(c, c_obs, G, drop=None):
    """The collision row of link centre c against the obstacle centred at c_obs with buffered
    generators G. Returns a dict:
      g       -max over the 72 candidates (plane p's positive side, then its negative side);
      plane, negative   the winner under the first-maximum rule (strict >, scan from -1e8);
      normal  the winning plane's normal [..., 3];
      gap     winner minus the runner-up candidate (>= 0). Candidates whose signed normal equals the
              winner's to SAME_NORMAL are the winner's own plane met again through another generator
              pair (a link box generator along a coordinate axis is parallel to that axis's radius
              generator): whichever of them wins, the Jacobian row is the same, so the runner-up is
              the best candidate with a different signed normal;
      cand    the candidates [..., 72] (position 2 p + negative).
    drop [..., 36] (optional): planes to treat as skipped."""
    G = np.asarray(G, dtype=np.float64)
    N = planes(G)
    diff = np.asarray(c, dtype=np.float64) - np.asarray(c_obs, dtype=np.float64)
    proj = np.einsum("...pe,...e->...p", N, diff)
    delta = np.abs(np.einsum("...pe,...je->...pj", N, G)).sum(-1)
    live = (N != 0).any(-1)
    if drop is not None:
        live = live & ~drop
    cand = np.stack([np.where(live, proj - delta, SKIPPED), np.where(live, -proj - delta, SKIPPED)], axis=-1)
    cand = cand.reshape(cand.shape[:-2] + (72,))
    win = np.argmax(cand, axis=-1)                       # first maximum
    top = np.take_along_axis(cand, win[..., None], -1)[..., 0]
    none = ~(top > SKIPPED)                              # nothing beat the start value: plane 0, positive
    win = np.where(none, 0, win)
    plane = win // 2
    normal = np.take_along_axis(N, plane[..., None, None], -2)[..., 0, :]
    signed = np.stack([N, -N], axis=-2).reshape(N.shape[:-2] + (72, 3))
    outward = np.take_along_axis(signed, win[..., None, None], -2)
    rest = np.where((np.abs(signed - outward) <= SAME_NORMAL).all(-1), -np.inf, cand)
    return dict(g=-np.where(none, SKIPPED, top), plane=plane, negative=(win % 2).astype(bool), normal=normal,
                gap=top - rest.max(-1), cand=cand)


def jac_row(winner, dc_dx):
    """[..., 7] derivative of g: -n . dc/dx_k for a positive-side winner, +n . dc/dx_k for a
    negative-side one (winner: what row() returned; dc_dx [..., 7, 3])"""
    dot = np.einsum("...e,...ke->...k", winner["normal"], np.asarray(dc_dx, dtype=np.float64))
    return np.where(winner["negative"][..., None], dot, -dot)


def rounding_bound(c, c_obs, G):
    """256 eps (|c - c_obs|_1 + sum_j |G_j|_1): about 40 operations feed a row, each on quantities
    bounded by that sum (the normals are unit vectors), so this carries roughly 6x headroom"""
    diff = np.asarray(c, dtype=np.float64) - np.asarray(c_obs, dtype=np.float64)
    return 256 * EPS * (np.abs(diff).sum(-1) + np.abs(np.asarray(G, dtype=np.float64)).sum((-1, -2)))


def intersects_lp(c, c_obs, G):
    """The exact test, one pair (c, c_obs [3], G [9, 3]): maximise s subject to
    G^T b = c - c_obs, |b_i| <= 1 - s. The sets intersect iff s > 0 (s = 0: they touch). Returns s;
    -inf when c - c_obs is not in the span of the generators. Used by the CPU test only."""
    from scipy.optimize import linprog

    G = np.asarray(G, dtype=np.float64)
    n = G.shape[0]
    cost = np.zeros(n + 1)
    cost[n] = -1.0
    A_eq = np.concatenate([G.T, np.zeros((3, 1))], axis=1)
    b_eq = np.asarray(c, dtype=np.float64) - np.asarray(c_obs, dtype=np.float64)
    eye = np.eye(n)
    A_ub = np.concatenate([np.concatenate([eye, np.ones((n, 1))], 1), np.concatenate([-eye, np.ones((n, 1))], 1)])
    r = linprog(cost, A_ub=A_ub, b_ub=np.ones(2 * n), A_eq=A_eq, b_eq=b_eq, bounds=[(None, None)] * (n + 1),
                method="highs", options=dict(primal_feasibility_tolerance=1e-10, dual_feasibility_tolerance=1e-10))
    if r.status == 2:
        return -np.inf
    if r.status != 0:
        raise RuntimeError(f"linprog: {r.message}")
    return float(r.x[n])
