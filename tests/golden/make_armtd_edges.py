"""Generate the ARMTD edge-world fixture tests/golden/armtd_edges.npz (build container, repo root; needs
the reference tree for the offline JRS files, read as data by tests/offline_jrs.py):

    python tests/golden/make_armtd_edges.py

Worlds (tests/armtd_edges.py describes what each is for; T = 100, O = 3 unless stated):

    rest, rest_kzero   qd0 = 0; rest_kzero's goal leaves joints 2 and 5 where q_plan(0) already is
    tiny               qd0 = (0.03, -0.03, 0.06, -0.06, h, -h, 1e-9), h = 0.5 k_range of h's own bin
    binedge            every qd0 the mean of two neighbouring C_KVI values
    fast               qd0 = (pi, -pi, 3, -3, 1.5, -1.5, 0.5): speed rows over the limit, status 4
    branch_a, branch_b q0 of the continuous joints on 0, pi/2, -pi/2, 3 pi and on +-1000 rad
    branch_a_turns     branch_a with its continuous joints SHIFT_TURNS whole turns on (q0 and q_des)
    limit_0.05, limit_0.001   joints 1, 3, 5 that far inside a position limit, moving towards it, the
                       goal beyond
    wrap               joint 0's goal exactly pi from q_plan(0)
    none               O = 0
    graze_rest         the rest start with its obstacles on the collision threshold

Obstacles are placed with the oracle (tests/boundary_worlds.tune_obstacle): "graze" obstacles so that
their largest collision value at x = 0 lies within 8e-4 of the threshold, the others 2 to 10 cm clear.
The tables are stored once per velocity bin. Outputs are the oracle's: status, feasible, iterations, k_opt,
cost, the count of collision rows within 1e-3 of the threshold at x = 0, and a SHA-1 of each world's inputs.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in ("armour-dev_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

import armtd_edges as E  # noqa: E402
import boundary_worlds as B  # noqa: E402
import offline_jrs as J  # noqa: E402
from armour_amd.robots import KINOVA  # noqa: E402
from oracle import OracleArmtd  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
T, O = E.T, 3
SHIFT_TURNS = 7
_CACHE = {}


def bin_of(v):
    return int(np.argmin(np.abs(v - J.C_KVI)))


def bin_table(b):
    if b not in _CACHE:
        _CACHE[b] = J.tables_from(J.load_jrs(J.C_KVI[b]))
    return _CACHE[b]


def half_range_speed():
    """h = 0.5 k_range(bin of h): t_mm = 0.5 exactly at x = -sign(qd0)"""
    h = 0.065
    for _ in range(8):
        h = 0.5 * bin_table(bin_of(h))[1]
    assert h == 0.5 * bin_table(bin_of(h))[1] == 0.5 * bin_table(bin_of(-h))[1]
    return h


def specs():
    rng = np.random.default_rng(4242)
    base_q0 = np.array([0.4, 0.5, -0.7, -1.0, 0.9, 0.3, -0.2])
    goal = lambda q0: q0 + rng.uniform(-0.012, 0.012, 7)
    out = []
    out.append(("rest", "plain", base_q0, np.zeros(7), goal(base_q0)))
    qd = goal(base_q0)
    qd[[2, 5]] = base_q0[[2, 5]]
    out.append(("rest_kzero", "plain", base_q0, np.zeros(7), qd))
    h = half_range_speed()
    out.append(("tiny", "graze", base_q0, np.array([0.03, -0.03, 0.06, -0.06, h, -h, 1e-9]), goal(base_q0)))
    mids = np.array([0.5 * (J.C_KVI[b] + J.C_KVI[b + 1]) for b in (200, 199, 210, 180, 230, 150, 260)])
    out.append(("binedge", "graze", base_q0, mids, goal(base_q0)))
    out.append(("fast", "plain", base_q0, np.array([np.pi, -np.pi, 3.0, -3.0, 1.5, -1.5, 0.5]), goal(base_q0)))
    qa = np.array([0.0, np.pi / 2, np.pi / 2, -np.pi / 2, -np.pi / 2, 0.0, 3 * np.pi])
    qda = rng.uniform(-0.1, 0.1, 7)
    ga = qa + 0.5 * qda + rng.uniform(-0.012, 0.012, 7)
    out.append(("branch_a", "plain", qa, qda, ga))
    qb = np.array([1000.0, -np.pi / 2, -1000.0, np.pi / 2, 3 * np.pi, 0.0, np.pi / 2])
    out.append(("branch_b", "plain", qb, rng.uniform(-0.1, 0.1, 7), goal(qb)))
    qs, gs = qa.copy(), ga.copy()
    qs[list(E.CONT)] += 2 * np.pi * SHIFT_TURNS
    gs[list(E.CONT)] += 2 * np.pi * SHIFT_TURNS
    out.append(("branch_a_turns", "plain", qs, qda, gs))
    for d in (0.05, 1e-3):
        q0, v, g = base_q0.copy(), np.zeros(7), goal(base_q0)
        for j, up in ((1, True), (3, False), (5, True)):
            q0[j] = KINOVA.state_ub[j] - d if up else KINOVA.state_lb[j] + d
            v[j] = 0.04 if up else -0.04
            g[j] = KINOVA.state_ub[j] + 0.2 if up else KINOVA.state_lb[j] - 0.2
        out.append((f"limit_{d:g}", "plain", q0, v, g))
    v = rng.uniform(-0.1, 0.1, 7)
    g = goal(base_q0)
    g[0] = base_q0[0] + 0.5 * v[0] + np.pi
    out.append(("wrap", "plain", base_q0, v, g))
    out.append(("none", "none", base_q0, rng.uniform(-0.1, 0.1, 7), goal(base_q0)))
    out.append(("graze_rest", "graze", base_q0, np.zeros(7), goal(base_q0)))
    return out


def main():
    rec = {k: [] for k in ("names", "kinds", "q0", "qd0", "q_des", "bins", "obstacles", "n_obs", "feasible", "status",
                           "iterations", "k_opt", "cost", "near_x0", "sha1")}
    worlds = specs()
    for s, (name, kind, q0, qd0, q_des) in enumerate(worlds):
        rng = np.random.default_rng(30_000 + s)
        bins = np.array([bin_of(v) for v in qd0])
        tab = np.array([bin_table(b)[0] for b in bins])
        kr = np.array([bin_table(b)[1] for b in bins])
        chk_tab, chk_kr = J.armtd_input(qd0)
        assert np.array_equal(tab, chk_tab) and np.array_equal(kr, chk_kr)
        x0 = np.zeros(7)
        n = 0 if kind == "none" else O
        obs = np.zeros((O, 12))
        if name == "branch_a_turns":   # the same obstacles as the unshifted world
            obs = rec["obstacles"][[w[0] for w in worlds].index("branch_a")].copy()
        elif n:
            R = OracleArmtd(q0, qd0, q_des, tab, kr, np.zeros((1, 12)), T=T, threads=8)
            R.reach()
            _, _, lc = R.eval(x0, centers=True)
            for k in range(n):
                target = B.COL_THR + rng.uniform(-8e-4, 4e-4) if kind == "graze" else -rng.uniform(0.02, 0.10)
                obs[k] = B.tune_obstacle(R, rng, lc, x0, T, 7, target, t_lo=0.5, nt=0)
        R = OracleArmtd(q0, qd0, q_des, tab, kr, obs[:n], T=T, threads=8)
        R.reach()
        g0 = R.eval(x0, jac=False)
        r = R.plan()
        for k, v in zip(("q0", "qd0", "q_des", "obstacles"), (q0, qd0, q_des, obs)):
            rec[k].append(np.asarray(v, dtype=np.float64))
        rec["names"].append(name)
        rec["kinds"].append(kind)
        rec["bins"].append(bins)
        rec["n_obs"].append(n)
        for k in ("feasible", "status", "iterations", "k_opt", "cost"):
            rec[k].append(r[k])
        rec["near_x0"].append(B.near_threshold_rows(g0, T, 7, n, nt=0) if n else 0)
        rec["sha1"].append(E.digest((q0, qd0, q_des, tab, kr, obs[:n])))
        print(f"{name:15s} {kind:6s} feasible={r['feasible']!s:5} status={r['status']} it={r['iterations']:3d} "
              f"near@x0={rec['near_x0'][-1]:4d} |k|max={np.abs(r['k_opt']).max():.4f} kr={np.round(kr, 3)}", flush=True)
    used = sorted({int(b) for bs in rec["bins"] for b in bs})
    remap = {b: i for i, b in enumerate(used)}
    out = {k: np.array(v) for k, v in rec.items()}
    out["bins"] = np.array([[remap[int(b)] for b in bs] for bs in rec["bins"]], dtype=np.int64)
    out["jrs_bin_c_kvi"] = J.C_KVI[used]
    out["jrs_tables"] = np.array([bin_table(b)[0] for b in used])
    out["jrs_k_range"] = np.array([bin_table(b)[1] for b in used])
    out["shift_turns"] = np.int64(SHIFT_TURNS)
    out["T"] = np.int64(T)
    np.savez_compressed(os.path.join(OUT, "armtd_edges.npz"), **out)
    print("bins stored:", len(used), "file bytes:", os.path.getsize(os.path.join(OUT, "armtd_edges.npz")))


if __name__ == "__main__":
    main()
