"""Robot tables the built-in Kinova and the Fetch fixture do not cover — TEST INFRASTRUCTURE.

"A robot is data" (include/armour_hip.h armour_robot, armour_amd.robot_tables) admits reversed joint
axes (code -a: the joint turns about -e_a, URDF <axis xyz="0 0 -1"/>), up to 9 joints and fixed
frames with any roll / pitch / yaw. The variants here are built from the committed tables only
(tests/golden/robot_fetch.json, robot_kinova_urdf.json and the built-in tables through the C ABI):

  KINOVA_REV   the built-in Kinova, joints 0, 3, 6 reversed
  FETCH_REV    Fetch, joints 1 (y, limits -1.221 / 1.518: the swap shows), 2 (continuous x), 5 (y)
               reversed
  KINOVA_9     the built-in Kinova + 2 fixed links with generic frames (9 joints, the most allowed)
  FETCH_9_REV  Fetch + 1 fixed link, joints 0, 4 reversed

The mirror identity the tests rest on needs no reference: robot B = reversed_robot(A, S) at
the state mirror_world(world, S) is robot A at the state `world`, joint angle for joint angle seen
about the same physical axes. Its links, and everything computed from them, are A's; its joint
quantities (k, q, qd, torques) are A's times sigma_j = -1 for j in S.
"""
from __future__ import annotations

import os

import numpy as np

from armour_amd import robot_tables as RT

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NF = 7
MAX_JOINTS = 9


def _norm(tables: dict) -> dict:
    """through the C structure and back: arrays shaped per joint, trimmed to num_joints"""
    return RT._shaped(RT.from_struct(RT.to_struct(tables)))


def kinova() -> dict:
    return RT.builtin(0)


def kinova_urdf() -> dict:
    return RT.load_json(os.path.join(GOLD, "robot_kinova_urdf.json"))


def fetch() -> dict:
    return RT.load_json(os.path.join(GOLD, "robot_fetch.json"))


def sigma(joints) -> np.ndarray:
    """[7] -1 on the joints of `joints`, +1 elsewhere"""
    s = np.ones(NF)
    s[list(joints)] = -1.0
    return s


def reversed_robot(base: dict, joints) -> dict:
    """`base` with the axes of `joints` reversed: the same mechanism described with those joint
    angles counted the other way, so the limits (lb, ub) become (-ub, -lb)"""
    r = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    for j in joints:
        assert 0 <= j < NF and r["axes"][j] != 0, j
        r["axes"][j] = -r["axes"][j]
        lb, ub = float(r["state_lb"][j]), float(r["state_ub"][j])
        r["state_lb"][j], r["state_ub"][j] = -ub, -lb
    return _norm(r)


def mirror_world(world, joints):
    """(q0, qd0, qdd0, q_des, obstacles) with the joint quantities of `joints` negated"""
    s = sigma(joints)
    q0, qd0, qdd0, q_des, obs = world
    return (s * np.asarray(q0), s * np.asarray(qd0), s * np.asarray(qdd0), s * np.asarray(q_des),
            np.array(obs, dtype=np.float64, copy=True))


def with_fixed_links(base: dict, n: int) -> dict:
    """`base` + n fixed joints (axis code 0) at the end of the chain, each with a non-zero offset, a
    generic (not axis-aligned) roll / pitch / yaw, a positive mass, an off-centre centre of mass, a
    full symmetric positive-definite inertia and a link box; the trailing zero `trans` row stays last"""
    nj = int(base["num_joints"])
    assert nj + n <= MAX_JOINTS
    r = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in base.items()}
    assert np.all(r["trans"][nj] == 0.0)
    for k in range(n):
        f = 1.0 + 0.5 * k
        trans = np.array([0.031, -0.017, 0.083]) * f
        rots = np.array([0.1, -0.2, 0.3]) * (1.0 if k % 2 == 0 else -1.3)
        com = np.array([0.012, -0.021, 0.034]) * f
        inertia = np.array([[2.1e-3, 2.0e-4, -1.0e-4], [2.0e-4, 1.7e-3, 3.0e-4], [-1.0e-4, 3.0e-4, 1.2e-3]]) * f
        assert np.all(np.linalg.eigvalsh(inertia) > 0)
        r["axes"] = np.append(r["axes"], 0)
        r["trans"] = np.vstack([r["trans"][:-1], trans, np.zeros(3)])
        r["rots"] = np.vstack([r["rots"], rots])
        r["mass"] = np.append(r["mass"], 0.4 * f)
        r["com"] = np.vstack([r["com"], com])
        r["inertia"] = np.concatenate([r["inertia"], inertia[None]])
        r["link_center"] = np.vstack([r["link_center"], np.array([0.004, -0.006, 0.03]) * f])
        r["link_generators"] = np.vstack([r["link_generators"], np.array([0.03, 0.025, 0.045]) * f])
        for name in ("friction", "damping", "armature"):
            r[name] = np.append(r[name], 0.0)
    r["num_joints"] = nj + n
    return _norm(r)


# name: (builder of the base tables, fixed links appended, reversed joints)
SPECS = {
    "KINOVA_REV": (kinova, 0, (0, 3, 6)),
    "FETCH_REV": (fetch, 0, (1, 2, 5)),
    "KINOVA_9": (kinova, 2, ()),
    "FETCH_9_REV": (fetch, 1, (0, 4)),
}
NAMES = tuple(SPECS)
_cache: dict = {}


def variant(name: str) -> dict:
    """the tables of one of NAMES (built once; the built-in Kinova tables come through the product
    library, so nothing is built at import)"""
    if name not in _cache:
        base, n_fixed, rev = SPECS[name]
        t = base()
        if n_fixed:
            t = with_fixed_links(t, n_fixed)
        if rev:
            t = reversed_robot(t, rev)
        _cache[name] = t
    return _cache[name]


def base_of(name: str) -> dict:
    """the variant's tables before its joints are reversed (its mirror partner)"""
    base, n_fixed, _ = SPECS[name]
    t = base()
    return with_fixed_links(t, n_fixed) if n_fixed else t


def __getattr__(name):   # KINOVA_REV, FETCH_REV, KINOVA_9, FETCH_9_REV as module attributes
    if name in SPECS:
        return variant(name)
    raise AttributeError(name)


# ---- the mirror identity -------------------------------------------------------------------------
# Shapes and cases shared by the oracle's (test_robot_variants.py) and the GPU's
# (test_gpu_robot_variants.py) mirror tests. case: (tables of A, reversed joints S, world seeds of
# armour_amd.make_world's default profile at MIRROR_O obstacles).
#
# The evaluation lines of the identity hold at every x but x_j = 0 for a limited joint j of S: there
# q_j(0) = q_j(1) = q0_j ties the two end candidates of the position extremum, the reference breaks
# the tie one way for the minimum and the other way for the maximum (KPR/Trajectory.cu:256-397 as
# oracle/src/traj.cpp extremum(): the minimum takes t = 1 with dq/dk = 1, the maximum t = 0 with
# dq/dk = 0), and the mirror exchanges minimum and maximum. Both are subgradients of the same kink.
# So MIRROR_X avoids zeros. The solver, however, starts at x = 0: its first Jacobian differs between
# A and B in those rows, the two solves take different paths, and with the solver's tolerances they
# stop 1e-9 to 1e-2 apart in k_opt on most worlds (oracle alone, seeds 40..399, farther apart than
# 1e-9: 342 of the 360 Kinova worlds, 359 of the 360 Fetch worlds; reversing a continuous joint alone
# leaves them within 3e-9). The seeds below are those where the oracle's two plans agree to 1e-9, ten
# times inside the bar, so that the test asks the same of the GPU.
# Each robot has two feasible worlds (status 0) and one infeasible world (status 4), except Fetch:
# of the default profile's seeds 0..12399 the oracle finds 32 infeasible Kinova worlds, and its two
# plans agree on one of them (11767; the others lie 2e-6 to 2.0 apart in k_opt); of seeds 0..13599 it
# finds no infeasible Fetch world at all, so Fetch has three feasible ones.
MIRROR_FEASIBLE = {"kinova": (True, True, False), "fetch": (True, True, True), "kinova9": (True, True, False)}
MIRROR_T, MIRROR_O = 20, 4
MIRROR_X = (np.array([0.5, -0.6, 0.7, 0.15, -0.5, 0.6, -0.7]), np.array([-0.93, 0.41, -0.08, -0.77, 0.29, 1.0, 0.64]))
MIRROR_CASES = {
    "kinova": (kinova, (0, 3, 6), (54, 268, 11767)),
    "fetch": (fetch, (0, 3, 6), (335, 628, 762)),
    "kinova9": (lambda: variant("KINOVA_9"), (1,), (51, 15, 44)),
}


def mirror_rows(T: int, NJ: int, O: int, joints):
    """(row map r', row sign rho) with g_B[r] = rho[r] g_A[r'[r]] for B = reversed_robot(A, joints) at
    the mirrored state and x_B = sigma x_A, over the rows [7T torque | NJ T O collision | 28 extremum]:
    torque rows keep their place and take sigma_j; collision rows are unchanged; of the extremum rows
    [min q, max q, min qd, max qd] (4 x 7), min and max of a reversed joint change places and sign"""
    m = 7 * T + NJ * T * O + 28
    rmap = np.arange(m)
    rho = np.ones(m)
    s = sigma(joints)
    rho[:7 * T] = np.tile(s, T)
    e0 = m - 28
    for j in joints:
        for lo in (0, 2):
            a, b = e0 + lo * 7 + j, e0 + (lo + 1) * 7 + j
            rmap[a], rmap[b] = b, a
            rho[a] = rho[b] = -1.0
    return rmap, rho


def mirrored_constraints(gA, JA, T: int, NJ: int, O: int, joints):
    """(g_B, J_B) that the identity predicts from A's: J_B[r, c] = rho_r sigma_c J_A[r', c]"""
    rmap, rho = mirror_rows(T, NJ, O, joints)
    s = sigma(joints)
    return rho * gA[rmap], rho[:, None] * s[None, :] * JA[rmap]


def mirror_eval_diffs(a: dict, b: dict, T: int, NJ: int, O: int, joints) -> dict:
    """largest absolute differences of every line of the identity after an evaluation of A at x and of
    B at sigma x. a, b: dict(centers [T, NJ, 3], gens [T, NJ, 3, 6], radius [T, 7], g [m], J [m, 7]).
    Also asserts that every collision decision (g > 1e-4) is identical."""
    gB, JB = mirrored_constraints(a["g"], a["J"], T, NJ, O, joints)
    nt, nc = 7 * T, NJ * T * O
    col = slice(nt, nt + nc)
    assert np.array_equal(a["g"][col] > 1e-4, b["g"][col] > 1e-4), "collision decisions differ"
    return dict(centers=np.abs(a["centers"] - b["centers"]).max(), gens=np.abs(a["gens"] - b["gens"]).max(),
                radius=np.abs(a["radius"] - b["radius"]).max(),
                torque=np.abs(gB[:nt] - b["g"][:nt]).max(), collision=np.abs(gB[col] - b["g"][col]).max() if nc else 0.0,
                extremum=np.abs(gB[nt + nc:] - b["g"][nt + nc:]).max(), jacobian=np.abs(JB - b["J"]).max())


def assert_mirror_plan(ra: dict, rb: dict, joints, tag=""):
    """plans of A and of its mirrored B: the same verdict, status and iteration count, the cost to
    rtol 1e-8, k_opt_B = sigma k_opt_A within 1e-8 (the bar of test_gpu_parity.
    test_rerun_bitwise_and_batch_position_stable for inputs that differ at rounding level)"""
    for f in ("feasible", "status", "iterations"):
        assert ra[f] == rb[f], (tag, f, ra[f], rb[f])
    np.testing.assert_allclose(rb["cost"], ra["cost"], rtol=1e-8, atol=1e-12, err_msg=str(tag))
    np.testing.assert_allclose(rb["k_opt"], sigma(joints) * ra["k_opt"], rtol=0, atol=1e-8, err_msg=str(tag))
