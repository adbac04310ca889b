"""Edges of the input domain — TEST INFRASTRUCTURE: deterministic case builders.

The generators (armour_amd.worlds.make_world, tests/boundary_worlds.start_state) draw continuous
joints in [-pi, pi], keep limited joints 0.2 rad clear of their limits, start speeds at or below half
the speed limit and goals within 0.8 pi/48 of the start. These builders leave those ranges, on the
built-in Kinova and the base world make_world(3, 3), at T = 10:

  * shift(n):       q0 and q_des of the continuous joints gain 2 pi n (multi-turn angles; the plan, the
                    link sets and every row but the continuous joints' position extrema do not change)
  * goal_shift(n):  only q_des gains 2 pi n (the wrapped cost does not change)
  * straddle(m):    q0 = m pi on the continuous joints (the branch points of cos / sin of an interval),
                    from rest and with the base world's rates
  * limit(j, d):    a limited joint starts d from its position limit (the state-limit rows active,
                    on the limit or infeasible)
  * speed(f):       joint 0 starts at f times its speed limit
  * far_goal:       goals on and beyond the wrap_to_pi tie and far enough to put every |k| on the box
"""
from __future__ import annotations

import numpy as np

from armour_amd.robots import KINOVA
from armour_amd.worlds import make_world

T, O = 10, 3
CONT = (0, 2, 4, 6)
LIMITED = (1, 3, 5)
SHIFTS = (1, -1, 7, -40, 150)
STRADDLES = (0, 0.5, -0.5, 1, -1, 2, 3.5)
TWO_PI = 2 * np.pi


def base_world():
    return tuple(np.array(v, dtype=np.float64) for v in make_world(3, O))


def _with(q0=None, qd0=None, qdd0=None, q_des=None):
    b = base_world()
    return (b[0] if q0 is None else q0, b[1] if qd0 is None else qd0, b[2] if qdd0 is None else qdd0,
            b[3] if q_des is None else q_des, b[4])


def shift(n):
    q0, _, _, q_des, _ = base_world()
    q0[list(CONT)] += TWO_PI * n
    q_des[list(CONT)] += TWO_PI * n
    return _with(q0=q0, q_des=q_des)


def goal_shift(n):
    q_des = base_world()[3]
    q_des[list(CONT)] += TWO_PI * n
    return _with(q_des=q_des)


def straddle(m, rest):
    q0 = np.zeros(7)
    q0[list(CONT)] = m * np.pi
    for j in LIMITED:
        v = m * np.pi
        q0[j] = v if (KINOVA.state_lb[j] + 0.3 <= v <= KINOVA.state_ub[j] - 0.3) else 0.0
    if rest:
        return _with(q0=q0, qd0=np.zeros(7), qdd0=np.zeros(7), q_des=q0 + 0.03)
    return _with(q0=q0, q_des=q0 + 0.03)


def limit(j, d, rest=False, lower=False):
    q0, _, _, q_des, _ = base_world()
    v = KINOVA.state_lb[j] + d if lower else KINOVA.state_ub[j] - d
    q0[j] = q_des[j] = v
    if rest:
        return _with(q0=q0, qd0=np.zeros(7), qdd0=np.zeros(7), q_des=q_des)
    return _with(q0=q0, q_des=q_des)


def speed(f):
    _, qd0, qdd0, _, _ = base_world()
    qd0[0] = f * KINOVA.speed_limits[0]
    qdd0[0] = 0.0
    return _with(qd0=qd0, qdd0=qdd0)


def _goal(changes):
    q0, _, _, q_des, _ = base_world()
    for j, d in changes:
        q_des[j] = q0[j] + d
    return _with(q_des=q_des)


def identity_cases():
    """[(name, world)]: the shift and straddle families (containment, parity, the shift identity)"""
    out = [("base", base_world())]
    out += [(f"shift{n:+d}", shift(n)) for n in SHIFTS]
    for m in STRADDLES:
        out.append((f"straddle{m:+g}_rest", straddle(m, True)))
        out.append((f"straddle{m:+g}_moving", straddle(m, False)))
    return out


def goal_shift_cases():
    return [(f"goal_shift{n:+d}", goal_shift(n)) for n in SHIFTS]


def limit_cases():
    out = []
    for j in LIMITED:
        for d in (0.05, 1e-3, 0.0, -1e-3):
            out.append((f"limit_j{j}_ub{d:+g}", limit(j, d)))
        out.append((f"limit_j{j}_lb+0.001", limit(j, 1e-3, lower=True)))
    for d in (0.05, 0.0125, 1e-3, 0.0):
        out.append((f"limit_j1_rest_ub{d:+g}", limit(1, d, rest=True)))
    return out


def speed_cases():
    return [(f"speed{f:+g}", speed(f)) for f in (0.8, 0.9, 0.999, 1.0, 1.001, -1.001)]


def far_goal_cases():
    return [("far_j0_plus_pi", _goal([(0, np.pi)])), ("far_j0_minus_pi", _goal([(0, -np.pi)])),
            ("far_j0_past_pi", _goal([(0, np.pi * (1 + 1e-12))])), ("far_j0_plus3", _goal([(0, 3.0)])),
            ("far_j2_minus3.3", _goal([(2, -3.3)])), ("far_j1_plus1", _goal([(1, 1.0)])),
            ("far_j3_minus2", _goal([(3, -2.0)])),
            ("far_all_half", _goal([(j, 0.5 if j % 2 == 0 else -0.5) for j in range(7)]))]


def plan_cases():
    """the limit, speed and far_goal families: one mixed-status batch (tests/golden/domain_edges.npz)"""
    return limit_cases() + speed_cases() + far_goal_cases()


def all_cases():
    return identity_cases() + goal_shift_cases() + plan_cases()
