"""The fixed list of tracking rollouts the armour_track tests run — TEST INFRASTRUCTURE.

Shared by tests/test_track_unit.py (the host build of track.h against track_model), tests/test_track_model.py
(the list's admission condition) and tests/test_gpu_track.py (the device against track_model), so that
all three see the same rollouts. A case is (robot, shape (N, S), window): N random trajectories, and
for rollout (n, s) one of six kinds, (n + s) % 6 for s < 6:

  0  nominal parameters, zero err0
  1  every link at 1 + 0.03          2  every link at 1 - 0.03
  3  kind 1 with err0 of norm 0.6 qe in position     4  kind 2 with the same err0
  5  every link at 1.2 (outside the stated uncertainty)

and for s >= 6 scales uniform in [0.97, 1.03] per link with an err0 of norm 0.3 qe. The Fetch fixture
(zero armature, V_m = 1e-7) runs with nominal parameters and zero err0 only, on quasi-static
trajectories (FETCH_MOTION): with perturbed parameters, or at nominal parameters on a motion of
ordinary size, 50 steps chatter and the outputs are sensitive to one ulp of the inputs (DESIGN.md
section 4), so those rollouts fail the admission condition below and are deliberately not on the list.

Admission condition: the model's own spread under a one-ulp perturbation of every input (tables,
trajectories, scales, err0) stays below 1e-9 in every output. SPREAD is the largest spread per output
field over the whole list and 8 perturbation draws, measured with track_model on a CPU by
`PYTHONPATH=armour-dev_amd python tests/track_cases.py`; TOL = 100 x SPREAD is the tolerance of the device tests: the
perturbation stands for input rounding only, while the device also differs in sin / cos by an ulp or
two, over 200 chained stages.
"""
from __future__ import annotations

import numpy as np

import robot_variants as RV
import track_model as TM

NF = 7
SHAPES = ((3, 5), (5, 1), (1, 17))
WINDOWS = ((0.0, 0.5), (0.5, 1.0))
STEPS = 50
ROBOTS = ("kinova", "KINOVA_REV", "KINOVA_9", "fetch")
FIELDS = ("max_pos_err", "max_vel_err", "max_torque", "max_V", "max_robust", "end_state")

# measured: largest |perturbed - base| per field over every rollout of the list, 8 draws
SPREAD = {
    "max_pos_err": 2.22e-15, "max_vel_err": 7.77e-15, "max_torque": 9.50e-14, "max_V": 9.58e-16, "max_robust": 1.48e-13,
    "end_state": 7.77e-15,
}
TOL = {k: 100.0 * v for k, v in SPREAD.items()}
ADMISSION = 1e-9
# The Fetch rollouts are quasi-static: qd0, qdd0 and k of the random trajectories times this factor.
# With Fetch's own V_m = 1e-7 the robust term switches on at ||r|| = alpha V_m / ||rho||, about 3e-8,
# and the inner stages of an RK4 step sit h^2 qdd / 8 off the desired trajectory: at 50 steps any
# motion with |qdd| above about 1e-3 chatters (errors of 0.1 .. 1 rad) even with nominal parameters.
FETCH_MOTION = 1e-5


def tables(name):
    if name == "kinova":
        return RV.kinova()
    if name == "fetch":
        return RV.fetch()
    return RV.variant(name)


def qe_of(tb):
    return float(np.sqrt(2 * tb["V_m"] / tb["M_min"]) / tb["K"])


def trajectories(N, seed):
    """[N, 4, 7] q0, qd0, qdd0, k"""
    rng = np.random.default_rng(1000 + seed)
    t = np.zeros((N, 4, NF))
    t[:, 0] = rng.uniform(-1.0, 1.0, (N, NF))
    t[:, 1] = rng.uniform(-0.5, 0.5, (N, NF))
    t[:, 2] = rng.uniform(-0.5, 0.5, (N, NF))
    t[:, 3] = rng.uniform(-1.0, 1.0, (N, NF))
    return t


def samples(tb, N, S, seed, nominal_only=False):
    """(scale [N, S, 2, NJ], err0 [N, S, 2, 7]) of the kinds above"""
    nj = int(tb["num_joints"])
    qe = qe_of(tb)
    rng = np.random.default_rng(2000 + seed)
    scale = np.ones((N, S, 2, nj))
    err0 = np.zeros((N, S, 2, NF))
    d = rng.normal(size=NF)
    d /= np.linalg.norm(d)
    if nominal_only:
        return scale, err0
    for n in range(N):
        for s in range(S):
            if s < 6:
                kind = (n + s) % 6
                scale[n, s] = {0: 1.0, 1: 1.03, 2: 0.97, 3: 1.03, 4: 0.97, 5: 1.2}[kind]
                if kind in (3, 4):
                    err0[n, s, 0] = 0.6 * qe * d
            else:
                scale[n, s] = rng.uniform(0.97, 1.03, (2, nj))
                e = rng.normal(size=NF)
                err0[n, s, 0] = 0.3 * qe * e / np.linalg.norm(e)
    return scale, err0


def case_inputs(robot, shape, seed=None):
    """(tables, traj, scale, err0) of one (robot, shape)"""
    tb = tables(robot)
    N, S = shape
    seed = SHAPES.index(shape) if seed is None else seed
    traj = trajectories(N, seed)
    if robot == "fetch":
        traj[:, 1:] *= FETCH_MOTION
    scale, err0 = samples(tb, N, S, seed, nominal_only=(robot == "fetch"))
    return tb, traj, scale, err0


def flat_inputs(robot):
    """every rollout of `robot` over all SHAPES as one flat batch: (tables, traj [R, 4, 7], scale [R, 2, NJ],
    err0 [R, 2, 7], slices {shape: slice})"""
    tr, sc, e0, where, at = [], [], [], {}, 0
    for shape in SHAPES:
        tb, traj, scale, err0 = case_inputs(robot, shape)
        N, S = shape
        tr.append(np.repeat(traj, S, axis=0))
        sc.append(scale.reshape(N * S, 2, -1))
        e0.append(err0.reshape(N * S, 2, NF))
        where[shape] = slice(at, at + N * S)
        at += N * S
    return tb, np.concatenate(tr), np.concatenate(sc), np.concatenate(e0), where


_REF = {}


def reference(robot, window):
    """track_model's outputs for every rollout of (robot, window), {shape: dict of [N, S, ...]}; computed once"""
    key = (robot, window)
    if key not in _REF:
        tb, traj, scale, err0, where = flat_inputs(robot)
        out = TM.Rollouts(tb, traj, scale, err0).run(window[0], window[1], STEPS)
        _REF[key] = {shape: {k: v[sl].reshape(shape + v.shape[1:]) for k, v in out.items()} for shape, sl in where.items()}
    return _REF[key]


def _ulp(x, rng):
    x = np.asarray(x, dtype=np.float64)
    return np.nextafter(x, np.where(rng.integers(0, 2, x.shape) == 1, np.inf, -np.inf))


def perturbed_tables(tb, rng):
    """every floating-point table entry moved by one ulp in a random direction (limits, which only
    classify joints as continuous, and the link boxes, which tracking does not read, stay)"""
    out = dict(tb)
    for k in ("trans", "rots", "mass", "com", "inertia", "damping", "armature"):
        out[k] = _ulp(tb[k], rng)
    for k in ("mass_uncertainty", "inertia_uncertainty", "gravity", "alpha", "V_m", "K"):
        out[k] = float(_ulp(tb[k], rng))
    return out


def measure_spread(draws=8, robots=ROBOTS, windows=WINDOWS, report=print):
    """{field: largest spread} over the list"""
    worst = {k: 0.0 for k in FIELDS}
    for robot in robots:
        tb, traj, scale, err0, _ = flat_inputs(robot)
        for window in windows:
            base = TM.Rollouts(tb, traj, scale, err0).run(window[0], window[1], STEPS)
            assert not base["status"].any(), (robot, window)
            here = {k: 0.0 for k in FIELDS}
            for d in range(draws):
                rng = np.random.default_rng(7000 + d)
                out = TM.Rollouts(perturbed_tables(tb, rng), _ulp(traj, rng), _ulp(scale, rng), _ulp(err0, rng)).run(
                    window[0], window[1], STEPS)
                for k in FIELDS:
                    here[k] = max(here[k], float(np.abs(out[k] - base[k]).max()))
            report(f"{robot:11s} [{window[0]}, {window[1]}] " + " ".join(f"{k} {here[k]:.2e}" for k in FIELDS))
            for k in FIELDS:
                worst[k] = max(worst[k], here[k])
    return worst


if __name__ == "__main__":
    w = measure_spread()
    print("SPREAD = {" + ", ".join(f'"{k}": {v:.2e}' for k, v in w.items()) + "}")
