"""The fixed list of armour_track_motion cases — TEST INFRASTRUCTURE, shared by tests/test_tracked_model.py
(the conditions the list has to meet, on the CPU) and tests/test_gpu_track_motion.py (the device against
tests/tracked_model.py), so that both see the same inputs.

Main list: the rollouts of tests/track_cases.py (shapes (W, S) = (3, 5), (5, 1), (1, 17), the six kinds of
sample, 50 steps) on the Kinova, KINOVA_REV and KINOVA_9, one trajectory per world. World w carries
COUNTS[w] = 3, 0, 1, 3, 1 obstacles: boxes with a random centre, sides of 5 .. 30 cm and a random
orientation (no generator is parallel to a link generator, so no pair's normal is an arbitrary unit
vector: the `fragile` pairs of episode_model.separations do not occur, and the CPU test asserts that).
Windows: "first" [0, 0.5] and "second" [0.5, 1] with the list's err0, and "chained": [0.5, 1] started
from the end state of "first" (err0 = end state - desired state at 0.5, each side from its own end state).
check_samples 2, 11 and 51 are check points c * stride of the same rollout, so one model run with 51
serves all three.

Flag cases (FLAG_CASES): one world, a few samples, each built so that one flag's quantity sits far from
its threshold (asserted on the CPU, not filtered at run time).

Tolerances, by the project's rule (tests/track_cases.py): 100 x the model's own largest
spread under a one-ulp perturbation of every input (tables with the link boxes, trajectories, scales,
err0, obstacles), 8 draws, over the whole main list with the chained window. The rollouts' own fields
are track_model's, measured there (track_cases.TOL); measured here with tracked_model by
`PYTHONPATH=armour-dev_amd python tests/tracked_cases.py`:

    robot       rec (q, qd)   clearance
    kinova      5.6e-16       8.9e-16
    KINOVA_REV  8.9e-16       7.5e-16
    KINOVA_9    6.1e-16       7.3e-16

The clearance additionally gets the rounding bound of its pair (tracked_model.state_clearance: bound).
`where` is compared where the model's runner-up exceeds twice that tolerance, which the CPU test asserts
for every rollout of the list.
"""
from __future__ import annotations

import numpy as np

import point_model as pm
import track_cases as TC
import track_model as TM
import tracked_model as KM

NF = 7
SHAPES = TC.SHAPES
STEPS = TC.STEPS
CHECKS = (2, 11, 51)
ROBOTS = ("kinova", "KINOVA_REV", "KINOVA_9")
WINDOWS = {"first": (0.0, 0.5), "second": (0.5, 1.0), "chained": (0.5, 1.0)}
COUNTS = (3, 0, 1, 3, 1)

# measured: largest |perturbed - base| over the main list, 8 draws (rec: the recorded states; clearance:
# per rollout, every check_samples)
SPREAD = {"rec": 8.88e-16, "clearance": 8.88e-16}
TOL = {k: 100.0 * v for k, v in SPREAD.items()}


def obstacles(W, seed):
    """a list of W arrays [COUNTS[w], 12]: centre, then three generators (rows of R' diag(half sides))"""
    rng = np.random.default_rng(3000 + seed)
    out = []
    for w in range(W):
        obs = np.zeros((COUNTS[w], 12))
        for o in range(COUNTS[w]):
            Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
            obs[o, :3] = rng.uniform([-0.6, -0.6, 0.1], [0.6, 0.6, 1.1])
            obs[o, 3:] = (Q * rng.uniform(0.025, 0.15, 3)[:, None]).reshape(-1)
        out.append(obs)
    return out


def case_inputs(robot, shape):
    """(tables, traj [W, 4, 7], scale, err0, obstacles) of one (robot, shape)"""
    tb, traj, scale, err0 = TC.case_inputs(robot, shape)
    return tb, traj, scale, err0, obstacles(shape[0], SHAPES.index(shape))


def worlds(traj, obs):
    """the batch armour_track_motion runs on: worlds at the trajectories' own states with these obstacles"""
    return [(traj[w, 0].copy(), traj[w, 1].copy(), traj[w, 2].copy(), traj[w, 0].copy(), obs[w]) for w in range(len(obs))]


def desired_state(traj, t):
    """[W, 2, 7] (q, qd) of the trajectories at t"""
    beta = pm.control_points(traj[:, 0], traj[:, 1], traj[:, 2], traj[:, 3] * TM.K_RANGE)
    q, qd, _ = pm.bezier(beta, t)
    return np.stack([q, qd], axis=1)


def chained_err0(traj, end_state):
    """the err0 [W, S, 2, 7] that continues rollouts which ended in end_state [W, S, 2, 7] at t = 0.5"""
    return end_state - desired_state(traj, 0.5)[:, None]


def subsample(robot, full, obs, C):
    """the outputs for check_samples = C from a model run with more (51 on the main list; the rollouts do
    not depend on C)"""
    stride = (full["rec"].shape[0] - 1) // (C - 1)
    W, S = full["status"].shape
    rec = full["rec"][::stride].reshape(C, W * S, 2, NF)
    flat = {k: full[k].reshape((W * S,) + full[k].shape[2:]) for k in TC.FIELDS + ("status",)}
    cl = [KM.state_clearance(robot, rec[:, r, 0], obs[r // S]) for r in range(W * S)]
    out = {k: full[k] for k in TC.FIELDS + ("status",)}
    out["clearance"] = np.array([c["clearance"] for c in cl]).reshape(W, S)
    out["where"] = np.array([c["where"] for c in cl], dtype=np.int32).reshape(W, S, 3)
    for k in ("runner_up", "bound", "fragile"):
        out[k] = np.array([c[k] for c in cl]).reshape(W, S)
    out["flags"] = KM.flags(robot, flat, rec, out["clearance"].reshape(-1)).reshape(W, S)
    out["margins"] = {bit: m.reshape(W, S) for bit, m in KM.flag_margins(robot, flat, rec).items()}
    first = np.argmin(out["clearance"], axis=1)
    out["world_clearance"] = out["clearance"][np.arange(W), first]
    ww = np.concatenate([first[:, None], out["where"][np.arange(W), first]], axis=1).astype(np.int32)
    ww[~np.isfinite(out["world_clearance"])] = -1
    out["world_where"] = ww
    out["rec"] = full["rec"][::stride]
    return out


def run_windows(tb, traj, scale, err0, obs):
    """{window name: the model's outputs with 51 check points}"""
    out = {}
    for name in ("first", "second"):
        t0, t1 = WINDOWS[name]
        out[name] = KM.track_motion(tb, traj, obs, scale, err0, t0, t1, STEPS, CHECKS[-1])
    out["chained"] = KM.track_motion(tb, traj, obs, scale, chained_err0(traj, out["first"]["end_state"]), 0.5, 1.0, STEPS,
                                     CHECKS[-1])
    return out


_REF = {}


def reference(robot, shape, window, C):
    """the model's outputs of one case; the rollouts are computed once per (robot, shape)"""
    if (robot, shape) not in _REF:
        _REF[(robot, shape)] = run_windows(*case_inputs(robot, shape))
    key = (robot, shape, window, C)
    if key not in _REF:
        tb, _, _, _, obs = case_inputs(robot, shape)
        _REF[key] = subsample(tb, _REF[(robot, shape)][window], obs, C)
    return _REF[key]


# ---- the long record --------------------------------------------------------------------------------
# More check points than a wave has lanes, so that the finish kernel's lane-strided loop takes a second
# trip (65) and a third (129): two Kinova worlds with 3 and 1 obstacles, 2 samples, 128 steps on [0, 0.5].
# The check points of 65 are the even ones of 129, so one model run serves both. The seed is fixed; the CPU
# test asserts the list's conditions (a unique minimiser among them) for it.
LONG_STEPS = 128
LONG_CHECKS = (65, 129)
LONG_WINDOW = (0.0, 0.5)
LONG_SEED = 11


def long_inputs():
    """(tables, traj [2, 4, 7], scale [2, 2, 2, NJ], err0 [2, 2, 2, 7], obstacles with 3 and 1 boxes)"""
    tb = TC.tables("kinova")
    scale, err0 = TC.samples(tb, 2, 2, LONG_SEED)
    obs = obstacles(3, LONG_SEED)
    return tb, TC.trajectories(2, LONG_SEED), scale, err0, [obs[0], obs[2]]


def long_reference(C):
    """the model's outputs of the long record with C check points; the rollouts are computed once"""
    if "long" not in _REF:
        tb, traj, scale, err0, obs = long_inputs()
        _REF["long"] = KM.track_motion(tb, traj, obs, scale, err0, LONG_WINDOW[0], LONG_WINDOW[1], LONG_STEPS, LONG_CHECKS[-1])
    if ("long", C) not in _REF:
        tb, _, _, _, obs = long_inputs()
        _REF[("long", C)] = subsample(tb, _REF["long"], obs, C)
    return _REF[("long", C)]


# ---- flag cases -----------------------------------------------------------------------------------
FLAG_CASES = ("collision", "bound", "position_limit", "speed_limit", "input")


def flag_case(name):
    """dict(tables, traj [1, 4, 7], scale, err0 [1, S, 2, 7], obstacles, window, C, bit, rollout: the
    sample that must raise `bit`, others: samples that must not raise it)"""
    tb = TC.tables("kinova")
    nj = int(tb["num_joints"])
    qe, qde = KM.thresholds(tb)
    S = 3
    traj = TC.trajectories(1, 50)
    scale = np.ones((1, S, 2, nj))
    scale[0, 1], scale[0, 2] = 1.03, 0.97
    err0 = np.zeros((1, S, 2, NF))
    obs = [np.zeros((0, 12))]
    case = dict(window=(0.0, 0.5), C=11, rollout=1, others=(0, 2))
    if name == "collision":
        # a 10 cm cube centred on link 4's box at the start: every sample collides, deepest at check point 0
        import episode_model as E
        c, _ = E.link_boxes(KM._shaped(tb), traj[:, 0])
        ob = np.zeros((1, 12))
        ob[0, :3] = c[0, 4]
        ob[0, 3:] = (0.05 * np.eye(3)).reshape(-1)
        traj[0, 1:3] = 0.0
        obs, case["bit"], case["others"] = [ob], KM.COLLISION, ()
    elif name == "bound":
        err0[0, 1, 0, 2] = 1.5 * qe
        case["bit"] = KM.BOUND
    elif name == "position_limit":
        # joint 1 at rest 1e-3 inside its upper limit; sample 1 starts 2e-3 further out
        traj[0, 1:] = 0.0
        traj[0, 0, 1] = float(tb["state_ub"][1]) - 1e-3
        err0[0, 1, 0, 1] = 2e-3
        case["bit"] = KM.LIMIT
    elif name == "speed_limit":
        traj[0, 1:] = 0.0
        traj[0, 1, 3] = float(tb["speed_limits"][3]) - 1e-3
        err0[0, 1, 1, 3] = 2e-3
        case["bit"], case["C"] = KM.LIMIT, 2
    elif name == "input":
        # torque limits at half of what sample 1 takes (the model's max_torque with the stock tables: the
        # limits enter no rollout)
        ref = TM.track(tb, traj, scale, err0, 0.0, 0.5, STEPS)
        tb = dict(tb)
        tb["torque_limits"] = np.array(tb["torque_limits"], dtype=np.float64, copy=True)
        tb["torque_limits"][:NF] = 0.5 * ref["max_torque"][0, 1]
        case["bit"] = KM.INPUT
        case["others"] = ()
    else:
        raise KeyError(name)
    case.update(tables=tb, traj=traj, scale=scale, err0=err0, obstacles=obs)
    return case


def flag_reference(name):
    if ("flag", name) not in _REF:
        c = flag_case(name)
        _REF[("flag", name)] = (c, KM.track_motion(c["tables"], c["traj"], c["obstacles"], c["scale"], c["err0"], c["window"][0],
                                                   c["window"][1], STEPS, c["C"]))
    return _REF[("flag", name)]


# ---- the spread -----------------------------------------------------------------------------------
def perturbed_tables(tb, rng):
    out = TC.perturbed_tables(tb, rng)
    for k in ("link_center", "link_generators"):
        out[k] = TC._ulp(tb[k], rng)
    return out


def measure_spread(draws=8, robots=ROBOTS, shapes=SHAPES, report=print):
    """{robot: {"rec", "clearance": largest spread}} over the main list"""
    worst = {}
    for robot in robots:
        here = {"rec": 0.0, "clearance": 0.0}
        for shape in shapes:
            tb, traj, scale, err0, obs = case_inputs(robot, shape)
            base = {(w, C): reference(robot, shape, w, C) for w in WINDOWS for C in CHECKS}
            for d in range(draws):
                rng = np.random.default_rng(9000 + d)
                ptb, pobs = perturbed_tables(tb, rng), [TC._ulp(o, rng) for o in obs]
                runs = run_windows(ptb, TC._ulp(traj, rng), TC._ulp(scale, rng), TC._ulp(err0, rng), pobs)
                for w in WINDOWS:
                    here["rec"] = max(here["rec"], float(np.abs(runs[w]["rec"] - base[(w, CHECKS[-1])]["rec"]).max()))
                    for C in CHECKS:
                        got = subsample(ptb, runs[w], pobs, C)["clearance"]
                        ref = base[(w, C)]["clearance"]
                        fin = np.isfinite(ref)
                        assert np.array_equal(fin, np.isfinite(got))
                        if fin.any():
                            here["clearance"] = max(here["clearance"], float(np.abs(got[fin] - ref[fin]).max()))
        report(f"{robot:11s} rec {here['rec']:.2e} clearance {here['clearance']:.2e}")
        worst[robot] = here
    return worst


if __name__ == "__main__":
    w = measure_spread()
    print("SPREAD = {" + ", ".join(f'"{k}": {max(v[k] for v in w.values()):.2e}' for k in ("rec", "clearance")) + "}")
