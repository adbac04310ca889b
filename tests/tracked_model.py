"""Model of armour_track_motion — TEST INFRASTRUCTURE: numpy, no oracle, no product code beyond the tables.

The definition in include/armour_hip.h (armour_track_motion), restated with the models the project has:

  * the rollouts are track_model's: the RK4 loop of Rollouts.run over Rollouts.stage, in the same order and
    therefore with the same bits, plus the record: check point c is the state (q, qd) at the first stage
    of step c * stride, the last one the state at t1; a rollout that stopped being finite records the
    state it keeps;
  * the true arm's clearance is episode_model's separation (collision_model.row on the link boxes of
    point forward kinematics) at the recorded q instead of a sampled curve: the minimum over (check point,
    link, obstacle) with its first minimiser in that order per rollout, then the minimum over a world's
    samples, ties to the lowest sample;
  * the flags, with strict comparisons;
  * a tracked episode's step (armour_episode_track): episode_model.step for the desired arm, the rollouts
    of the true arms from their carried absolute states along what the world executes, the fold into the
    world's record and the stops.
"""
from __future__ import annotations

import numpy as np

import collision_model as C
import episode_model as E
import track_model as TM

NF = 7
COLLISION, INPUT, BOUND, LIMIT, NOT_FINITE = 1, 2, 4, 8, 16


def run_recorded(R, t0, t1, steps, check_samples, start=None):
    """(out, rec): Rollouts.run's outputs of the rollouts R (a track_model.Rollouts) and the record
    rec [check_samples, R, 2, 7]; start [R, 2, 7] (optional): the absolute start state (q, qd) instead of the
    desired state plus err0"""
    assert check_samples >= 2 and steps % (check_samples - 1) == 0
    stride = steps // (check_samples - 1)
    q_des, qd_des, _ = R.desired(t0)
    q, qd = q_des + R.err0[:, 0], qd_des + R.err0[:, 1]
    if start is not None:
        q, qd = np.array(start[:, 0], dtype=np.float64), np.array(start[:, 1], dtype=np.float64)
    n = R.R
    out = dict(max_pos_err=np.zeros((n, NF)), max_vel_err=np.zeros((n, NF)), max_torque=np.zeros((n, NF)),
               max_V=np.zeros(n), max_robust=np.zeros(n))
    rec = np.zeros((check_samples, n, 2, NF))
    alive = np.ones(n, dtype=bool)

    def record(S, q, qd):
        nonlocal alive
        alive = alive & S["ok"]
        a = alive
        for name, val in (("max_pos_err", np.abs(q - S["q_des"])), ("max_vel_err", np.abs(qd - S["qd_des"])),
                          ("max_torque", np.abs(S["u"])), ("max_V", S["V"]), ("max_robust", S["lam"])):
            out[name][a] = np.fmax(out[name][a], val[a])

    h = (t1 - t0) / steps
    hh = 0.5 * h
    with np.errstate(all="ignore"):
        for s in range(steps):
            if s % stride == 0:
                rec[s // stride, :, 0], rec[s // stride, :, 1] = q, qd
            t = t0 + s * h
            S1 = R.stage(t, q, qd)
            record(S1, q, qd)
            q2, v2 = q + hh * qd, qd + hh * S1["qdd"]
            S2 = R.stage(t + hh, q2, v2)
            q3, v3 = q + hh * v2, qd + hh * S2["qdd"]
            S3 = R.stage(t + hh, q3, v3)
            q4, v4 = q + h * v3, qd + h * S3["qdd"]
            S4 = R.stage(t + h, q4, v4)
            qn = q + (h / 6) * (qd + 2 * v2 + 2 * v3 + v4)
            vn = qd + (h / 6) * (S1["qdd"] + 2 * S2["qdd"] + 2 * S3["qdd"] + S4["qdd"])
            good = S1["ok"] & S2["ok"] & S3["ok"] & S4["ok"] & np.all(np.isfinite(qn), axis=1) & np.all(np.isfinite(vn), axis=1)
            alive = alive & good
            q = np.where(alive[:, None], qn, q)
            qd = np.where(alive[:, None], vn, qd)
        record(R.stage(t1, q, qd), q, qd)
    rec[check_samples - 1, :, 0], rec[check_samples - 1, :, 1] = q, qd
    out["end_state"] = np.stack([q, qd], axis=1)
    out["status"] = (~alive).astype(np.int32)
    return out, rec


def _shaped(robot):
    from armour_amd import robot_tables as RT

    return RT._shaped(robot)


def state_clearance(robot, q, obstacles):
    """the true arm at the recorded q [C, 7] against obstacles [O, 12]: dict(clearance, where (check point,
    link, obstacle): the first minimum in that order, runner_up: the smallest separation elsewhere minus the
    minimum, bound: the rounding bound of the pair (collision_model.rounding_bound + episode_model.fk_bound
    at the recorded angles), fragile: some pair of the minimiser is parallel to rounding
    (episode_model.separations))"""
    obstacles = np.asarray(obstacles, dtype=np.float64).reshape(-1, 12)
    if obstacles.shape[0] == 0:
        return dict(clearance=np.inf, where=(-1, -1, -1), runner_up=np.inf, bound=0.0, fragile=False)
    robot = _shaped(robot)
    q = np.asarray(q, dtype=np.float64)
    c, G = E.link_boxes(robot, q)                                  # [C, NJ, 3], [C, NJ, 3, 3]
    shape = (q.shape[0], G.shape[1], obstacles.shape[0])
    Gob = obstacles[:, 3:].reshape(-1, 3, 3)
    G9 = np.concatenate([np.broadcast_to(Gob[None, None], shape + (3, 3)), np.broadcast_to(G[:, :, None], shape + (3, 3)),
                         np.zeros(shape + (3, 3))], axis=-2)
    cl, co = c[:, :, None, :], obstacles[None, None, :, :3]
    sep = -C.row(cl, co, G9)["g"]
    deg = C.degenerate(G9)
    length = np.sqrt((G9 * G9).sum(-1))
    mixed = np.array([a < 3 <= b < 6 for a, b in C.PAIRS])
    live = (length[..., C._IA] > 0) & (length[..., C._IB] > 0) & ((C._cross(G9)[0] != 0).sum(-1) > 1)
    fragile = (deg & live & mixed).any(-1)
    z = np.zeros(NF)
    bound = C.rounding_bound(cl, co, G9).max() + max(E.fk_bound(robot, (qc, z, z, z)) for qc in q)
    flat = sep.reshape(-1)
    i = int(np.argmin(flat))
    rest = np.delete(flat, i)
    return dict(clearance=float(flat[i]), where=tuple(int(v) for v in np.unravel_index(i, sep.shape)),
                runner_up=float(rest.min() - flat[i]) if rest.size else np.inf, bound=float(bound),
                fragile=bool(fragile.reshape(-1)[i]))


def thresholds(robot):
    """(qe, qde) as the library derives them from the tables"""
    eps = float(np.sqrt(2 * robot["V_m"] / robot["M_min"]))
    return eps / float(robot["K"]), 2 * eps


def flag_margins(robot, out, rec):
    """per rollout, the signed distance of each flag's quantity from its threshold (> 0: raised), [R] each:
    INPUT max_j (max_torque - torque_limits), BOUND max_j of (max_pos_err - qe, max_vel_err - qde), LIMIT the
    largest of state_lb - q, q - state_ub and |qd| - speed_limits over the check points and joints"""
    qe, qde = thresholds(robot)
    lb, ub = np.asarray(robot["state_lb"], dtype=np.float64)[:NF], np.asarray(robot["state_ub"], dtype=np.float64)[:NF]
    sp, tq = np.asarray(robot["speed_limits"], dtype=np.float64)[:NF], np.asarray(robot["torque_limits"], dtype=np.float64)[:NF]
    q, qd = rec[:, :, 0], rec[:, :, 1]                              # [C, R, 7]
    lim = np.maximum(np.maximum(lb - q, q - ub), np.abs(qd) - sp).max(axis=(0, 2))
    return {INPUT: (out["max_torque"] - tq).max(axis=1),
            BOUND: np.maximum(out["max_pos_err"] - qe, out["max_vel_err"] - qde).max(axis=1), LIMIT: lim}


def flags(robot, out, rec, clearance):
    """[R] the bit mask of each rollout (clearance [R])"""
    f = np.where(np.asarray(clearance) <= 0, COLLISION, 0)
    for bit, m in flag_margins(robot, out, rec).items():
        f = f | np.where(m > 0, bit, 0)
    return (f | np.where(out["status"] != 0, NOT_FINITE, 0)).astype(np.int32)


def track_motion(robot, traj, obstacles, scale=None, err0=None, t0=0.0, t1=0.5, steps=50, check_samples=11):
    """armour_track_motion's outputs for traj [W, 4, 7], obstacles (a list of W arrays [O_w, 12]), scale
    [W, S, 2, NJ] / None, err0 [W, S, 2, 7] / None, shaped [W, S, ...] and [W, ...]; plus rec [C, W, S, 2, 7],
    and per rollout the model's runner_up, bound and fragile, and the flag margins (flag_margins)"""
    traj = np.asarray(traj, dtype=np.float64)
    W = traj.shape[0]
    S = 1 if scale is None and err0 is None else (np.shape(scale)[1] if scale is not None else np.shape(err0)[1])
    sc = None if scale is None else np.asarray(scale, dtype=np.float64).reshape(W * S, 2, -1)
    e0 = None if err0 is None else np.asarray(err0, dtype=np.float64).reshape(W * S, 2, NF)
    flat, rec = run_recorded(TM.Rollouts(robot, np.repeat(traj, S, axis=0), sc, e0), t0, t1, steps, check_samples)
    out = {k: v.reshape((W, S) + v.shape[1:]) for k, v in flat.items()}
    cl = [state_clearance(robot, rec[:, r, 0], obstacles[r // S]) for r in range(W * S)]
    out["clearance"] = np.array([c["clearance"] for c in cl]).reshape(W, S)
    out["where"] = np.array([c["where"] for c in cl], dtype=np.int32).reshape(W, S, 3)
    for k in ("runner_up", "bound", "fragile"):
        out[k] = np.array([c[k] for c in cl]).reshape(W, S)
    out["flags"] = flags(robot, flat, rec, out["clearance"].reshape(-1)).reshape(W, S)
    out["margins"] = {bit: m.reshape(W, S) for bit, m in flag_margins(robot, flat, rec).items()}
    first = np.argmin(out["clearance"], axis=1)                     # (the first minimum: ties to the lowest sample)
    out["world_clearance"] = out["clearance"][np.arange(W), first]
    ww = np.concatenate([first[:, None], out["where"][np.arange(W), first]], axis=1).astype(np.int32)
    ww[~np.isfinite(out["world_clearance"])] = -1
    out["world_where"] = ww
    out["rec"] = rec.reshape((check_samples, W, S, 2, NF))
    return out


# ---- tracked episodes -----------------------------------------------------------------------------
def episode_begin(state, S, err0=None):
    """the tracking state of one world after armour_episode_track: state (episode_model.begin), S true arms,
    err0 [S, 2, 7] or None"""
    true = np.repeat(np.stack([state["q"], state["qd"]])[None], S, axis=0)
    if err0 is not None:
        true = true + np.asarray(err0, dtype=np.float64)
    return dict(true=true, clearance=np.inf, clearance_at=(-1, -1, -1, -1), max_pos_err=np.zeros(NF), max_vel_err=np.zeros(NF),
                max_torque=np.zeros(NF), max_V=0.0, max_robust=0.0, flags=0, flag_step=[-1] * 5,
                last_flags=np.zeros(S, dtype=np.int32))


def episode_segment(state, k_opt, accept):
    """(trajectory, window) the true arms of a running world follow this step, or None when it executes
    nothing (frozen, or no fail-safe)"""
    if state["status"] != 0:
        return None
    z = np.zeros(NF)
    if accept:
        return (state["q"], state["qd"], state["qdd"], np.asarray(k_opt, dtype=np.float64)), (0.0, E.T_PLAN)
    if state["mode"] == 1 and state["pending"] is not None:
        return state["pending"], (E.T_PLAN, 1.0)
    if state["mode"] == 1:
        return None
    return (state["q"], z, z, z), (0.0, E.T_PLAN)


def episode_rollouts(robot, segments, trues, scales, steps, check_samples):
    """the rollouts of several worlds' true arms: segments [(trajectory, window) or None], trues [[S, 2, 7]],
    scales [[S, 2, NJ] or None]; returns [(out, rec) or None] per world. Worlds that share a window run as one
    batch (the rollouts do not see each other)."""
    res = [None] * len(segments)
    for win in sorted({seg[1] for seg in segments if seg is not None}):
        ws = [w for w, seg in enumerate(segments) if seg is not None and seg[1] == win]
        S = trues[ws[0]].shape[0]
        nj = int(robot["num_joints"])
        traj = np.concatenate([np.repeat(np.stack(segments[w][0])[None], S, axis=0) for w in ws])
        scale = np.concatenate([np.ones((S, 2, nj)) if scales[w] is None else np.asarray(scales[w], dtype=np.float64) for w in ws])
        out, rec = run_recorded(TM.Rollouts(robot, traj, scale, None), win[0], win[1], steps, check_samples,
                                start=np.concatenate([trues[w] for w in ws]))
        for i, w in enumerate(ws):
            sl = slice(i * S, (i + 1) * S)
            res[w] = ({k: v[sl] for k, v in out.items()}, rec[:, sl])
    return res


def episode_fold(robot, state, after, tracked, rolled, obstacles, stops=(1, 1, 0)):
    """(state, tracked, step outputs) of one world that executed a segment: `after` is episode_model.step's
    state (the existing rules), rolled = (out, rec) of its true arms"""
    s, t = dict(after), dict(tracked)
    out, rec = rolled
    S = t["true"].shape[0]
    step_no = state["steps"]
    cl = [state_clearance(robot, rec[:, r, 0], obstacles) for r in range(S)]
    clear = np.array([c["clearance"] for c in cl])
    fl = flags(robot, out, rec, clear)
    first = int(np.argmin(clear))
    if clear[first] < t["clearance"]:
        t["clearance"] = float(clear[first])
        t["clearance_at"] = (step_no, first, cl[first]["where"][1], cl[first]["where"][2])
    for k in ("max_pos_err", "max_vel_err", "max_torque"):
        t[k] = np.fmax(t[k], out[k].max(axis=0))
    t["max_V"], t["max_robust"] = max(t["max_V"], float(out["max_V"].max())), max(t["max_robust"], float(out["max_robust"].max()))
    every = int(np.bitwise_or.reduce(fl))
    t["flag_step"] = [step_no if (every >> b) & 1 and old < 0 else old for b, old in enumerate(t["flag_step"])]
    t["flags"] = t["flags"] | every
    t["last_flags"], t["true"] = fl, out["end_state"]
    if s["status"] not in (4, 2):
        for bit, status, on in ((COLLISION, 2, 1), (NOT_FINITE, 8, 1), (INPUT, 5, stops[0]), (BOUND, 6, stops[1]),
                                (LIMIT, 7, stops[2])):
            if every & bit and on:
                s["status"] = status
                break
    step_out = dict(out, rec=rec, clearance=clear, bound=np.array([c["bound"] for c in cl]),
                    runner_up=np.array([c["runner_up"] for c in cl]), fragile=np.array([c["fragile"] for c in cl]),
                    margins=flag_margins(robot, out, rec), flags=fl)
    return s, t, step_out


def episode_step(robot, state, tracked, k_opt, accept, obstacles, goal, scale=None, steps=50, stops=(1, 1, 0), check_samples=11,
                 **config):
    """(state, tracked, step outputs or None) after one armour_episode_step of one tracked world: state and
    the plan as episode_model.step takes them, tracked from episode_begin or the previous step, scale
    [S, 2, NJ] or None, stops = (stop_on_input, stop_on_bound, stop_on_limit)"""
    after = E.step(robot, state, k_opt, accept, obstacles, goal, check_samples=check_samples, **config)
    seg = episode_segment(state, k_opt, accept)
    if seg is None:
        return after, dict(tracked), None
    rolled = episode_rollouts(robot, [seg], [tracked["true"]], [scale], steps, check_samples)[0]
    return episode_fold(robot, state, after, tracked, rolled, obstacles, stops)
