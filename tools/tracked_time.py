#!/usr/bin/env python3
"""Device time of the recording rollouts and the true-arm check (armour_track_motion, armour_episode_track).

    python tools/tracked_time.py record [--parent-lib PATH]   # the cost of the record
    python tools/tracked_time.py episode                      # a tracked episode step at the survey batch
    python tools/tracked_time.py --child KIND ...             # one process: one JSON line

record: N worlds x S uncertainty samples x `steps` RK4 steps over [0, 0.5] (tools/track_time.py's rollouts).
Processes are started one after the other, in turn: "record" (armour_track_motion with `checks` check
points, this tree's library: track_ms of the recording row kernel and check_ms of the true-arm check),
"plain" (armour_track, this tree's library) and, with --parent-lib, "parent" (armour_track on that
library, loaded through ARMOUR_LIB), so all see the same machine state. Each process warms up once and
times `reps` calls. Printed: every process's milliseconds, the medians, record - plain (the cost of
the record) and plain against parent with both ranges.

episode: W survey worlds (armour_amd.make_world, profile "survey") at T time steps with O obstacles, one
planner with armour_episode_track (S samples, `steps` steps, `checks` check points) and one without; a
warm-up step and `reps` timed steps each, in turn. Printed per step: rollout ms, true-arm check ms
(W x S x checks blocks), the desired arm's check ms, and the step's wall time on both planners.
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))


def rollouts(a):
    import armour_amd as A
    from armour_amd import robot_tables as RT

    rng = np.random.default_rng(a.seed)
    traj = np.zeros((a.N, 4, 7))
    traj[:, 0] = rng.uniform(-1.0, 1.0, (a.N, 7))
    traj[:, 1] = rng.uniform(-0.5, 0.5, (a.N, 7))
    traj[:, 2] = rng.uniform(-0.5, 0.5, (a.N, 7))
    traj[:, 3] = rng.uniform(-1.0, 1.0, (a.N, 7))
    return A, traj, A.uncertainty_samples(RT.builtin(0), a.S, seed=a.seed)


def child_record(a):
    A, traj, scale = rollouts(a)
    os.environ.pop("ARMOUR_TRACK_KERNEL", None)
    if a.child == "record":
        obs = [A.make_world(s, 3)[4] for s in range(8)]
        P = A.Planner(T=10, max_obstacles=3, max_worlds=a.N, device=a.device)
        P.reach([(traj[w, 0], traj[w, 1], traj[w, 2], traj[w, 0], obs[w % 8]) for w in range(a.N)])
        call = lambda: P.track_motion(traj, scale, None, 0.0, 0.5, a.steps, a.checks)   # noqa: E731
    else:
        P = A.Planner(T=10, max_obstacles=3, max_worlds=1, device=a.device)
        call = lambda: P.track(traj, scale, None, 0.0, 0.5, a.steps)                    # noqa: E731
    call()
    ms, check = [], []
    for _ in range(a.reps):
        out = call()
        ms.append(out["track_ms"])
        check.append(out.get("check_ms", 0.0))
    P.close()
    print(json.dumps(dict(kind=a.child, ms=ms, check_ms=check, failed=int(out["status"].sum()),
                          worst_pos_err_over_qe=float(out["max_pos_err"].max() / out["qe"]))), flush=True)


def child_episode(a):
    import armour_amd as A
    from armour_amd import robot_tables as RT

    worlds = [A.make_world(50_000 + s, a.O, profile="survey") for s in range(a.N)]
    goals = np.array([w[0] + 12 * (w[3] - w[0]) for w in worlds])
    scale = A.uncertainty_samples(RT.builtin(0), a.S, seed=a.seed)
    planners = {}
    for name in ("tracked", "plain"):
        P = A.Planner(T=a.T, max_obstacles=a.O, max_worlds=a.N, device=a.device)
        P.episode_begin(worlds, goals, check_samples=a.checks)
        if name == "tracked":
            P.episode_track(scale=scale, steps=a.steps)
        planners[name] = P
    rows = []
    for step in range(a.reps + 1):
        row = dict(step=step)
        for name, P in planners.items():
            t0 = time.perf_counter()
            running, _, tm = P.episode_step()
            row[name + "_wall_ms"] = (time.perf_counter() - t0) * 1e3
            row[name + "_running"] = running
            row[name + "_check_ms"] = tm["check_ms"]
            if name == "tracked":
                tr = P.episode_tracked()
                row.update(rollout_ms=tr["rollout_ms"], true_check_ms=tr["check_ms"], flags=int(np.bitwise_or.reduce(tr["flags"])),
                           flagged_worlds=int(np.sum(tr["flags"] != 0)))
        rows.append(row)
    for P in planners.values():
        P.close()
    print(json.dumps(dict(kind="episode", rows=rows)), flush=True)


def run_child(a, kind, env=None):
    cmd = [sys.executable, os.path.abspath(__file__), a.mode, "--child", kind] + [
        f"--{k}={getattr(a, k)}" for k in ("N", "S", "steps", "checks", "reps", "device", "seed", "T", "O")]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env)
    if r.returncode != 0:
        sys.exit(f"{kind} process failed ({r.returncode}):\n{r.stderr[-2000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=["record", "episode"])
    ap.add_argument("--child", choices=["record", "plain", "parent", "episode"], help="run one process of this kind")
    ap.add_argument("--parent-lib", default="", help="record: another build of the library for the A/B of armour_track")
    ap.add_argument("--N", type=int, default=1308)
    ap.add_argument("--S", type=int, default=8)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--checks", type=int, default=11)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=5, help="record: per kind")
    ap.add_argument("--T", type=int, default=100)
    ap.add_argument("--O", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child_episode(a) if a.child == "episode" else child_record(a)
    if a.mode == "episode":
        out = run_child(a, "episode")
        print(f"W {a.N} T {a.T} O {a.O} S {a.S} steps {a.steps} check points {a.checks}: {a.N * a.S} rollouts, "
              f"{a.N * a.S * a.checks} true-arm check blocks (step 0 is the warm-up)")
        for r in out["rows"]:
            print(f"step {r['step']}: rollouts {r['rollout_ms']:8.3f} ms  true-arm check {r['true_check_ms']:7.3f} ms  desired-arm check "
                  f"{r['tracked_check_ms']:6.3f} ms  wall tracked {r['tracked_wall_ms']:8.1f} ms  untracked {r['plain_wall_ms']:8.1f} ms  "
                  f"running {r['tracked_running']} / {r['plain_running']}  flags {r['flags']} on {r['flagged_worlds']} worlds")
        return
    kinds = ["record", "plain"] + (["parent"] if a.parent_lib else [])
    res = {k: [] for k in kinds}
    for i in range(a.processes):
        for kind in kinds:
            env = dict(os.environ, ARMOUR_LIB=os.path.abspath(a.parent_lib)) if kind == "parent" else None
            line = run_child(a, kind, env)
            res[kind].append(line)
            print(f"process {i} {kind:6s} ms " + " ".join(f"{v:8.3f}" for v in line["ms"]) +
                  ("   check ms " + " ".join(f"{v:6.3f}" for v in line["check_ms"]) if kind == "record" else "") +
                  f"   failed {line['failed']} max |e| / qe {line['worst_pos_err_over_qe']:.3f}", flush=True)
    print(f"N {a.N} S {a.S} steps {a.steps} check points {a.checks}: {a.N * a.S} rollouts")
    med = {}
    for kind in kinds:
        ms = np.array([np.median(ln["ms"]) for ln in res[kind]])
        med[kind] = float(np.median(ms))
        print(f"{kind:6s} median of {len(ms)} processes {med[kind]:8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f})")
    chk = np.array([np.median(ln["check_ms"]) for ln in res["record"]])
    print(f"true-arm check: median {np.median(chk):.3f} ms (min {chk.min():.3f}, max {chk.max():.3f})")
    print(f"record - plain = {med['record'] - med['plain']:+.3f} ms ({100 * (med['record'] / med['plain'] - 1):+.2f} %)")
    if a.parent_lib:
        print(f"plain - parent = {med['plain'] - med['parent']:+.3f} ms ({100 * (med['plain'] / med['parent'] - 1):+.2f} %)")


if __name__ == "__main__":
    main()
