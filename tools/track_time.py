#!/usr/bin/env python3
"""Device time of armour_track for the row kernel and the serial kernel (ARMOUR_TRACK_KERNEL).

    python tools/track_time.py                      # 5 processes per kernel, interleaved, on one GPU
    python tools/track_time.py --child row          # one process: one JSON line

Each process creates a planner (built-in Kinova), runs N trajectories x S uncertainty samples
(armour_amd.uncertainty_samples) x `steps` RK4 steps over [0, 0.5] once to warm up and `reps` times
timed, and reports track_ms (HIP events around the kernel). The parent starts the processes one after
the other, row and serial in turn, so both kernels see the same machine state, and prints the
milliseconds of every process, their median, and rollout-steps per second.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))


def child(a):
    import armour_amd as A
    from armour_amd import robot_tables as RT

    if a.child == "serial":
        os.environ["ARMOUR_TRACK_KERNEL"] = "serial"
    else:
        os.environ.pop("ARMOUR_TRACK_KERNEL", None)
    rng = np.random.default_rng(a.seed)
    traj = np.zeros((a.N, 4, 7))
    traj[:, 0] = rng.uniform(-1.0, 1.0, (a.N, 7))
    traj[:, 1] = rng.uniform(-0.5, 0.5, (a.N, 7))
    traj[:, 2] = rng.uniform(-0.5, 0.5, (a.N, 7))
    traj[:, 3] = rng.uniform(-1.0, 1.0, (a.N, 7))
    scale = A.uncertainty_samples(RT.builtin(0), a.S, seed=a.seed)
    P = A.Planner(T=10, max_obstacles=3, max_worlds=1, device=a.device)
    P.track(traj, scale, None, 0.0, 0.5, a.steps)
    ms = []
    for _ in range(a.reps):
        out = P.track(traj, scale, None, 0.0, 0.5, a.steps)
        ms.append(out["track_ms"])
    P.close()
    print(json.dumps(dict(kernel=a.child, ms=ms, failed=int(out["status"].sum()), max_robust=float(out["max_robust"].max()),
                          worst_pos_err_over_qe=float(out["max_pos_err"].max() / out["qe"]))), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", choices=["row", "serial"], help="run one process of this kernel")
    ap.add_argument("--N", type=int, default=1308)
    ap.add_argument("--S", type=int, default=8)
    ap.add_argument("--steps", type=int, default=250)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--processes", type=int, default=5, help="per kernel")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.child:
        return child(a)
    res = {"row": [], "serial": []}
    for i in range(a.processes):
        for kern in ("row", "serial"):
            cmd = [sys.executable, os.path.abspath(__file__), "--child", kern] + [
                f"--{k}={getattr(a, k)}" for k in ("N", "S", "steps", "reps", "device", "seed")]
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                sys.exit(f"{kern} process {i} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            line = json.loads(r.stdout.strip().splitlines()[-1])
            res[kern].append(line)
            print(f"process {i} {kern:6s} ms " + " ".join(f"{v:8.3f}" for v in line["ms"]) +
                  f"   failed {line['failed']} max lambda {line['max_robust']:.3f} max |e| / qe {line['worst_pos_err_over_qe']:.3f}",
                  flush=True)
    work = a.N * a.S * a.steps
    print(f"N {a.N} S {a.S} steps {a.steps}: {a.N * a.S} rollouts, {work} rollout-steps")
    med = {}
    for kern, lines in res.items():
        ms = np.array([np.median(ln["ms"]) for ln in lines])
        med[kern] = float(np.median(ms))
        print(f"{kern:6s} median of {len(ms)} processes {med[kern]:8.3f} ms (min {ms.min():.3f}, max {ms.max():.3f}): "
              f"{work / med[kern] * 1e3:.3e} rollout-steps/s")
    print(f"serial / row = {med['serial'] / med['row']:.2f}")


if __name__ == "__main__":
    main()
