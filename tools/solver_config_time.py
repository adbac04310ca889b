"""Time per solve of the solver configurations (armour_solver_options) on a GPU: the default (1, 16, 0),
the reference's configuration (2, 16, 6) and the quality-function pair with the default's floor, grid and
Hessian (3, 16, 0), on 327 and 1308 survey worlds at T = 100, O = 20 and on eight of them (the tail's
latency-bound case). Per arm: nlp_ms (the library's own timing of the solve, best and median of the
repeats), mean iterations and mean evaluations per world, and the path census' qf_sigma launches.
One planner per batch size, the options switched between plans (armour_set_solver_options), so every arm
plans on the same reach sets' inputs and buffers.

usage: python tools/solver_config_time.py [repeats] [sizes, comma separated]  ->  profiles/solver_config_time.txt"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))
import armour_amd as A  # noqa: E402

ARMS = (("default", (1, 16, 0)), ("reference (2, 16, 6)", (2, 16, 6)), ("pair, default floor (3, 16, 0)", (3, 16, 0)))
T, O = 100, 20


def main():
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    sizes = [int(v) for v in sys.argv[2].split(",")] if len(sys.argv) > 2 else [8, 327, 1308]
    lines = [f"solver configurations, survey worlds (seeds 0..W-1), T = {T}, O = {O}, {reps} plans per arm after one warm-up; "
             "nlp_ms best / median, per world: iterations, evaluations; qf_sigma launches per plan"]
    for W in sizes:
        worlds = [A.make_world(s, O, profile="survey") for s in range(W)]
        P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
        base = None
        for name, (mu, G, h) in ARMS:
            P.set_solver_options(mu_strategy=mu, qf_grid=G, lbfgs_history=h)
            P.plan(worlds)  # warm-up (the plane cache's pool, first-launch costs)
            ms = []
            for _ in range(reps):
                before = P.path_counts()
                res, tm = P.plan(worlds)
                ms.append(tm["nlp_ms"])
            sig = P.path_counts()["qf_sigma"] - before["qf_sigma"]
            it = np.mean([r["iterations"] for r in res])
            ev = np.mean([r["evaluations"] for r in res])
            feas = sum(r["feasible"] for r in res)
            best = min(ms)
            base = best if base is None else base
            lines.append(f"W = {W:5d}  {name:32s} nlp_ms {best:9.3f} / {np.median(ms):9.3f}  ({best / base:5.2f} x default)  "
                         f"iterations {it:6.2f}  evaluations {ev:6.2f}  feasible {feas:4d}  qf_sigma {sig}")
            print(lines[-1], flush=True)
        P.close()
    out = os.path.join(ROOT, "profiles", "solver_config_time.txt")
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
