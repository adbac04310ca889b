"""One mixed call against ten grouped calls on the reference's 100 saved worlds (run on the GPU).

The saved worlds (tests/golden/saved_worlds_T100.npz, T = 100) carry 5 to 14 obstacles. Side A plans
all 100 in one Planner.plan_mixed call on one planner; side B is what the uniform entry needs: one
planner per obstacle count and one Planner.plan call each, ten calls. Every planner is built before
any timing, both sides are warmed up once, then the sides alternate for `repeats` rounds in this one
process. A call ends in a host wait for its results, so the host clock around it is the call's time.
Printed: the median (and min, max) over the rounds of each side's wall time and of its summed
reach_kernel_ms, reach_ms and nlp_ms (armour_timing: device events), and how the two sides' plans
compare. The sides need not agree bitwise here: the 100-world call's reach runs on the bundle engine
and every group (at most 22 worlds, 2200 jobs) on the per-job engine, whose reach sets differ at
rounding level; the bar is the saved worlds' own (decisions, status and
iteration counts identical, k_opt within 1e-8, cost within 1e-8 relative). With ARMOUR_ENGINE=job
and ARMOUR_REACH_WIDE=0 in the environment both sides run the per-job engine's 128-thread kernel,
whose reach sets do not depend on the batch, and the plans are bitwise equal.

usage: python tools/mixed_ab.py [repeats=15]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))

import armour_amd as A  # noqa: E402
from armour_amd.worlds import csv_world  # noqa: E402

KEYS = ("wall_ms", "reach_kernel_ms", "reach_ms", "nlp_ms")


def saved_worlds():
    fx = np.load(os.path.join(ROOT, "tests", "golden", "saved_worlds_T100.npz"))
    worlds = []
    for r in fx["rows"]:
        n = int(np.max(np.nonzero(~np.all(np.isnan(r), axis=1))[0])) + 1  # drop the padding rows
        worlds.append(csv_world(r[:n]))
    return worlds, [int(c) for c in fx["num_obstacles"]]


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 15
    worlds, counts = saved_worlds()
    groups = {n: [i for i, c in enumerate(counts) if c == n] for n in sorted(set(counts))}
    PM = A.Planner(T=100, max_obstacles=max(counts), max_worlds=len(worlds))
    PG = {n: A.Planner(T=100, max_obstacles=n, max_worlds=len(idx)) for n, idx in groups.items()}

    def mixed():
        t0 = time.perf_counter()
        res, tm = PM.plan_mixed(worlds)
        wall = (time.perf_counter() - t0) * 1e3
        return res, dict(wall_ms=wall, reach_kernel_ms=tm["reach_kernel_ms"], reach_ms=tm["reach_ms"], nlp_ms=tm["nlp_ms"])

    def grouped():
        out = [None] * len(worlds)
        acc = dict.fromkeys(KEYS, 0.0)
        t0 = time.perf_counter()
        for n, idx in groups.items():
            res, tm = PG[n].plan([worlds[i] for i in idx])
            for i, r in zip(idx, res):
                out[i] = r
            for k in KEYS[1:]:
                acc[k] += tm[k]
        acc["wall_ms"] = (time.perf_counter() - t0) * 1e3
        return out, acc

    ra, _ = mixed()      # warm-up of both sides: code objects, first-use allocations
    rb, _ = grouped()
    bitwise = sum(np.array_equal(a["k_opt"], b["k_opt"]) and a["cost"] == b["cost"] and a["iterations"] == b["iterations"]
                  and a["evaluations"] == b["evaluations"] and a["status"] == b["status"] and a["feasible"] == b["feasible"]
                  for a, b in zip(ra, rb))
    decisions = sum((a["feasible"], a["status"], a["iterations"]) == (b["feasible"], b["status"], b["iterations"])
                    for a, b in zip(ra, rb))
    dk = max(float(np.abs(a["k_opt"] - b["k_opt"]).max()) for a, b in zip(ra, rb))
    dc = max(abs(a["cost"] - b["cost"]) / max(abs(b["cost"]), 1e-300) for a, b in zip(ra, rb))
    same = decisions == len(worlds) and dk <= 1e-8 and dc <= 1e-8
    rec = {"mixed": [], "grouped": []}
    for _ in range(repeats):
        rec["mixed"].append(mixed()[1])
        rec["grouped"].append(grouped()[1])
    print(f"100 saved worlds, T=100, obstacle counts {dict((n, len(i)) for n, i in groups.items())}")
    print(f"engine: {os.environ.get('ARMOUR_ENGINE', 'default (by batch size)')}"
          f"{' ARMOUR_REACH_WIDE=' + os.environ['ARMOUR_REACH_WIDE'] if 'ARMOUR_REACH_WIDE' in os.environ else ''}")
    print(f"mixed call against grouped calls: {bitwise}/100 worlds bitwise equal; feasible, status and iterations "
          f"identical for {decisions}/100; max |k_opt difference| {dk:.3e}; max relative cost difference {dc:.3e}")
    print(f"{repeats} alternating rounds after one warm-up of each side; median [min, max], ms")
    for side, label in (("mixed", "one plan_mixed call (1 planner)"), ("grouped", "ten plan calls (10 planners), summed")):
        print(f"  {label}")
        for k in KEYS:
            v = np.array([r[k] for r in rec[side]])
            print(f"    {k:16s} {np.median(v):9.3f} [{v.min():9.3f}, {v.max():9.3f}]")
    m = np.median([r["wall_ms"] for r in rec["mixed"]])
    g = np.median([r["wall_ms"] for r in rec["grouped"]])
    print(f"  wall: grouped / mixed = {g / m:.2f}x")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
