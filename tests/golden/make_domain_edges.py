"""Generate tests/golden/domain_edges.npz (build container, repo root):

    python tests/golden/make_domain_edges.py

The limit, speed and far_goal cases of tests/domain_edges.py (T = 10, O = 3, the built-in Kinova) with
the oracle's (CPU restatement's) plan on each: feasible, status, iterations, evaluations, k_opt, cost.
tests/test_domain_edges.py pins the oracle to them; tests/test_gpu_domain_edges.py holds the HIP path
to them. Parity with the reference itself stays unpinned.
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import domain_edges as DE  # noqa: E402
from oracle import OraclePlanner  # noqa: E402

PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "domain_edges.npz")


def generate(verbose=False):
    rec = {k: [] for k in ("names", "q0", "qd0", "qdd0", "q_des", "obstacles", "feasible", "status", "iterations",
                           "evaluations", "k_opt", "cost")}
    for name, world in DE.plan_cases():
        R = OraclePlanner(*world, T=DE.T, threads=4)
        R.reach()
        r = R.plan()
        for k, v in zip(("q0", "qd0", "qdd0", "q_des", "obstacles"), world):
            rec[k].append(np.asarray(v, dtype=np.float64))
        rec["names"].append(name)
        for k in ("feasible", "status", "iterations", "evaluations", "k_opt", "cost"):
            rec[k].append(r[k])
        if verbose:
            print(f"{name:24s} feasible={r['feasible']!s:5} status={r['status']} it={r['iterations']:3d} "
                  f"max|k|={np.abs(r['k_opt']).max():.6f}", flush=True)
    out = {k: np.array(v) for k, v in rec.items()}
    out["T"] = np.int64(DE.T)
    return out


if __name__ == "__main__":
    np.savez_compressed(PATH, **generate(verbose=True))
    print("wrote", PATH, os.path.getsize(PATH), "bytes")
