"""Bitwise A/B of two library builds (development tool): the same worlds planned by the in-tree
library and by a variant next to it (armour-dev_amd/armour_amd/<variant>.so, loaded through
ARMOUR_LIB in a child process each), then k_opt, cost, iterations, evaluations, status and the
constraint values compared bit for bit. Of the first NX worlds of every batch each child also
records eval_constraints (g and J) at two fixed points, one inside the plane cache's box and one
with a coordinate beyond it (the full scan), and the eval_candidates outputs at NC fixed points
(more than one cand_rows chunk, the last one partial; skipped where the build reports no plane
cache, ARMOUR_PLANE_CACHE=0). With `mixed` the batches are planned by plan_mixed with the obstacle
counts cycled over MIXED. Environment variables (ARMOUR_EVAL_FULL, ...) reach both children.

usage: python tools/plan_ab.py <variant .so name> [W] [T] [profile] [batch] [mixed]"""
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "gpurun_out")
NX, NC = 96, 40
MIXED = (0, 1, 6, 20)
FIELDS = ("k", "cost", "it", "ev", "st", "g", "eg", "eJ", "cc", "cv", "cf", "cb")


def child(lib, W, T, profile, batch, mixed, out):
    os.environ["ARMOUR_LIB"] = os.path.join(ROOT, "armour-dev_amd", "armour_amd", lib)
    sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))
    import armour_amd as A

    worlds = [A.make_world(s, 20, profile=profile) for s in range(W)]
    if mixed:
        worlds = [w[:4] + (w[4][:MIXED[i % len(MIXED)]],) for i, w in enumerate(worlds)]
    P = A.Planner(T=T, max_obstacles=20, max_worlds=batch)
    rec = {k: [] for k in FIELDS}
    for b0 in range(0, W, batch):
        ws = worlds[b0:b0 + batch]
        print(f"{lib}: worlds {b0}..{b0 + len(ws) - 1}", flush=True)
        res, _ = (P.plan_mixed if mixed else P.plan)(ws)
        for w, r in enumerate(res):
            rec["k"].append(r["k_opt"]); rec["cost"].append(r["cost"]); rec["it"].append(r["iterations"])
            rec["ev"].append(r["evaluations"]); rec["st"].append(r["status"]); rec["g"].append(P.constraints(w))
        nx = min(NX, len(ws))
        rng = np.random.default_rng(b0)
        X = rng.uniform(-1.0, 1.0, (len(ws), NC, 7))
        if os.environ.get("ARMOUR_PLANE_CACHE") == "0":   # candidate evaluation has no full-scan path
            print(f"{lib}: eval_candidates not recorded (ARMOUR_PLANE_CACHE=0)")
        else:
            c = P.eval_candidates(X)
            rec["cc"].append(c["cost"][:nx].ravel()); rec["cv"].append(c["violation"][:nx].ravel())
            rec["cf"].append(c["feasible"][:nx].ravel()); rec["cb"].append(c["best"][:nx])
        for w in range(nx):   # last: eval_constraints resets the plan state
            inside = 0.9 * X[w, 0]
            beyond = inside.copy()
            beyond[w % 7] = 1.25
            for x in (inside, beyond):
                g, J = P.eval_constraints(w, x)
                rec["eg"].append(g); rec["eJ"].append(J.ravel())
    flat = lambda v: np.concatenate([np.atleast_1d(a) for a in v]) if v else np.zeros(0)
    np.savez(out, **{k: flat(v) for k, v in rec.items()})


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2], int(sys.argv[3]), int(sys.argv[4]), sys.argv[5], int(sys.argv[6]), sys.argv[7] == "mixed",
              sys.argv[8])
        sys.exit(0)
    var = sys.argv[1]
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 96
    T = int(sys.argv[3]) if len(sys.argv) > 3 else 100
    profile = sys.argv[4] if len(sys.argv) > 4 else "survey"
    batch = int(sys.argv[5]) if len(sys.argv) > 5 else W
    mixed = sys.argv[6] if len(sys.argv) > 6 else "uniform"
    os.makedirs(OUT, exist_ok=True)
    outs = []
    for lib in ("libarmour_hip.so", var):
        o = os.path.join(OUT, f"plan_ab_{lib}.npz")
        subprocess.run([sys.executable, __file__, "--child", lib, str(W), str(T), profile, str(batch), mixed, o], check=True)
        outs.append(dict(np.load(o)))
    a, b = outs
    # tobytes: NaN (a failed world's cost) equal to itself, -0.0 different from 0.0
    bad = [k for k in a if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or a[k].tobytes() != b[k].tobytes()]
    nw = int(np.sum(np.any(a["k"].reshape(W, 7) != b["k"].reshape(W, 7), axis=1) | (a["it"] != b["it"])))
    env = " ".join(f"{k}={v}" for k, v in sorted(os.environ.items()) if k.startswith("ARMOUR_") and k != "ARMOUR_LIB")
    print(f"{W} worlds (T={T}, {profile}, {mixed}, batches of {batch}{', ' + env if env else ''}): "
          f"{a['g'].size} plan g values, {a['eg'].size} + {a['eJ'].size} eval_constraints g + J values, "
          f"{a['cc'].size} candidates: fields differing {bad or 'none'}, worlds differing {nw}")
    sys.exit(1 if bad else 0)
