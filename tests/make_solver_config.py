"""Generate tests/golden/solver_config.npz: the oracle's plans under the optional solver configurations
(armour_solver_options; oracle/src/ipm.cpp mu_strategy 2 / 3, qf_grid, lbfgs_hist) on the sets the GPU
tests compare against (tests/test_gpu_solver_config.py). Test tooling, run on the CPU from the
repository root after the oracle is built:

    python tests/make_solver_config.py

Per set and configuration (mu_strategy, qf_grid, lbfgs_history) it stores the oracle's clean plan of
every world (k_opt, cost, status, feasible, iterations, evaluations, restart_iter), the largest
distances of the oracle's own plans at noise 1e-15, 1e-14 and 3e-14 from it (dk_noise, dit_noise; dst_noise
is 1 where a noisy plan changed status or feasibility), and a SHA-1 of each world's inputs. The noise
is oracle_plan_ex's relative perturbation of g and J: what rounding-level differences in the row sums
do to a plan under the configuration, which is what the GPU tests' per-world tolerances are made of.

It also prints, per configuration, the median distance in k_opt from the default solver's plan and
(with --golden) from the oracle's golden-section sigma search, the figures DESIGN.md section 5 quotes.
"""
from __future__ import annotations

import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("armour-dev_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))

GOLD = os.path.join(ROOT, "tests", "golden")
OUT = os.path.join(GOLD, "solver_config.npz")
NOISE = (1e-15, 1e-14, 3e-14)
REFERENCE = (2, 16, 6)   # the reference's Ipopt configuration on the 16-point sigma grid
SURVEY_T, SURVEY_O, SURVEY_N = 20, 8, 64   # seeds 0 .. 63; the GPU cases plan the first 48
# set -> configurations (tests/test_gpu_solver_config.py cases 1 and 2)
CONFIGS = {
    "survey_T20_O8": [REFERENCE],
    "boundary_small_T20_O6": [REFERENCE, (3, 16, 0), (1, 16, 6), (2, 8, 6)],
    "armtd_T100_O10": [REFERENCE],
}


def key(cfg):
    return "%d_%d_%d" % tuple(cfg)


def flags_of(cfg):
    """OraclePlanner.plan's (mu_strategy, flags) of a configuration: qf_grid in bits 8-15 (strategies 2
    and 3 only), lbfgs_hist in bits 16-23"""
    mu, G, h = cfg
    return mu, ((G << 8) if mu >= 2 else 0) | (h << 16)


def set_worlds(name):
    """(T, O, worlds, armtd) of a set; a world is the tuple its planner takes"""
    import armour_amd as A

    if name == "survey_T20_O8":
        return SURVEY_T, SURVEY_O, [A.make_world(s, SURVEY_O, profile="survey") for s in range(SURVEY_N)], False
    fx = dict(np.load(os.path.join(GOLD, name + ".npz")))
    W = len(fx["kinds"])
    O = fx["obstacles"].shape[1]
    if name.startswith("armtd"):
        return int(fx["T"]), O, [(fx["q0"][w], fx["qd0"][w], fx["q_des"][w], fx["tables"][w], fx["k_range"][w],
                                  fx["obstacles"][w]) for w in range(W)], True
    return int(fx["T"]), O, [(fx["q0"][w], fx["qd0"][w], fx["qdd0"][w], fx["q_des"][w], fx["obstacles"][w])
                             for w in range(W)], False


def world_sha1(world):
    h = hashlib.sha1()
    for a in world:
        h.update(np.ascontiguousarray(np.asarray(a, dtype=np.float64)).tobytes())
    return h.hexdigest()


def oracle_of(world, T, armtd, threads=8):
    from oracle import OracleArmtd, OraclePlanner

    R = (OracleArmtd if armtd else OraclePlanner)(*world, T=T, threads=threads)
    R.reach()
    return R


FIELDS = ("k_opt", "cost", "status", "feasible", "iterations", "evaluations", "restart_iter")


def plans_of(R, cfg):
    """the clean plan's fields and (dk_noise, dit_noise, dst_noise) of one world under cfg"""
    mu, flags = flags_of(cfg)
    clean = R.plan(mu_strategy=mu, flags=flags)
    dk, dit, dst = 0.0, 0, 0
    for nz in NOISE:
        r = R.plan(mu_strategy=mu, flags=flags, noise=nz)
        dk = max(dk, float(np.abs(r["k_opt"] - clean["k_opt"]).max()))
        dit = max(dit, abs(r["iterations"] - clean["iterations"]))
        dst |= int(r["status"] != clean["status"] or r["feasible"] != clean["feasible"])
    return clean, dk, dit, dst


def generate(golden=False):
    out = {}
    for name, cfgs in CONFIGS.items():
        T, O, worlds, armtd = set_worlds(name)
        out[f"{name}/sha1"] = np.array([world_sha1(w) for w in worlds])
        refs = [oracle_of(w, T, armtd) for w in worlds]
        default = [R.plan() for R in refs]
        for cfg in cfgs:
            rec = {k: [] for k in FIELDS + ("dk_noise", "dit_noise", "dst_noise")}
            for R in refs:
                clean, dk, dit, dst = plans_of(R, cfg)
                for k in FIELDS:
                    rec[k].append(clean[k])
                rec["dk_noise"].append(dk)
                rec["dit_noise"].append(dit)
                rec["dst_noise"].append(dst)
            for k, v in rec.items():
                out[f"{name}/{key(cfg)}/{k}"] = np.array(v)
            k_opt, st = np.array(rec["k_opt"]), np.array(rec["status"])
            d_def = np.abs(k_opt - np.array([r["k_opt"] for r in default])).max(axis=1)
            conv = st == 0
            line = (f"{name} {key(cfg)}: status {np.bincount(st, minlength=5).tolist()} infeasible "
                    f"{int(np.sum(~np.array(rec['feasible'], dtype=bool)))}/{len(refs)} restarts "
                    f"{[(w, int(r)) for w, r in enumerate(rec['restart_iter']) if r >= 0]} "
                    f"evaluations {np.mean(rec['evaluations']):.1f} (default {np.mean([r['evaluations'] for r in default]):.1f}) "
                    f"|dk| from the default, converged worlds: median {np.median(d_def[conv]) if conv.any() else float('nan'):.1e} "
                    f"max dk_noise {max(rec['dk_noise']):.1e} worlds with dit_noise>0 {int(np.sum(np.array(rec['dit_noise']) > 0))}")
            if golden and cfg[0] >= 2:
                mu, flags = flags_of((cfg[0], 0, cfg[2]))  # qf_grid 0: the oracle's golden-section search
                gs = np.array([R.plan(mu_strategy=mu, flags=flags)["k_opt"] for R in refs])
                d = np.abs(k_opt - gs).max(axis=1)
                line += f" |dk| from the golden-section search, converged: median {np.median(d[conv]):.1e}"
            print(line, flush=True)
    return out


if __name__ == "__main__":
    np.savez_compressed(OUT, **generate(golden="--golden" in sys.argv[1:]))
    print("wrote", OUT)
