"""The runs behind tests/golden/sq_parent_*.npy: both reach engines and both bundle-kernel shapes on
the commit before the keep / prune decisions moved to squared norms. Shared by
tools/record_lane_parent.py (`sq` mode, which recorded the fixtures on that commit's build) and
tests/test_gpu_sq_threshold.py (which runs the same on the current build).

Cases (survey worlds):
  t2    1 world,  T = 2,   O = 2:  one bundle with two live lanes (tests/test_gpu_lane_scalar_wave.py)
  t66   1 world,  T = 66,  O = 2:  two bundles, the second with two live lanes
  b100  3 worlds, T = 100, O = 20: case b of lane_onepass_cases.py (5 bundles, two hold two worlds)
Variants: the bundle engine in its wide and dense shapes and the per-job engine.

What is read back, and how it is reduced to digests, is lane_onepass_cases.reach_outputs: reach
outputs, constraint values and Jacobians at three k, monomial counts, the plans, the op dump."""
import os

import numpy as np

import armour_amd as A
import lane_onepass_cases as C

CASES = {"t2": (1, 2, 2, 5300), "t66": (1, 66, 2, 5300), "b100": (3, 100, 20, 5100)}  # worlds, T, O, seed
VARIANTS = {"wide": ("lane", "wide"), "dense": ("lane", "dense"), "job": ("job", None)}
ITEMS = C.ITEMS
GOLDEN = C.GOLDEN
PATHS = {}  # (case, variant, fallback) -> the planner's path census when run_case closed it


def worlds_of(case):
    n, _, O, seed = CASES[case]
    return [A.make_world(seed + s, O, profile="survey") for s in range(n)]


def run_case(case, variant, fallback=False):
    """({item: array}, reach_bytes) of one planner; fallback: ARMOUR_SQ_THRESHOLD=0, the sqrt kernels"""
    _, T, O, _ = CASES[case]
    engine, shape = VARIANTS[variant]
    worlds = worlds_of(case)
    with C.env(ARMOUR_ENGINE=engine, ARMOUR_LANE_SHAPE=shape, ARMOUR_DUMP_OPS="1",
               ARMOUR_SQ_THRESHOLD="0" if fallback else None):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=len(worlds))
    out, nbytes = C.reach_outputs(P, worlds)
    PATHS[case, variant, fallback] = P.path_counts()
    P.close()
    return out, nbytes


def record(out_dir):
    for case in CASES:
        dg, nb, dumps = [], [], []
        for variant in VARIANTS:
            out, b = run_case(case, variant)
            dg.append(C.digests(out))
            nb.append(b)
            dumps.append(out["dump_lane0"])
        np.save(os.path.join(out_dir, f"sq_parent_{case}_digests.npy"), np.stack(dg))
        np.save(os.path.join(out_dir, f"sq_parent_{case}_dump.npy"), np.stack(dumps))
        np.save(os.path.join(out_dir, f"sq_parent_{case}_bytes.npy"), np.array(nb))
        print("sq", case, "reach_bytes", nb, "dump", np.stack(dumps).shape, flush=True)
