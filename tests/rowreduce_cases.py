"""Cases of tests/test_gpu_row_reduce_plans.py and tools/record_rowreduce_parent.py: plans whose row
passes reduce through every form of the block reduction's call sites, recorded on the build before
the reduce-scatter (tests/golden/rowreduce_parent_<case>.npy) and compared with later builds bit for
bit. A world's rows: 7 T torque + 7 T O collision + 28 extremum rows + 7 variables, in row blocks of
1024 (row_chunk) on 256 threads."""
import os

import numpy as np

import armour_amd as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MIXED_O = (0, 1, 6, 3)
# name: (T, max obstacles, worlds, mixed obstacle counts)
CASES = {
    "one_block": (10, 3, 8, False),    # 315 rows: one row block, most threads with one row or none
    "two_blocks": (30, 6, 8, False),   # 1505 rows: two blocks, the last one partial
    "mixed": (30, 6, 8, True),         # plan_mixed with a world of no obstacle: the _mx kernels
    "one_world": (30, 6, 1, False),    # the tail's launches, register form
    "wide": (100, 20, 72, False),      # 15 blocks x 72 worlds >= 4 x CUs: ipm_rows_DA_lds
}
FIELDS = ("k_opt", "cost", "status", "iterations", "evaluations", "kkt")


def worlds_of(case):
    T, O, W, mixed = CASES[case]
    worlds = [A.make_world(s, O, profile="survey") for s in range(W)]
    if mixed:
        worlds = [w[:4] + (w[4][:MIXED_O[i % len(MIXED_O)]],) for i, w in enumerate(worlds)]
    return worlds


def run_case(case):
    """(record [W, 13] doubles: k_opt 7, cost, status, iterations, evaluations, kkt, feasible; path counts)"""
    T, O, W, mixed = CASES[case]
    worlds = worlds_of(case)
    P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    res, _ = (P.plan_mixed if mixed else P.plan)(worlds)
    paths = P.path_counts()
    P.close()
    rec = np.array([list(r["k_opt"]) + [r["cost"], r["status"], r["iterations"], r["evaluations"], r["kkt"], float(r["feasible"])]
                    for r in res], dtype=np.float64)
    return rec, paths


def golden_path(case, out_dir=GOLDEN):
    return os.path.join(out_dir, f"rowreduce_parent_{case}.npy")
