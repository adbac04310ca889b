"""Record tests/golden/rowreduce_parent_<case>.npy: the plans of tests/rowreduce_cases.py (k_opt, cost,
status, iterations, evaluations, kkt, feasible per world). Run on the build whose results are to be
kept (ARMOUR_LIB selects a library); tests/test_gpu_row_reduce_plans.py compares later builds with
it bit for bit.

usage: python tools/record_rowreduce_parent.py [out_dir]   (default tests/golden)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import rowreduce_cases as C  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN
os.makedirs(out_dir, exist_ok=True)
for case in C.CASES:
    rec, paths = C.run_case(case)
    np.save(C.golden_path(case, out_dir), rec)
    st = rec[:, 8].astype(int)
    print(case, "status counts", {int(s): int(np.sum(st == s)) for s in np.unique(st)},
          "paths", {k: v for k, v in paths.items() if v and k.startswith(("da_", "resto_", "ipm_iter", "batch_"))}, flush=True)
