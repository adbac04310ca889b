"""Record tests/golden/lane_parent_*.npy: the bundle engine's reach outputs, op dump and reach_bytes
on the cases of tests/lane_onepass_cases.py, in both kernel shapes. Run on the build whose results
are to be kept (ARMOUR_LIB selects a library); tests/test_gpu_lane_onepass.py compares later builds
with it bit for bit.

Per case: lane_parent_<case>_digests.npy [2 shapes][items][32] sha256 of every read-back array,
lane_parent_<case>_dump.npy [nops][8] op dump of job 0 (dense shape), lane_parent_<case>_bytes.npy
[2] reach_bytes.

`sq` mode records tests/golden/sq_parent_*.npy instead: the cases of tests/sq_threshold_cases.py on
the bundle engine's two shapes and on the per-job engine (per case: digests [3 variants][items][32],
op dumps of job 0 [3][nops][8], reach_bytes [3]); tests/test_gpu_sq_threshold.py compares with them.

usage: python tools/record_lane_parent.py [sq] [out_dir]   (default tests/golden)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lane_onepass_cases as C  # noqa: E402

sq = sys.argv[1:2] == ["sq"]
if sq:
    del sys.argv[1]
out_dir = sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN
os.makedirs(out_dir, exist_ok=True)
if sq:
    import sq_threshold_cases as Q  # noqa: E402

    Q.record(out_dir)
    sys.exit(0)
for case in C.CASES:
    dg, nb, dump = [], [], None
    for shape in C.SHAPES:
        d, dump, b, _ = C.run_case(case, shape)
        dg.append(d)
        nb.append(b)
    np.save(os.path.join(out_dir, f"lane_parent_{case}_digests.npy"), np.stack(dg))
    np.save(os.path.join(out_dir, f"lane_parent_{case}_dump.npy"), dump)
    np.save(os.path.join(out_dir, f"lane_parent_{case}_bytes.npy"), np.array(nb))
    print(case, "reach_bytes", nb, "shapes agree", bool(np.array_equal(dg[0], dg[1])), "dump", dump.shape, flush=True)
