"""Record tests/golden/lane_parent_*.npy: the bundle engine's reach outputs, op dump and reach_bytes
on the cases of tests/lane_onepass_cases.py, in both kernel shapes. Run on the build whose results
are to be kept (ARMOUR_LIB selects a library); tests/test_gpu_lane_onepass.py compares later builds
with it bit for bit.

Per case: lane_parent_<case>_digests.npy [2 shapes][items][32] sha256 of every read-back array,
lane_parent_<case>_dump.npy [nops][8] op dump of job 0 (dense shape), lane_parent_<case>_bytes.npy
[2] reach_bytes.

usage: python tools/record_lane_parent.py [out_dir]   (default tests/golden)"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import lane_onepass_cases as C  # noqa: E402

out_dir = sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN
os.makedirs(out_dir, exist_ok=True)
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
