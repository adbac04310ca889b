"""Plans through the row passes' block reduction (block_reduce.h: reduce-scatter sums) against the
record of the build before it (tests/golden/rowreduce_parent_*.npy, tools/record_rowreduce_parent.py):
every recorded field of every world bit for bit. The cases (tests/rowreduce_cases.py) reach each
call site's forms: one row block with most threads idle, a partial last block, the mixed-batch (_mx)
kernels with a world of no obstacle, one world on the tail path in the register form, and a grid wide
enough for ipm_rows_DA_lds; the survey worlds include locally infeasible ones (status 4), whose
restoration phases run resto_rows_G and resto_rows_V."""
import numpy as np
import pytest

import rowreduce_cases as C
from paths import assert_paths

pytestmark = pytest.mark.gpu

PATHS = {
    "one_block": dict(ran=("batch_uniform", "da_regs"), not_ran=("da_lds", "batch_mixed")),
    "two_blocks": dict(ran=("batch_uniform", "da_regs"), not_ran=("da_lds", "batch_mixed")),
    "mixed": dict(ran=("batch_mixed", "da_regs"), not_ran=("da_lds", "batch_uniform")),
    "one_world": dict(ran=("ipm_iter_tail", "da_regs"), not_ran=("da_lds",)),
    "wide": dict(ran=("da_lds", "da_regs", ("resto_inline", "resto_after_loop"))),
}
# every case holds a world ending locally infeasible (status 4: its restoration phase ran)
INFEASIBLE = tuple(C.CASES)


@pytest.mark.parametrize("case", list(C.CASES))
def test_plans_match_the_parent_record(case):
    ref = np.load(C.golden_path(case))
    rec, paths = C.run_case(case)
    assert_paths(paths, **PATHS[case])
    assert rec.shape == ref.shape == (C.CASES[case][2], 13)
    st, st_ref = rec[:, 8].astype(int), ref[:, 8].astype(int)
    counts = {int(s): int(np.sum(st == s)) for s in np.unique(st)}
    counts_ref = {int(s): int(np.sum(st_ref == s)) for s in np.unique(st_ref)}
    print(case, "status counts", counts, "recorded", counts_ref)
    assert counts == counts_ref
    if case in INFEASIBLE:
        assert counts.get(4, 0) >= 1, "no world in the restoration phase"
    names = ["k_opt"] * 7 + ["cost", "status", "iterations", "evaluations", "kkt", "feasible"]
    bad = sorted({(w, names[j]) for w, j in zip(*np.nonzero(rec.view(np.uint64) != ref.view(np.uint64)))})
    assert not bad, f"{len(bad)} fields differ from the parent record, first {bad[:8]}"
