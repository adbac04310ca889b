"""The bundle engine after cross_const became one compacting pass: the runs of lane_onepass_cases.py
equal, bit for bit, what the commit before recorded in tests/golden/lane_parent_*.npy (reach outputs,
op dump, reach_bytes, in both kernel shapes); the capacity retry still plans bitwise as the default
capacities do; the two shapes agree on the reach outputs."""
import os

import numpy as np
import pytest

import lane_onepass_cases as C
from paths import assert_paths

pytestmark = pytest.mark.gpu


def golden(case, what):
    return np.load(os.path.join(C.GOLDEN, f"lane_parent_{case}_{what}.npy"))


_runs = {}


def run(case, shape):
    """one run per (case, shape), shared by the tests below and left unchanged"""
    if (case, shape) not in _runs:
        _runs[case, shape] = C.run_case(case, shape)
    assert_paths(C.PATHS[case, shape], **shape_paths(shape))
    return _runs[case, shape]


def shape_paths(shape):
    """assert_paths' arguments for a bundle-engine planner of one kernel shape"""
    other = "dense" if shape == "wide" else "wide"
    return dict(ran=("reach_lane_" + shape,), not_ran=("reach_lane_" + other, "reach_job_256", "reach_job_128"))


@pytest.mark.parametrize("shape", C.SHAPES)
@pytest.mark.parametrize("case", C.CASES)
def test_equals_parent_recording(case, shape):
    dg, dump, nbytes, _ = run(case, shape)
    want = golden(case, "digests")[C.SHAPES.index(shape)]
    assert want.shape == dg.shape
    # the op dump in full first: a differing op is a better message than a differing digest
    np.testing.assert_array_equal(dump, golden(case, "dump"))
    differ = [k for i, k in enumerate(C.ITEMS) if not np.array_equal(dg[i], want[i])]
    assert not differ, differ
    assert nbytes == golden(case, "bytes")[C.SHAPES.index(shape)]


def test_shapes_agree_on_reach_outputs():
    a, b = run("b", "wide")[3], run("b", "dense")[3]
    for k in C.ITEMS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert run("b", "wide")[2] == run("b", "dense")[2]


@pytest.mark.parametrize("shape", C.SHAPES)
def test_capacity_retry_plans_bitwise(shape):
    """case b with the arena at a quarter (plus a margin of 64) of what its largest bundle uses: every
    bundle overflows the first launch (the error flag marks all three worlds, once), the retry's
    fourfold arena holds the largest bundle, and what comes out equals the run with default capacities"""
    ref = run("b", shape)[3]
    P, worlds = C.planner("b", shape, dump=False)
    P.reach(worlds)
    occ = P.occupancy()
    assert_paths(P.path_counts(), ran=shape_paths(shape)["ran"], not_ran=("reach_retry",))
    P.close()
    assert occ["worlds_retried"][0] == 0
    hcap, ccap = occ["arena_hashes"][0] // 4 + 64, occ["arena_rows"][0] // 4 + 64
    P, worlds = C.planner("b", shape, dump=False, hcap=hcap, ccap=ccap)
    # (reach_bytes is not compared here: the overflowed first launch adds the bytes of the operators
    # it ran before the overflow, and where a bundle overflows depends on the arena size)
    out, _ = C.reach_outputs(P, worlds, dump=False)
    occ = P.occupancy()
    # reach_outputs reaches once and plans once: one retry launch each, in the shape of the first launch
    paths = P.path_counts()
    P.close()
    assert occ["worlds_retried"][0] == 3 and occ["worlds_failed"][0] == 0
    assert_paths(paths, exactly={"reach_retry": 2, "reach_lane_" + shape: 4}, **shape_paths(shape))
    for k in C.ITEMS:
        if not k.startswith("dump"):
            np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
