"""The reach engines with their keep / prune decisions on squared norms (pz_engine.h SqThr).

The device's own self-check (armour_sq_selfcheck): for thr = 5e-4, 1e-160 and 1.0 the squared
threshold is verified and sqrt(S) against thr and S against S* decide alike on the 2 * 65536 + 1
doubles around S* and on 2^20 random magnitudes.

The runs of sq_threshold_cases.py (nearly empty bundles at T = 2 and T = 66, a 3-world batch at
T = 100; both engines, both bundle shapes) equal, bit for bit, what the commit before recorded in
tests/golden/sq_parent_*.npy: reach outputs, op dumps, reach_bytes and plans. The two shapes agree
with each other, and the forced fallback (ARMOUR_SQ_THRESHOLD=0: the sqrt kernels) with the default."""
import os

import numpy as np
import pytest

import armour_amd as A
import sq_threshold_cases as Q
from paths import assert_paths

pytestmark = pytest.mark.gpu
S_STAR = float.fromhex("0x1.0c6f7a0b5ed8ep-22")  # tests/test_sq_threshold.py

_runs = {}


def run(case, variant, fallback=False):
    """one run per (case, variant, fallback), shared by the tests below and left unchanged"""
    key = (case, variant, fallback)
    if key not in _runs:
        _runs[key] = Q.run_case(case, variant, fallback)
    # the run took the engine and shape of its variant, and the sqrt kernels only as the forced fallback
    mine = {"wide": "reach_lane_wide", "dense": "reach_lane_dense", "job": ("reach_job_256", "reach_job_128")}[variant]
    others = tuple(n for n in ("reach_lane_wide", "reach_lane_dense", "reach_job_256", "reach_job_128") if n not in mine)
    assert_paths(Q.PATHS[key], ran=(mine, "reach_sqrt" if fallback else "reach_sq"),
                 not_ran=others + ("reach_sq" if fallback else "reach_sqrt",))
    return _runs[key]


def golden(case, what):
    return np.load(os.path.join(Q.GOLDEN, f"sq_parent_{case}_{what}.npy"))


@pytest.mark.parametrize("thr", [5e-4, 1e-160, 1.0])
def test_device_selfcheck(thr):
    rng = np.random.default_rng(20240)
    values = 10.0 ** rng.uniform(-12, 3, 1 << 20)
    s, valid, bad = A.sq_selfcheck(thr, 65536, values)
    assert valid
    assert bad == 0
    assert np.sqrt(s) <= thr < np.sqrt(np.nextafter(s, np.inf))
    if thr == 5e-4:
        assert s == S_STAR
    if thr == 1e-160:
        assert s == 1e-320


@pytest.mark.parametrize("variant", list(Q.VARIANTS))
@pytest.mark.parametrize("case", list(Q.CASES))
def test_equals_parent_recording(case, variant):
    out, nbytes = run(case, variant)
    v = list(Q.VARIANTS).index(variant)
    # the op dump in full first: a differing op is a better message than a differing digest
    np.testing.assert_array_equal(out["dump_lane0"], golden(case, "dump")[v])
    dg, want = Q.C.digests(out), golden(case, "digests")[v]
    assert want.shape == dg.shape
    differ = [k for i, k in enumerate(Q.ITEMS) if not np.array_equal(dg[i], want[i])]
    assert not differ, differ
    assert nbytes == golden(case, "bytes")[v]


@pytest.mark.parametrize("case", list(Q.CASES))
def test_shapes_agree_bitwise(case):
    (a, na), (b, nb) = run(case, "wide"), run(case, "dense")
    for k in Q.ITEMS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert na == nb


@pytest.mark.parametrize("variant", list(Q.VARIANTS))
@pytest.mark.parametrize("case", list(Q.CASES))
def test_forced_fallback_equals_default(case, variant):
    (a, na), (b, nb) = run(case, variant), run(case, variant, fallback=True)
    for k in Q.ITEMS:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert na == nb
