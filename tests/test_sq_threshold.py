"""The keep / prune threshold on squared norms (pz_engine.h SqThr, Decide), built for the host as
tests/emu builds the engine headers (tests/sq_unit): the reach engines decide sqrt(S) > thr as
S > S*, with S* the largest double whose square root is still <= thr.

The reference of every comparison is numpy's correctly rounded sqrt applied to S and compared with
thr, in the three polarities the engines use: f > thr, !(f > thr) and !(f <= thr). No mismatch is
allowed anywhere: on the band of +-2^17 ulps around S* and on 2^20 random magnitudes for the robot's
threshold 5e-4, and on the special thresholds 0, a denormal, 1e-160, 1.0, 1e200, inf, a negative
value and NaN, each over its own band and over S = +0, denormals, inf and NaN."""
import ctypes
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
UNIT = os.path.join(HERE, "sq_unit")
THR = 5e-4                                    # robots.cpp planner_defaults: simplify_threshold
S_STAR = float.fromhex("0x1.0c6f7a0b5ed8ep-22")  # thr * thr plus one ulp
DBL_MAX = np.finfo(np.float64).max
SPECIAL_S = np.array([0.0, 5e-324, 1e-310, 2.2250738585072014e-308, 1e-320, 2.5e-7, 1.0, 1e200, DBL_MAX, np.inf, np.nan])
THRESHOLDS = {"robot": THR, "zero": 0.0, "neg_zero": -0.0, "denormal": 5e-324, "1e-160": 1e-160, "one": 1.0,
              "1e200": 1e200, "inf": np.inf, "negative": -3.0, "nan": np.nan}

_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(UNIT, "libsq_check.so")
        if not os.path.exists(so):
            subprocess.run(["make", "-C", UNIT], check=True, capture_output=True)
        L = ctypes.CDLL(so)
        dp = ctypes.POINTER(ctypes.c_double)
        L.sq_host_threshold.argtypes = [ctypes.c_double, dp, ctypes.POINTER(ctypes.c_int)]
        L.sq_host_eval.argtypes = [ctypes.c_double, ctypes.c_double, dp, ctypes.c_longlong, ctypes.POINTER(ctypes.c_ubyte)]
        L.sq_host_frob.argtypes = [dp, ctypes.c_int, dp, dp]
        _lib = L
    return _lib


def threshold(thr):
    s, v = ctypes.c_double(0), ctypes.c_int(0)
    lib().sq_host_threshold(thr, ctypes.byref(s), ctypes.byref(v))
    return s.value, bool(v.value)


def evaluate(thr, s, S):
    S = np.ascontiguousarray(S, dtype=np.float64)
    out = np.zeros(S.size, dtype=np.uint8)
    lib().sq_host_eval(thr, s, S.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), S.size,
                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)))
    return out


def band(s, half):
    """the doubles within `half` ulps of s >= +0, clamped to [+0, +inf]"""
    b = np.array([s], dtype=np.float64).view(np.int64)[0]
    bits = np.clip(b + np.arange(-half, half + 1, dtype=np.int64), 0, np.array([np.inf]).view(np.int64)[0])
    return bits.view(np.float64)


def check(thr, s, S):
    """every polarity of the squared form, of the sqrt form and of the raw constructors' run-time
    form against numpy's sqrt"""
    with np.errstate(invalid="ignore"):
        f = np.sqrt(S)
        gt = f > thr
        nle = ~(f <= thr)
    got = evaluate(thr, s, S)
    for bit, want, name in ((1, gt, "S > S*"), (2, nle, "!(S <= S*)"), (4, gt, "sqrt(S) > thr"), (8, nle, "!(sqrt(S) <= thr)"),
                            (16, nle, "raw form, valid"), (32, nle, "raw form, fallback")):
        have = (got & bit) != 0
        bad = np.flatnonzero(have != want)
        assert bad.size == 0, f"thr {thr!r}: {name} differs at S = {S[bad[:4]]!r} ({bad.size} of {S.size})"
        # !(f > thr), the third polarity, is the complement of the first by construction of the
        # sites (`!thr.gt(S)`); a NaN sum fails both comparisons, so the complement holds there too
        assert np.array_equal(~have, ~want)


def test_robot_threshold_value():
    s, valid = threshold(THR)
    assert valid
    assert s == S_STAR
    assert s == np.nextafter(THR * THR, np.inf)
    assert np.sqrt(s) <= THR < np.sqrt(np.nextafter(s, np.inf))


def test_robot_threshold_band():
    s, _ = threshold(THR)
    check(THR, s, band(s, 1 << 17))


def test_robot_threshold_random_magnitudes():
    s, _ = threshold(THR)
    rng = np.random.default_rng(20240)
    S = 10.0 ** rng.uniform(-12, 3, 1 << 20)
    check(THR, s, S)
    # the same magnitudes as norms: S = f * f lands next to the boundary whenever f is next to thr
    f = THR * (1 + rng.uniform(-1e-12, 1e-12, 1 << 16))
    check(THR, s, f * f)


@pytest.mark.parametrize("name", list(THRESHOLDS))
def test_special_thresholds(name):
    thr = THRESHOLDS[name]
    s, valid = threshold(thr)
    assert valid, "the defining pair holds (or the threshold is a special case): the squared form is used"
    if math.isnan(thr):
        assert math.isnan(s)
    elif thr < 0:
        assert s < 0
    elif thr == np.inf:
        assert s == np.inf
    else:
        # the defining pair, with numpy's sqrt
        assert s >= 0 and np.sqrt(s) <= thr
        assert s == DBL_MAX or thr < np.sqrt(np.nextafter(s, np.inf))
    want = {"zero": 0.0, "neg_zero": 0.0, "denormal": 0.0, "1e-160": 1e-320, "1e200": DBL_MAX, "robot": S_STAR}
    if name in want:
        assert s == want[name]
    S = [SPECIAL_S]
    if s >= 0:
        S.append(band(s, 1 << 12))
    check(thr, s, np.concatenate(S))


def test_special_sums_at_the_robot_threshold():
    s, _ = threshold(THR)
    check(THR, s, SPECIAL_S)
    got = evaluate(THR, s, np.array([0.0, np.nan, np.inf]))
    assert list(got & 3) == [0, 2, 3]  # +0 pruned; NaN: not kept by `>`, kept by `!(<=)`; inf kept


@pytest.mark.parametrize("n", [1, 3, 9])
def test_norm_is_the_root_of_the_same_sum(n):
    rng = np.random.default_rng(n)
    dp = ctypes.POINTER(ctypes.c_double)
    for _ in range(200):
        x = np.ascontiguousarray(rng.normal(size=n) * 10.0 ** rng.integers(-8, 3))
        sq, nm = ctypes.c_double(0), ctypes.c_double(0)
        lib().sq_host_frob(x.ctypes.data_as(dp), n, ctypes.byref(sq), ctypes.byref(nm))
        assert nm.value == np.sqrt(sq.value)
        # Eigen's packet-of-2 redux order (oracle/src/pz.cpp frob_norm)
        q = x * x
        want = q[0] if n == 1 else (q[0] + q[1]) + q[2] if n == 3 else \
            (((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7]))) + q[8]
        assert sq.value == want
