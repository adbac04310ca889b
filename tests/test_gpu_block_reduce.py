"""The row passes' block reduction on the device (tests/reduce_unit: block_reduce.h's block_reduce_n at
256 threads with every call site's width and kinds, beside a verbatim copy of the butterfly form it
replaced). Every output is bit-equal to that copy and to the numpy tree (reduce_model: xor levels
1 .. 32 per wave, then the waves in order), on inputs that tell associations and lanes apart.

Where the comparison is not by bits, and why:
  a NaN among a sum slot's inputs, or +inf and -inf in one sum slot: the total is a NaN, whose sign
    and payload IEEE 754 leaves open (numpy's host and the device choose differently); NaN-ness is
    required, and every other slot's bits;
  a max / min slot whose result is a zero, against numpy only: maxNum / minNum leave the sign of
    max(+0, -0) open; against the parent copy these slots are compared by bits like all others."""
import ctypes
import os

import numpy as np
import pytest

import reduce_model as M

pytestmark = pytest.mark.gpu
UNIT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "reduce_unit")
WIDTHS = (1, 2, 7, 19, 37, 55)   # the call sites' widths (nlp_kernels.hip); no fused width is used
BLOCKS, THREADS = 64, 256
MAX_START, MIN_START = 0.0, 1e300   # the max / min accumulators' start values (sums start at 0)


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(os.path.join(UNIT, "libreduce_test.so"))
    L.reduce_run.argtypes = [ctypes.c_int, ctypes.c_int] + [ctypes.c_void_p] * 3
    return L


def kinds_of(L, N):
    return [L.reduce_site_kind(N, k) for k in range(N)]


def run(L, N, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    assert x.shape == (BLOCKS, THREADS, N)
    new, old = np.empty((BLOCKS, N)), np.empty((BLOCKS, N))
    rc = L.reduce_run(N, BLOCKS, x.ctypes.data, new.ctypes.data, old.ctypes.data)
    assert rc == 0, rc
    return new, old


def mixed(rng, shape):
    return rng.choice([-1.0, 1.0], shape) * 10.0 ** rng.uniform(-30, 30, shape)


def inputs(name, N, kinds, rng):
    shape = (BLOCKS, THREADS, N)
    if name == "mixed":
        return mixed(rng, shape)
    if name == "zeros":
        return np.zeros(shape)
    if name == "signed_zeros":
        return rng.choice([0.0, -0.0], shape)
    if name == "subnormals":
        return rng.choice([-1.0, 1.0], shape) * rng.integers(0, 1 << 20, shape) * 5e-324
    if name == "idle_lanes":
        # most threads had no row: they hold the accumulators' start values
        x = mixed(rng, shape)
        idle = rng.random((BLOCKS, THREADS, 1)) < 0.7
        idle[: BLOCKS // 4] = np.arange(THREADS)[None, :, None] >= 5   # one row block, 5 busy threads
        start = np.array([0.0 if k == 0 else MAX_START if k == 1 else MIN_START for k in kinds])
        # the busy lanes of a max slot are non-negative, those of a min slot below its start
        x = np.where(np.array(kinds) == 1, np.abs(x), x)
        return np.where(idle, start, x)
    if name == "inf":
        x = mixed(rng, shape)
        # per block and slot: no inf, +inf only, -inf only, or both (a sum slot then totals NaN)
        mode = rng.integers(0, 4, (BLOCKS, 1, N))
        hit = rng.random(shape) < 0.02
        sign = np.where(mode == 1, 1.0, np.where(mode == 2, -1.0, rng.choice([-1.0, 1.0], shape)))
        return np.where(hit & (mode > 0), sign * np.inf, x)
    if name == "nan":
        x = mixed(rng, shape)
        sums = [k for k in range(N) if kinds[k] == 0]
        for b in range(BLOCKS):
            x[b, rng.integers(THREADS), sums[b % len(sums)]] = np.nan
        return x
    raise AssertionError(name)


CASES = ("mixed", "zeros", "signed_zeros", "subnormals", "idle_lanes", "inf", "nan")


@pytest.mark.parametrize("N", WIDTHS)
def test_block_reduce_bits(lib, N):
    kinds = kinds_of(lib, N)
    assert kinds == {55: [1 if 7 <= k <= 9 else 2 if k == 54 else 0 for k in range(55)], 19: [2, 2] + [0] * 17,
                     37: [0] * 36 + [1]}.get(N, [0] * N)
    rng = np.random.default_rng(1000 + N)
    karr = np.array(kinds)
    for name in CASES:
        x = inputs(name, N, kinds, rng)
        new, old = run(lib, N, x)
        ref = M.block_reduce(x, kinds)
        nb, ob, rb = M.bits(new), M.bits(old), M.bits(ref)
        print(f"N={N} {name}: differing from parent {int(np.sum(nb != ob))}, from numpy {int(np.sum(nb != rb))} of {nb.size}; "
              f"NaN outputs {int(np.isnan(new).sum())}")
        if name in ("inf", "nan"):
            nan_ok = np.isnan(ref) & (karr == 0)[None, :]
            assert np.array_equal(np.isnan(new), np.isnan(ref)) and np.array_equal(np.isnan(old), np.isnan(ref)), name
            if name == "nan":
                assert nan_ok.sum() == BLOCKS and np.array_equal(np.isnan(ref), nan_ok)
            else:
                assert nan_ok.sum() > 0
        else:
            nan_ok = np.zeros_like(new, dtype=bool)
            assert not np.isnan(new).any() and not np.isnan(ref).any(), name
        assert np.array_equal(nb[~nan_ok], ob[~nan_ok]), (name, "parent copy")
        zero_extremum = (karr != 0)[None, :] & (new == 0) & (ref == 0)
        strict = ~nan_ok & ~zero_extremum
        assert np.array_equal(nb[strict], rb[strict]), (name, "numpy tree")
        if name == "mixed":
            # the data can fail: the same tree with its levels reversed gives other bits
            rev = M.block_reduce(x, kinds, levels=M.LEVELS[::-1])
            s = karr == 0
            differ = np.mean(M.bits(rev[:, s]) != rb[:, s])
            print(f"N={N}: levels reversed differ in {differ:.0%} of the sums")
            assert differ > 0.25, differ
