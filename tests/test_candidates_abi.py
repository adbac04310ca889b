"""armour_eval_candidates at the C boundary and in the Python binding, without a device: the header
declares the entry, the built library exports it, and Planner.eval_candidates refuses a wrong shape,
a non-finite value and a value outside [-1, 1] with ValueError before the library is called."""
import numpy as np
import pytest

import armour_amd as A
from test_abi import exported, header_functions, lib_path  # noqa: F401  (lib_path: fixture)

NAME = "armour_eval_candidates"


def test_header_declares_and_library_exports(lib_path):
    assert NAME in header_functions()
    assert NAME in exported(lib_path)
    assert NAME in A.ABI_SYMBOLS
    assert A.lib().armour_eval_candidates.argtypes is not None


def bare_planner(W):
    """a Planner object that never reached the library (no device here): any call into it would fail
    on the null handle, so a ValueError shows the check came first"""
    P = object.__new__(A.Planner)
    P.h = None
    P._W = W
    return P


@pytest.mark.parametrize("shape", [(7,), (3, 6), (2, 3, 8), (3, 4, 7), (2, 0, 7), (0, 7), (2, 2, 2, 7)])
def test_wrong_shapes(shape):
    with pytest.raises(ValueError, match="shape"):
        bare_planner(2).eval_candidates(np.zeros(shape))


def test_shared_candidates_need_a_batch():
    with pytest.raises(ValueError, match="batch"):
        bare_planner(0).eval_candidates(np.zeros((4, 7)))


@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_non_finite(bad):
    x = np.zeros((2, 5, 7))
    x[1, 4, 6] = bad
    with pytest.raises(ValueError, match="non-finite"):
        bare_planner(2).eval_candidates(x)


@pytest.mark.parametrize("bad", [1.0 + 1e-12, -1.0 - 1e-12, 3.0])
def test_outside_the_box(bad):
    x = np.zeros((5, 7))
    x[2, 0] = bad
    with pytest.raises(ValueError, match=r"\[-1, 1\]"):
        bare_planner(3).eval_candidates(x)


def test_accepted_forms():
    x = A.candidates_array(np.ones((4, 7)), 3)          # [N, 7]: the same candidates for every world
    assert x.shape == (3, 4, 7) and x.flags["C_CONTIGUOUS"] and x.dtype == np.float64
    y = A.candidates_array(-np.ones((3, 4, 7), dtype=np.float32), 3)
    assert y.shape == (3, 4, 7) and y.dtype == np.float64
