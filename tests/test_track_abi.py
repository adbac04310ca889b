"""armour_track at the C boundary and in the Python binding, without a device: the header declares it,
the built library exports it, the binding binds it with a structure of the header's layout, a call
with null arguments returns ARMOUR_E_ARG with a message (the argument checks come before any device
work), and the binding refuses wrong array shapes."""
import ctypes
import re

import numpy as np
import pytest

import armour_amd as A
from test_abi import HEADER, exported, header_functions, lib_path  # noqa: F401  (lib_path: fixture)


def test_header_declares_and_library_exports(lib_path):
    assert "armour_track" in header_functions()
    assert "armour_track" in exported(lib_path)
    assert "armour_track" in A.ABI_SYMBOLS
    assert A.lib().armour_track.argtypes is not None
    assert callable(A.Planner.track) and callable(A.uncertainty_samples)


def test_structure_follows_the_header():
    src = open(HEADER).read()
    assert re.search(r"#define\s+ARMOUR_TRACK_MAX_STEPS\s+100000\b", src) and A.TRACK_MAX_STEPS == 100000
    body = re.search(r"typedef struct armour_track_output \{(.*?)\} armour_track_output;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [n for n, _ in A.TrackOutput._fields_]
    # seven pointers and a double
    assert ctypes.sizeof(A.TrackOutput) == 8 * 8 and A.TrackOutput.track_ms.offset == 7 * 8


def test_null_arguments_are_refused(lib_path):
    L = A.lib()
    traj = np.zeros((1, 4, 7))
    out = A.TrackOutput()
    assert L.armour_track(None, 1, A._ptr(traj), 1, None, None, 0.0, 0.5, 10, ctypes.byref(out)) == A.ARMOUR_E_ARG
    assert b"null" in L.armour_last_error()
    assert L.armour_track(None, 1, None, 1, None, None, 0.0, 0.5, 10, None) == A.ARMOUR_E_ARG
    assert b"null" in L.armour_last_error()


def test_uncertainty_samples():
    tb = dict(num_joints=8, mass_uncertainty=0.03, inertia_uncertainty=0.05)
    s = A.uncertainty_samples(tb, 6, seed=4)
    assert s.shape == (6, 2, 8)
    assert np.all(s[0] == 1.0)
    assert np.all(s[1, 0] == 1.03) and np.all(s[1, 1] == 1.05)
    assert np.all(s[2, 0] == 0.97) and np.all(s[2, 1] == 0.95)
    assert np.all(np.abs(s[3:, 0] - 1) <= 0.03) and np.all(np.abs(s[3:, 1] - 1) <= 0.05)
    assert len(np.unique(s[3:])) == s[3:].size                      # uniform per link, not per sample
    assert np.array_equal(s, A.uncertainty_samples(tb, 6, seed=4))  # reproducible
    assert A.uncertainty_samples(tb, 1).shape == (1, 2, 8)
    with pytest.raises(ValueError):
        A.uncertainty_samples(tb, 0)


def bare_planner(NJ=7):
    P = object.__new__(A.Planner)
    P.h = None
    P.NJ = NJ
    return P


@pytest.mark.parametrize("shape", [(4, 7), (0, 4, 7), (2, 3, 7), (2, 4, 6)])
def test_track_refuses_wrong_traj_shapes(shape):
    with pytest.raises(ValueError, match="traj"):
        bare_planner().track(np.zeros(shape))


@pytest.mark.parametrize("shape", [(2, 3, 2, 8), (3, 3, 2, 7), (2, 3, 7), (2, 0, 2, 7)])
def test_track_refuses_wrong_scale_shapes(shape):
    with pytest.raises(ValueError, match="scale"):
        bare_planner().track(np.zeros((2, 4, 7)), scale=np.ones(shape))


@pytest.mark.parametrize("shape", [(2, 3, 2, 6), (3, 3, 2, 7), (2, 2, 7), (2, 4, 2, 7)])
def test_track_refuses_wrong_err0_shapes(shape):
    with pytest.raises(ValueError, match="err0"):
        bare_planner().track(np.zeros((2, 4, 7)), scale=np.ones((2, 3, 2, 7)), err0=np.zeros(shape))
