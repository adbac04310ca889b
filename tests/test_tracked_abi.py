"""armour_track_motion, armour_episode_track and armour_episode_get_tracked at the C boundary and in the
Python binding, without a device: the header declares them, the built library exports them, the binding
binds them with structures of the header's layout, a call
with null arguments or with a `steps` that is no multiple of check_samples - 1 returns ARMOUR_E_ARG with
a message (these checks come before any device work), and the binding refuses wrong array shapes."""
import ctypes
import re

import numpy as np
import pytest

import armour_amd as A
from test_abi import HEADER, exported, header_functions, lib_path  # noqa: F401  (lib_path: fixture)


NEW = ("armour_track_motion", "armour_episode_track", "armour_episode_get_tracked")


def test_header_declares_and_library_exports(lib_path):
    for name in NEW:
        assert name in header_functions(), name
        assert name in exported(lib_path), name
        assert name in A.ABI_SYMBOLS, name
        assert getattr(A.lib(), name).argtypes is not None, name
    assert callable(A.Planner.track_motion) and callable(A.Planner.episode_track) and callable(A.Planner.episode_tracked)


def struct_names(src, name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        if decl.strip():
            first, *more = decl.split(",")
            names += [re.sub(r"\[.*", "", v.split()[-1].lstrip("*")) for v in [first] + more]
    return names


def test_episode_structures_follow_the_header():
    src = open(HEADER).read()
    assert struct_names(src, "armour_episode_track_config") == [n for n, _ in A.EpisodeTrackConfig._fields_]
    assert struct_names(src, "armour_episode_tracked") == [n for n, _ in A.EpisodeTracked._fields_]
    # int, two pointers, four ints; a double, 4 ints, 23 doubles, 6 ints
    assert ctypes.sizeof(A.EpisodeTrackConfig) == 8 + 2 * 8 + 4 * 4
    assert ctypes.sizeof(A.EpisodeTracked) == 8 + 16 + 23 * 8 + 24 and A.EpisodeTracked.flags.offset == 8 + 16 + 23 * 8
    assert len(A.EPISODE_STATUS) == 9


def test_episode_entries_refuse_null_arguments(lib_path):
    L = A.lib()
    cfg = A.EpisodeTrackConfig(1, None, None, 10, 1, 1, 0)
    assert L.armour_episode_track(None, ctypes.byref(cfg)) == A.ARMOUR_E_ARG and b"null" in L.armour_last_error()
    rec = (A.EpisodeTracked * 1)()
    assert L.armour_episode_get_tracked(None, rec, None, None, None) == A.ARMOUR_E_ARG and b"null" in L.armour_last_error()


@pytest.mark.parametrize("kw, word", [(dict(scale=np.ones((3, 2, 2, 7))), "scale"), (dict(scale=np.ones((2, 2, 8))), "scale"),
                                      (dict(err0=np.zeros((2, 2, 7))), "err0"),
                                      (dict(scale=np.ones((2, 3, 2, 7)), err0=np.zeros((2, 2, 2, 7))), "err0"),
                                      (dict(scale=np.ones((2, 3, 2, 7)), num_samples=2), "num_samples")])
def test_episode_track_refuses_wrong_shapes(kw, word):
    with pytest.raises(ValueError, match=word):
        bare_planner().episode_track(**kw)


def test_structure_and_flags_follow_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct armour_track_motion_output \{(.*?)\} armour_track_motion_output;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [decl.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip()]
    assert names == [n for n, _ in A.TrackMotionOutput._fields_]
    # the embedded armour_track_output, five pointers and a double
    assert A.TrackMotionOutput.track.offset == 0 and A.TrackMotionOutput.clearance.offset == ctypes.sizeof(A.TrackOutput)
    assert ctypes.sizeof(A.TrackMotionOutput) == ctypes.sizeof(A.TrackOutput) + 6 * 8
    for name, bit in (("COLLISION", 1), ("INPUT", 2), ("BOUND", 4), ("LIMIT", 8), ("NOT_FINITE", 16)):
        assert re.search(rf"#define\s+ARMOUR_TRACK_{name}\s+{bit}\b", src), name
        assert getattr(A, "TRACK_" + name) == bit


def _call(p, traj, steps, check_samples, out=True):
    o = A.TrackMotionOutput()
    rc = A.lib().armour_track_motion(p, A._ptr(traj) if traj is not None else None, 1, None, None, 0.0, 0.5, steps,
                                     check_samples, ctypes.byref(o) if out else None)
    return rc, A.lib().armour_last_error()


def test_null_arguments_are_refused(lib_path):
    traj = np.zeros((1, 4, 7))
    for args in ((None, traj, 10, 11), (None, None, 10, 11)):
        rc, msg = _call(*args)
        assert rc == A.ARMOUR_E_ARG and b"null" in msg
    rc, msg = _call(None, traj, 10, 11, out=False)
    assert rc == A.ARMOUR_E_ARG and b"null" in msg


@pytest.mark.parametrize("steps, check_samples, word", [(10, 4, b"multiple"), (50, 12, b"multiple"), (7, 3, b"multiple"),
                                                       (10, 1, b"check_samples"), (10, 0, b"check_samples"),
                                                       (10, -3, b"check_samples")])
def test_steps_and_check_samples_that_do_not_fit_are_refused(lib_path, steps, check_samples, word):
    rc, msg = _call(None, np.zeros((1, 4, 7)), steps, check_samples)
    assert rc == A.ARMOUR_E_ARG and word in msg, msg


def bare_planner(W=2, NJ=7):
    P = object.__new__(A.Planner)
    P.h = None
    P.NJ = NJ
    P._W = W
    return P


@pytest.mark.parametrize("shape", [(4, 7), (0, 4, 7), (3, 4, 7), (1, 4, 7), (2, 3, 7), (2, 4, 6)])
def test_track_motion_refuses_wrong_traj_shapes(shape):
    with pytest.raises(ValueError, match="traj"):
        bare_planner().track_motion(np.zeros(shape))


@pytest.mark.parametrize("shape", [(2, 3, 2, 8), (3, 3, 2, 7), (2, 3, 7), (2, 0, 2, 7)])
def test_track_motion_refuses_wrong_scale_shapes(shape):
    with pytest.raises(ValueError, match="scale"):
        bare_planner().track_motion(np.zeros((2, 4, 7)), scale=np.ones(shape))


@pytest.mark.parametrize("shape", [(2, 3, 2, 6), (3, 3, 2, 7), (2, 2, 7), (2, 4, 2, 7)])
def test_track_motion_refuses_wrong_err0_shapes(shape):
    with pytest.raises(ValueError, match="err0"):
        bare_planner().track_motion(np.zeros((2, 4, 7)), scale=np.ones((2, 3, 2, 7)), err0=np.zeros(shape))
