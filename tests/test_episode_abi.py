"""armour_check_motion and the armour_episode_* entries at the C boundary and in the Python binding,
without a device: the header declares them, the built library exports them, the binding binds them
with structures of the header's layout, and a call with null arguments returns ARMOUR_E_ARG with a
message (the argument checks come before any device work)."""
import ctypes
import re

import numpy as np
import pytest

import armour_amd as A
from test_abi import HEADER, exported, header_functions, lib_path  # noqa: F401  (lib_path: fixture)

NAMES = ("armour_check_motion", "armour_episode_begin", "armour_episode_step", "armour_episode_get")


def test_header_declares_and_library_exports(lib_path):
    for name in NAMES:
        assert name in header_functions(), name
        assert name in exported(lib_path), name
        assert name in A.ABI_SYMBOLS, name
        assert getattr(A.lib(), name).argtypes is not None, name
    for name in ("check_motion", "episode_begin", "episode_step", "episode_states"):
        assert callable(getattr(A.Planner, name)), name
    assert callable(A.run_episodes)


def test_structures_follow_the_header():
    src = open(HEADER).read()
    assert re.search(r"#define\s+ARMOUR_T_PLAN\s+0\.5\b", src) and A.T_PLAN == 0.5
    cfg = re.search(r"typedef struct armour_episode_config \{(.*?)\} armour_episode_config;", src, re.S).group(1)
    st = re.search(r"typedef struct armour_episode_state \{(.*?)\} armour_episode_state;", src, re.S).group(1)

    def fields(body):
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        out = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                out += [re.sub(r"\[.*?\]", "", n).strip() for n in decl.split(None, 1)[1].split(",")]
        return out

    assert fields(cfg) == [n for n, _ in A.EpisodeConfig._fields_]
    assert fields(st) == [n for n, _ in A.EpisodeState._fields_]
    # 4 x 7 doubles, 5 ints (+ padding), a double, 3 ints (+ padding), a double
    assert ctypes.sizeof(A.EpisodeState) == 28 * 8 + 24 + 8 + 16 + 8
    assert A.EpisodeState.clearance.offset == 28 * 8 + 24 and A.EpisodeState.goal_distance.offset == 28 * 8 + 24 + 8 + 16


def test_null_arguments_are_refused(lib_path):
    L = A.lib()
    traj = np.zeros((1, 4, 7))
    clear = np.zeros(1)
    where = np.zeros(3, dtype=np.int32)
    ip = ctypes.POINTER(ctypes.c_int)
    assert L.armour_check_motion(None, A._ptr(traj), 0.0, 1.0, 3, A._ptr(clear), where.ctypes.data_as(ip)) == A.ARMOUR_E_ARG
    assert b"null" in L.armour_last_error()
    cfg = A.EpisodeConfig(0.1, np.pi / 30, 11)
    world = (A.World * 1)()
    goals = np.zeros((1, 7))
    assert L.armour_episode_begin(None, 1, world, A._ptr(goals), ctypes.byref(cfg)) == A.ARMOUR_E_ARG
    assert L.armour_episode_step(None, None, None, None, None) == A.ARMOUR_E_ARG
    assert L.armour_episode_get(None, None) == A.ARMOUR_E_ARG
    assert b"null" in L.armour_last_error()


def bare_planner(W):
    P = object.__new__(A.Planner)
    P.h = None
    P._W = W
    return P


@pytest.mark.parametrize("shape", [(4, 7), (2, 3, 7), (3, 4, 7), (2, 4, 6)])
def test_check_motion_refuses_wrong_shapes(shape):
    with pytest.raises(ValueError, match="shape"):
        bare_planner(2).check_motion(np.zeros(shape))


def test_episode_begin_refuses_wrong_goals():
    worlds = [A.make_world(s, 2) for s in range(2)]
    with pytest.raises(ValueError, match="goals"):
        bare_planner(0).episode_begin(worlds, np.zeros((3, 7)))
