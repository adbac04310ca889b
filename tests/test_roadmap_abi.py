"""The roadmap entries (armour_roadmap_*, armour_episode_roadmap, armour_episode_get_roadmap) at the C boundary
and in the Python binding, without a device: the header declares them and the two structures, the built
library exports them, the binding binds them with structures of the header's layout, and null arguments and
bad configurations are refused with ARMOUR_E_ARG and a message that names the field (the argument checks come
before any device work)."""
import ctypes
import re

import numpy as np
import pytest

import armour_amd as A
from test_abi import HEADER, exported, header_functions, lib_path  # noqa: F401  (lib_path: fixture)

NAMES = ("armour_roadmap_build", "armour_roadmap_get", "armour_roadmap_waypoint", "armour_episode_roadmap",
         "armour_episode_get_roadmap")


def test_header_declares_and_library_exports(lib_path):
    for name in NAMES:
        assert name in header_functions(), name
        assert name in exported(lib_path), name
        assert name in A.ABI_SYMBOLS, name
        assert getattr(A.lib(), name).argtypes is not None, name
    for name in ("roadmap_build", "roadmap", "roadmap_waypoint", "episode_roadmap", "episode_roadmap_state"):
        assert callable(getattr(A.Planner, name)), name
    assert callable(A.roadmap_nodes)


def fields(body):
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            out += [re.sub(r"\[.*?\]", "", part).split()[-1] for part in decl.split(",")]   # (the last word: the name)
    return out


def test_structures_follow_the_header():
    src = open(HEADER).read()
    assert int(re.search(r"#define\s+ARMOUR_ROADMAP_MAX_NODES\s+(\d+)", src).group(1)) == A.ROADMAP_MAX_NODES == 1023
    assert float(re.search(r"#define\s+ARMOUR_ROADMAP_MIN_EDGE\s+(\S+)", src).group(1)) == A.ROADMAP_MIN_EDGE == 1e-6
    cfg = re.search(r"typedef struct armour_roadmap_config \{(.*?)\} armour_roadmap_config;", src, re.S).group(1)
    st = re.search(r"typedef struct armour_roadmap_stats \{(.*?)\} armour_roadmap_stats;", src, re.S).group(1)
    assert fields(cfg) == [n for n, _ in A.RoadmapConfig._fields_]
    assert fields(st) == [n for n, _ in A.RoadmapStats._fields_]
    # an int (+ padding) and three doubles; five long longs, an int (+ padding) and four doubles
    assert ctypes.sizeof(A.RoadmapConfig) == 8 + 3 * 8 and A.RoadmapConfig.connect_radius.offset == 8
    assert ctypes.sizeof(A.RoadmapStats) == 5 * 8 + 8 + 4 * 8 and A.RoadmapStats.build_ms.offset == 48
    for word in ("robot_arm_sampling_based_HLP.m", "strengthening", "ARMOUR_E_CAPACITY", "armour_check_motion"):
        assert word in src, word


def test_null_arguments_are_refused(lib_path):
    L = A.lib()
    cfg = A.RoadmapConfig(100, 1.0, 0.05, 0.02)
    x = np.zeros((1, 100, 7))
    g = np.zeros((1, 7))
    assert L.armour_roadmap_build(None, ctypes.byref(cfg), A._ptr(x), A._ptr(g), None) == A.ARMOUR_E_ARG
    assert b"null" in L.armour_last_error()
    assert L.armour_roadmap_get(None, 0, None, None, None, None, None) == A.ARMOUR_E_ARG
    assert L.armour_roadmap_waypoint(None, A._ptr(g), 0.1, None, None, None) == A.ARMOUR_E_ARG
    assert L.armour_episode_roadmap(None, ctypes.byref(cfg), A._ptr(x)) == A.ARMOUR_E_ARG
    assert L.armour_episode_get_roadmap(None, None, None) == A.ARMOUR_E_ARG
    assert b"null" in L.armour_last_error()


def bare_planner(W):
    P = object.__new__(A.Planner)
    P.h = None
    P._W = W
    return P


@pytest.mark.parametrize("shape", [(100, 7), (3, 100, 7), (2, 100, 6)])
def test_roadmap_build_refuses_wrong_shapes(shape):
    with pytest.raises(ValueError, match="nodes"):
        bare_planner(2).roadmap_build(np.zeros(shape), np.zeros((2, 7)))
    with pytest.raises(ValueError, match="nodes"):
        bare_planner(2).episode_roadmap(np.zeros(shape))


def test_roadmap_build_refuses_wrong_goals_and_queries():
    with pytest.raises(ValueError, match="goals"):
        bare_planner(2).roadmap_build(np.zeros((2, 10, 7)), np.zeros((3, 7)))
    with pytest.raises(ValueError, match="q must"):
        bare_planner(2).roadmap_waypoint(np.zeros((3, 7)))


def test_roadmap_nodes_recipe():
    import episode_model as E

    robot = E.kinova()
    rng = np.random.default_rng(3)
    q0 = np.array([3.0, 2.3, -3.0, -2.5, 0.0, 2.0, 0.0])
    goal = np.array([-3.0, -2.3, 3.0, 2.5, 0.5, -2.0, 0.0])
    nodes = A.roadmap_nodes(robot, q0, goal, 500, 0.3, rng)
    assert nodes.shape == (500, 7)
    lb, ub = robot["state_lb"][:7], robot["state_ub"][:7]
    lim = lb > -1000.0
    assert np.all(nodes[:, lim] >= lb[lim]) and np.all(nodes[:, lim] <= ub[lim])
    assert np.any(nodes[:, 1] == ub[1]) and np.any(nodes[:, 1] == lb[1])       # clipped at both ends
    # joint 0 is continuous: the tube follows the short way round (3.0 -> -3.0 across pi), not through 0
    assert np.all(np.abs(nodes[:, 0]) > 3.0 - 5 * 0.3)
