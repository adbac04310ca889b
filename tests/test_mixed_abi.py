"""Mixed batches (worlds with different numbers of obstacles) at the boundary, without a device: the
three entry points are declared in include/armour_hip.h, listed in the binding and exported by the
library; the Planner has plan_mixed / reach_mixed; and a mixed list marshals into armour_world
records that keep each world's own count and obstacle block."""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import armour_amd as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "armour_hip.h")
MIXED = ("armour_plan_batch_mixed", "armour_reach_batch_mixed", "armour_world_num_obstacles")


@pytest.fixture(scope="module")
def lib_path():
    if not os.path.exists(A.LIB_PATH):
        subprocess.run(["make", "-C", os.path.join(ROOT, "armour-dev_amd", "csrc"), "../armour_amd/libarmour_hip.so"],
                       check=True, capture_output=True)
    return A.LIB_PATH


def test_mixed_symbols_declared_bound_and_exported(lib_path):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(armour_\w+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], check=True, capture_output=True, text=True).stdout
    exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    L = A.lib()
    for name in MIXED:
        assert name in declared, name
        assert name in A.ABI_SYMBOLS, name
        assert name in exported, name
        assert hasattr(L, name), name
    # the mixed entries take what the uniform ones take
    assert L.armour_plan_batch_mixed.argtypes == L.armour_plan_batch.argtypes
    assert L.armour_reach_batch_mixed.argtypes == L.armour_reach_batch.argtypes


def test_planner_has_mixed_methods():
    assert callable(getattr(A.Planner, "plan_mixed", None))
    assert callable(getattr(A.Planner, "reach_mixed", None))


def test_mixed_counts_marshalling():
    counts = [3, 0, 5, 5, 1, 0, 2]
    worlds = [A.make_world(40 + s, n) for s, n in enumerate(counts)]
    holder = types.SimpleNamespace()   # owns the obstacle block, as a Planner does (self._keep)
    arr = A.Planner._worlds(holder, worlds)
    assert ctypes.sizeof(arr) == len(worlds) * ctypes.sizeof(A.World)
    seen = set()
    for i, (w, n) in enumerate(zip(worlds, counts)):
        a = arr[i]
        assert a.num_obstacles == n, i
        for k, f in enumerate(("q0", "qd0", "qdd0", "q_des")):
            assert np.array_equal(np.array(getattr(a, f)[:]), np.asarray(w[k], dtype=float)), (i, f)
        if n == 0:
            assert not a.obstacles, i              # a world without obstacles: a null pointer
            continue
        got = np.ctypeslib.as_array(a.obstacles, shape=(n * 12,)).reshape(n, 12)
        assert np.array_equal(got, np.asarray(w[4], dtype=float).reshape(n, 12)), i
        addr = ctypes.addressof(a.obstacles.contents)
        assert addr not in seen, i                 # its own block, also for the two worlds of 5
        seen.add(addr)
