"""tests/golden/solver_config.npz (tests/make_solver_config.py) without a device: the oracle reproduces
the frozen plans of the optional solver configurations, the sets meet the conditions the GPU tests'
bars lean on, and the C ABI carries the options and their three path counters."""
import os
import re

import numpy as np
import pytest

import armour_amd as A
import make_solver_config as M
from test_abi import HEADER, exported, lib_path  # noqa: F401  (lib_path: the fixture that builds the library)

GPU_WORLDS = {"survey_T20_O8": 48}  # worlds of a set the GPU cases plan (default: all)


@pytest.fixture(scope="module")
def fx():
    return dict(np.load(M.OUT))


@pytest.mark.parametrize("name", list(M.CONFIGS))
def test_oracle_reproduces_the_fixture(fx, name):
    """the clean plan of every world under every configuration of the set, and the inputs' SHA-1"""
    T, _, worlds, armtd = M.set_worlds(name)
    assert [M.world_sha1(w) for w in worlds] == list(fx[f"{name}/sha1"])
    for w, world in enumerate(worlds):
        R = M.oracle_of(world, T, armtd, threads=4)
        for cfg in M.CONFIGS[name]:
            mu, flags = M.flags_of(cfg)
            r = R.plan(mu_strategy=mu, flags=flags)
            pre = f"{name}/{M.key(cfg)}/"
            for k in ("status", "feasible", "iterations", "evaluations", "restart_iter"):
                assert int(r[k]) == int(fx[pre + k][w]), (cfg, w, k)
            assert np.array_equal(r["k_opt"], fx[pre + "k_opt"][w]) and r["cost"] == fx[pre + "cost"][w], (cfg, w)


def test_sets_meet_the_conditions_the_bars_lean_on(fx):
    restarts = {("boundary_small_T20_O6", (1, 16, 6)): {1: 1, 8: 4, 9: 1}, ("boundary_small_T20_O6", (2, 8, 6)): {8: 4},
                ("armtd_T100_O10", M.REFERENCE): {2: 7}, ("boundary_small_T20_O6", M.REFERENCE): {},
                ("boundary_small_T20_O6", (3, 16, 0)): {}, ("survey_T20_O8", M.REFERENCE): {}}
    for name, cfgs in M.CONFIGS.items():
        for cfg in cfgs:
            pre = f"{name}/{M.key(cfg)}/"
            n = GPU_WORLDS.get(name, len(fx[pre + "status"]))
            st, feas = fx[pre + "status"], fx[pre + "feasible"].astype(bool)
            # no status or feasibility verdict moves under noise: they are compared exactly on the GPU
            assert not fx[pre + "dst_noise"].any(), (name, cfg)
            # loose worlds (k_opt tolerance above 1e-6, or an iteration count that moves under noise, on a
            # converged or feasible plan) are at most a tenth of what the GPU case plans
            plan = (st[:n] == 0) | feas[:n]
            loose = plan & ((10.0 * fx[pre + "dk_noise"][:n] > 1e-6) | (fx[pre + "dit_noise"][:n] > 0))
            print(name, cfg, "loose worlds", np.flatnonzero(loose).tolist(), "of", n)
            assert 10 * int(loose.sum()) <= n, (name, cfg, np.flatnonzero(loose))
            assert {w: int(r) for w, r in enumerate(fx[pre + "restart_iter"]) if r >= 0} == restarts[name, cfg], (name, cfg)
            assert (st == 0).any() and (st == 4).any(), (name, cfg)
            if name.startswith("survey"):
                assert 0.25 <= np.mean(~feas) <= 0.5, (name, cfg, np.mean(~feas))  # (seeds 0 .. 63: 32 of 64)


def test_options_in_the_abi(lib_path):  # noqa: F811
    """the two entries are exported, bound and documented; the path counters' names are unique and end in the
    three new ones, so that every earlier index keeps its meaning"""
    L = A.lib()
    header = open(HEADER).read()
    for sym in ("armour_get_solver_options", "armour_set_solver_options"):
        assert sym in exported(lib_path) and sym in A.ABI_SYMBOLS and hasattr(L, sym)
        assert re.search(r"\*/\s*typedef struct armour_solver_options \{.*?\} armour_solver_options;\s*int armour_get_solver_options", header, flags=re.S)
    doc = re.search(r"/\* The interior-point solver's configuration.*?\*/", header, flags=re.S).group(0)
    for word in ("armour_set_solver_options", "ARMOUR_E_ARG", "ARMOUR_E_STATE", "ARMOUR_MU_STRATEGY", "ARMOUR_QF_GRID", "ARMOUR_LBFGS"):
        assert word in doc, word
    count = int(re.search(r"#define\s+ARMOUR_PATH_COUNT\s+(\d+)", header).group(1))
    names = [L.armour_path_name(i).decode() for i in range(count)]
    assert len(set(names)) == count
    assert names[-3:] == ["solve_quality", "qf_sigma", "hess_lbfgs"]
    assert names.index("solve_adaptive") < count - 3 and names[count - 4] == "track_serial_episode"
    import ctypes
    assert ctypes.sizeof(A.SolverOptions) == 12
    o = A.SolverOptions()
    assert L.armour_get_solver_options(None, ctypes.byref(o)) == A.ARMOUR_E_ARG
    assert L.armour_set_solver_options(None, ctypes.byref(o)) == A.ARMOUR_E_ARG
    for f in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        text = open(os.path.join(os.path.dirname(HEADER), "..", f)).read()
        assert "ARMOUR_QF_GRID" in text or f != "INTEGRATION.md", f
        assert "armour_set_solver_options" in text or "set_solver_options" in text, f
