"""The input domain check (include/armour_hip.h armour_check_world / armour_check_armtd_world), through
ctypes, no device: values that are not finite or angles beyond ARMOUR_MAX_ABS_ANGLE are refused with
ARMOUR_E_ARG and a message that names the field; everything inside the domain is accepted, every edge
case of tests/domain_edges.py included. The planning entries run this check before they copy or
launch anything (planner.hip upload_worlds, upload_armtd), and armour_main reports a refused world as a failed
replan."""
import os
import re
import subprocess

import numpy as np
import pytest

import armour_amd as A
import domain_edges as DE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "armour_hip.h")
BAD = [np.nan, np.inf, -np.inf, 1e17, -1e17]
FIELDS = ("q0", "qd0", "qdd0", "q_des")


def max_abs_angle():
    m = re.search(r"#define\s+ARMOUR_MAX_ABS_ANGLE\s+(\S+)", open(HEADER).read())
    return float(m.group(1))


def _mutated(k, i, v):
    w = [np.array(a, dtype=np.float64) for a in DE.base_world()]
    w[k][i] = v
    return tuple(w)


def test_constant_bounds_the_wrap_loop():
    """the continuous joints' bounds (+-1000) lie inside the domain, and the wrapped difference of two
    angles inside it takes fewer turns than wrap_to_pi allows (nlp_kernels.hip WRAP_MAX_TURNS)"""
    m = max_abs_angle()
    assert 1000 < m <= 1e4
    src = open(os.path.join(ROOT, "armour-dev_amd", "csrc", "nlp_kernels.hip")).read()
    turns = int(re.search(r"WRAP_MAX_TURNS\s*=\s*(\d+)", src).group(1))
    assert 2 * m / (2 * np.pi) < turns


@pytest.mark.parametrize("k", range(4), ids=FIELDS)
def test_bad_values_refused_with_the_field_named(k):
    over = np.nextafter(max_abs_angle(), np.inf)
    for i in (0, 1, 6):
        for v in BAD + ([over, -over] if FIELDS[k] in ("q0", "q_des") else []):
            # a finite rate is inside the domain whatever its size: only the angles carry the bound
            if FIELDS[k] in ("qd0", "qdd0") and np.isfinite(v):
                assert A.check_world(_mutated(k, i, v)) is None
                continue
            msg = A.check_world(_mutated(k, i, v))
            assert msg is not None and f"{FIELDS[k]}[{i}]" in msg, (FIELDS[k], i, v, msg)


def test_bad_obstacle_values_and_counts_refused():
    for idx in (0, 11, 35):
        for v in (np.nan, np.inf, -np.inf):
            w = [np.array(a, dtype=np.float64) for a in DE.base_world()]
            w[4].reshape(-1)[idx] = v
            msg = A.check_world(tuple(w))
            assert msg is not None and f"obstacles[{idx}]" in msg, msg
    assert "num_obstacles" in A.check_world(DE.base_world(), max_obstacles=2)
    assert A.check_world(DE.base_world(), max_obstacles=3) is None
    L = A.lib()
    assert L.armour_check_world(None, 3) == A.ARMOUR_E_ARG
    w = A.World()
    w.num_obstacles = -1
    assert L.armour_check_world(w, 3) == A.ARMOUR_E_ARG and b"num_obstacles" in L.armour_last_error()
    w.num_obstacles = 2   # a positive count with a null pointer
    assert L.armour_check_world(w, 3) == A.ARMOUR_E_ARG and b"obstacles" in L.armour_last_error()


def test_values_inside_the_domain_accepted():
    m = max_abs_angle()
    for k in (0, 3):
        for v in (m, -m, np.nextafter(m, 0), 1000.0, -999.9):
            assert A.check_world(_mutated(k, 2, v)) is None, (FIELDS[k], v)
    for k in (1, 2):
        assert A.check_world(_mutated(k, 0, 1e17)) is None


def test_every_domain_edge_case_accepted():
    cases = DE.all_cases()
    assert len(cases) == 58
    for name, world in cases:
        assert A.check_world(world, max_obstacles=DE.O) is None, name


def _armtd_world(T=10):
    b = DE.base_world()
    tab = np.zeros((7, 6, T))
    tab[:, 0] = 1.0
    return [b[0].copy(), b[1].copy(), b[3].copy(), tab, np.full(7, np.pi / 72), b[4].copy()]


def test_armtd_world_check():
    T = 10
    assert A.check_armtd_world(_armtd_world(T), T, DE.O) is None
    over = np.nextafter(max_abs_angle(), np.inf)
    for k, name, vals in ((0, "q0", BAD + [over]), (1, "qd0", BAD[:3]), (2, "q_des", BAD + [-over]),
                          (4, "k_range", BAD[:3])):
        for v in vals:
            w = _armtd_world(T)
            w[k][3] = v
            msg = A.check_armtd_world(w, T, DE.O)
            assert msg is not None and f"{name}[3]" in msg, (name, v, msg)
    for idx in (0, 7 * 6 * T - 1):
        w = _armtd_world(T)
        w[3].reshape(-1)[idx] = np.nan
        msg = A.check_armtd_world(w, T, DE.O)
        assert msg is not None and f"jrs_tables[{idx}]" in msg, msg
    w = _armtd_world(T)
    w[5][1, 4] = np.inf
    assert "obstacles[16]" in A.check_armtd_world(w, T, DE.O)
    assert "num_obstacles" in A.check_armtd_world(_armtd_world(T), T, 2)


def _write_input(d, world):
    q0, qd0, qdd0, q_des, obs = world
    with open(os.path.join(d, "armour.in"), "w") as f:
        for v in (q0, qd0, qdd0, q_des):
            f.write(" ".join(repr(float(x)) for x in v) + "\n")
        f.write(f"{len(obs)}\n")
        for o in obs:
            f.write(" ".join(repr(float(x)) for x in o) + "\n")


def test_armour_main_reports_a_world_outside_the_domain_as_a_failed_replan(tmp_path):
    """-1 in armour.out, a non-zero status and the field on stderr. The check sits in plan_dir, which
    the in-process and the served path share, before a planner is created: no device is needed."""
    exe = os.path.join(ROOT, "armour-dev_amd", "armour_amd", "armour_main")
    _write_input(str(tmp_path), _mutated(3, 0, 1e17))
    env = dict(os.environ, ARMOUR_NUM_TIME_STEPS="10", ARMOUR_NO_SERVE="1")
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0
    assert (tmp_path / "armour.out").read_text().split() == ["-1"]
    assert "q_des[0]" in r.stderr, r.stderr
