"""The bundle-engine runs behind tests/golden/lane_parent_*.npy: the cases, what is read back from a
planner after a reach, and how it is reduced to digests. Shared by tools/record_lane_parent.py (which
recorded the fixtures on the commit before cross_const became one compacting pass) and
tests/test_gpu_lane_onepass.py (which runs the same on the current build).

Cases, all T = 100, O = 20, survey worlds, ARMOUR_ENGINE=lane:
  a      1 world: 2 bundles, the second with 36 live lanes
  b      3 worlds: 5 bundles (two hold jobs of two worlds, the last has 44 live lanes)
  fetch  1 world on the Fetch tables (8 links; other operand sizes and CROSS_C counts)

What the C ABI hands out after a reach is what is recorded. The link k-monomial hashes and
coefficients and the torque centres, radii and monomials have no getter of their own; the constraint
values and Jacobians at three fixed k evaluate exactly those arrays, and the k-only monomial counts are
read directly, so a change in any of them changes a digest."""
import hashlib
import os

import numpy as np

import armour_amd as A
from armour_amd import robot_tables as RT

T, O = 100, 20
SHAPES = ("wide", "dense")
CASES = ("a", "b", "fetch")
ITEMS = ("link_generators", "torque_radius", "link_counts", "torque_counts", "g_x0", "J_x0", "g_x1", "J_x1",
         "g_x2", "J_x2", "k_opt", "iterations", "link_centers", "constraints", "dump_lane0", "dump_lane63")
# the third k is neither symmetric nor evenly spaced, so changes that cancel at the first two show
XS = (np.zeros(7), np.linspace(-0.7, 0.7, 7), np.array([0.31, -0.52, 0.77, -0.13, 0.64, -0.9, 0.05]))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PATHS = {}  # (case, shape) -> the planner's path census when run_case closed it


class env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.prev = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *exc):
        for k, v in self.prev.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def case_setup(case):
    """(robot tables or None, worlds)"""
    if case == "fetch":
        robot = RT.load_json(os.path.join(GOLDEN, "robot_fetch.json"))
        return robot, [A.make_world(5200, O, robot=RT.geometry(robot), profile="survey")]
    n = 1 if case == "a" else 3
    return None, [A.make_world(5100 + s, O, profile="survey") for s in range(n)]


def planner(case, shape, dump=True, hcap=None, ccap=None):
    robot, worlds = case_setup(case)
    with env(ARMOUR_ENGINE="lane", ARMOUR_LANE_SHAPE=shape, ARMOUR_DUMP_OPS="1" if dump else None,
             ARMOUR_LANE_HCAP=hcap, ARMOUR_LANE_CCAP=ccap):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=len(worlds), robot=robot)
    return P, worlds


def reach_outputs(P, worlds, dump=True):
    """{item: array} of everything read back after P.reach(worlds) and, for the link centres and
    constraints at the optimum, after P.plan(worlds); worlds concatenated; and reach_bytes"""
    tm = P.reach(worlds)
    out = {k: [] for k in ITEMS if not k.startswith("dump")}
    for w in range(len(worlds)):
        out["link_generators"].append(P.link_generators(w))
        out["torque_radius"].append(P.torque_radius(w))
        lk, tq = P.monomial_counts(w)
        out["link_counts"].append(lk)
        out["torque_counts"].append(tq)
        for k, x in enumerate(XS):
            g, J = P.eval_constraints(w, x)
            out[f"g_x{k}"].append(g)
            out[f"J_x{k}"].append(J)
    res, _ = P.plan(worlds)
    for w, r in enumerate(res):
        out["k_opt"].append(r["k_opt"])
        out["iterations"].append(np.array([r["iterations"], r["error"]], dtype=np.int64))
        out["link_centers"].append(P.link_centers(w))
        out["constraints"].append(P.constraints(w))
    out = {k: np.ascontiguousarray(np.concatenate([np.asarray(v).reshape(-1) for v in vs])) for k, vs in out.items()}
    if dump:
        for lane in (0, 63):
            with env(ARMOUR_DUMP_LANE=lane):
                out[f"dump_lane{lane}"] = P.reach_dump()
    return out, float(tm["reach_bytes"])


def digest(a):
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def digests(out):
    return np.stack([digest(out[k]) for k in ITEMS])


def run_case(case, shape):
    """(digests [len(ITEMS), 32] uint8, dump of lane 0 [nops, 8], reach_bytes, {item: array})"""
    P, worlds = planner(case, shape)
    out, nbytes = reach_outputs(P, worlds)
    PATHS[case, shape] = P.path_counts()
    P.close()
    return digests(out), out["dump_lane0"], nbytes, out
