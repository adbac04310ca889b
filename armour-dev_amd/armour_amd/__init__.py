"""armour_amd — Python binding of the MI355X-native ARMOUR planner (libarmour_hip.so).

The product is the C ABI in include/armour_hip.h; this module is a thin ctypes layer over it,
used by tests/, bench.py and __graft_entry__.py. It loads the in-tree library and raises if the
library or a GPU is missing — there is no CPU fallback.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from .robots import KINOVA
from .worlds import csv_world, example_world, make_world, straight_line_waypoint

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("ARMOUR_LIB") or os.path.join(_HERE, "libarmour_hip.so")  # ARMOUR_LIB: diagnostics builds
NF = 7
_LIB = None
_dp = ctypes.POINTER(ctypes.c_double)


ARMOUR_E_ARG, ARMOUR_E_HIP, ARMOUR_E_CAPACITY, ARMOUR_E_STATE, ARMOUR_E_INTERNAL = -1, -2, -3, -4, -5  # include/armour_hip.h


class ArmourError(RuntimeError):
    pass


class Config(ctypes.Structure):
    _fields_ = [("robot", ctypes.c_int), ("num_time_steps", ctypes.c_int), ("max_obstacles", ctypes.c_int),
                ("max_worlds", ctypes.c_int), ("device", ctypes.c_int), ("max_iter", ctypes.c_int)]


class SolverOptions(ctypes.Structure):  # armour_solver_options
    _fields_ = [("mu_strategy", ctypes.c_int), ("qf_grid", ctypes.c_int), ("lbfgs_history", ctypes.c_int)]


class World(ctypes.Structure):
    _fields_ = [("q0", ctypes.c_double * NF), ("qd0", ctypes.c_double * NF), ("qdd0", ctypes.c_double * NF),
                ("q_des", ctypes.c_double * NF), ("num_obstacles", ctypes.c_int), ("obstacles", _dp)]


_WORLD_DTYPE = np.dtype({"names": ["q0", "qd0", "qdd0", "q_des", "num_obstacles", "obstacles"],
                         "formats": [(np.float64, NF)] * 4 + [np.int32, np.uintp],
                         "offsets": [World.q0.offset, World.qd0.offset, World.qdd0.offset, World.q_des.offset,
                                     World.num_obstacles.offset, World.obstacles.offset],
                         "itemsize": ctypes.sizeof(World)})


class ArmtdWorld(ctypes.Structure):
    _fields_ = [("q0", ctypes.c_double * NF), ("qd0", ctypes.c_double * NF), ("q_des", ctypes.c_double * NF),
                ("jrs_tables", _dp), ("k_range", ctypes.c_double * NF), ("num_obstacles", ctypes.c_int),
                ("obstacles", _dp)]


class Result(ctypes.Structure):
    _fields_ = [("k_opt", ctypes.c_double * NF), ("feasible", ctypes.c_int), ("solver_status", ctypes.c_int),
                ("iterations", ctypes.c_int), ("evaluations", ctypes.c_int), ("cost", ctypes.c_double),
                ("kkt_error", ctypes.c_double), ("error", ctypes.c_int)]


class Timing(ctypes.Structure):
    _fields_ = [("reach_ms", ctypes.c_double), ("nlp_ms", ctypes.c_double), ("total_ms", ctypes.c_double),
                ("reach_kernel_ms", ctypes.c_double), ("reach_bytes", ctypes.c_double)]

    def as_dict(self):
        return {name: getattr(self, name) for name, _ in self._fields_}


class EpisodeConfig(ctypes.Structure):
    """armour_episode_config (include/armour_hip.h)"""
    _fields_ = [("lookahead", ctypes.c_double), ("goal_radius", ctypes.c_double), ("check_samples", ctypes.c_int)]


class EpisodeState(ctypes.Structure):
    """armour_episode_state (include/armour_hip.h)"""
    _fields_ = [("q", ctypes.c_double * NF), ("qd", ctypes.c_double * NF), ("qdd", ctypes.c_double * NF),
                ("q_des", ctypes.c_double * NF), ("status", ctypes.c_int), ("mode", ctypes.c_int),
                ("steps", ctypes.c_int), ("failed_plans", ctypes.c_int), ("failed_streak", ctypes.c_int),
                ("clearance", ctypes.c_double), ("clearance_at", ctypes.c_int * 3), ("goal_distance", ctypes.c_double)]


T_PLAN = 0.5  # ARMOUR_T_PLAN
EPISODE_STATUS = ("running", "goal reached", "collided", "no fail-safe", "left the input domain",
                  "input over the limit", "ultimate bound exceeded", "joint limit exceeded", "rollout not finite")


class TrackOutput(ctypes.Structure):
    """armour_track_output (include/armour_hip.h): the caller's output arrays (null: skipped) and the
    device time of the rollouts"""
    _fields_ = [("max_pos_err", _dp), ("max_vel_err", _dp), ("max_torque", _dp), ("max_V", _dp), ("max_robust", _dp),
                ("end_state", _dp), ("status", ctypes.POINTER(ctypes.c_int)), ("track_ms", ctypes.c_double)]


TRACK_MAX_STEPS = 100000  # ARMOUR_TRACK_MAX_STEPS


class TrackMotionOutput(ctypes.Structure):
    """armour_track_motion_output (include/armour_hip.h): the rollouts' outputs, the true arm's clearance
    per rollout and per world, the flags, and the device time of the check"""
    _fields_ = [("track", TrackOutput), ("clearance", _dp), ("where", ctypes.POINTER(ctypes.c_int)),
                ("flags", ctypes.POINTER(ctypes.c_int)), ("world_clearance", _dp),
                ("world_where", ctypes.POINTER(ctypes.c_int)), ("check_ms", ctypes.c_double)]


class EpisodeTrackConfig(ctypes.Structure):
    """armour_episode_track_config (include/armour_hip.h)"""
    _fields_ = [("num_samples", ctypes.c_int), ("scale", _dp), ("err0", _dp), ("steps", ctypes.c_int),
                ("stop_on_input", ctypes.c_int), ("stop_on_bound", ctypes.c_int), ("stop_on_limit", ctypes.c_int)]


class EpisodeTracked(ctypes.Structure):
    """armour_episode_tracked (include/armour_hip.h): a world's record of its true arms"""
    _fields_ = [("clearance", ctypes.c_double), ("clearance_at", ctypes.c_int * 4), ("max_pos_err", ctypes.c_double * NF),
                ("max_vel_err", ctypes.c_double * NF), ("max_torque", ctypes.c_double * NF), ("max_V", ctypes.c_double),
                ("max_robust", ctypes.c_double), ("flags", ctypes.c_int), ("flag_step", ctypes.c_int * 5)]


class RoadmapConfig(ctypes.Structure):
    """armour_roadmap_config (include/armour_hip.h)"""
    _fields_ = [("num_nodes", ctypes.c_int), ("connect_radius", ctypes.c_double), ("edge_step", ctypes.c_double),
                ("margin", ctypes.c_double)]


class RoadmapStats(ctypes.Structure):
    """armour_roadmap_stats (include/armour_hip.h)"""
    _fields_ = [("free_nodes", ctypes.c_longlong), ("candidate_edges", ctypes.c_longlong), ("edges", ctypes.c_longlong),
                ("edge_samples", ctypes.c_longlong), ("reachable", ctypes.c_longlong), ("relax_rounds_max", ctypes.c_int),
                ("build_ms", ctypes.c_double * 4)]


ROADMAP_MAX_NODES = 1023      # ARMOUR_ROADMAP_MAX_NODES
ROADMAP_MIN_EDGE = 1e-6       # ARMOUR_ROADMAP_MIN_EDGE


# ARMOUR_TRACK_COLLISION .. ARMOUR_TRACK_NOT_FINITE: the bits of armour_track_motion's flags
TRACK_COLLISION, TRACK_INPUT, TRACK_BOUND, TRACK_LIMIT, TRACK_NOT_FINITE = 1, 2, 4, 8, 16


class PlanOutput(ctypes.Structure):
    """armour_plan_output (include/armour_hip.h): the single-world entry's result and the caller's
    output arrays (null: skipped)"""
    _fields_ = [("result", Result), ("timing", Timing), ("constraints", _dp), ("joint_bounds", _dp),
                ("link_centers", _dp), ("link_generators", _dp), ("torque_radius", _dp)]


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise ArmourError(f"HIP planner library not built: {LIB_PATH} (run __graft_entry__.build())")
        L = ctypes.CDLL(LIB_PATH)
        L.armour_create.restype = ctypes.c_void_p
        L.armour_create.argtypes = [ctypes.POINTER(Config)]
        L.armour_create_robot.restype = ctypes.c_void_p
        L.armour_create_robot.argtypes = [ctypes.POINTER(Config), ctypes.c_void_p]
        L.armour_robot_builtin.argtypes = [ctypes.c_int, ctypes.c_void_p]
        L.armour_device_compute_units.argtypes = [ctypes.c_int]
        L.armour_copy_bandwidth.restype = ctypes.c_double
        L.armour_copy_bandwidth.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_int]
        L.armour_destroy.argtypes = [ctypes.c_void_p]
        L.armour_last_error.restype = ctypes.c_char_p
        L.armour_num_constraints.argtypes = [ctypes.c_void_p, ctypes.c_int]
        L.armour_num_joints.argtypes = [ctypes.c_void_p]
        L.armour_create_armtd.restype = ctypes.c_void_p
        L.armour_create_armtd.argtypes = [ctypes.POINTER(Config)]
        L.armour_plan_armtd_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ArmtdWorld),
                                              ctypes.POINTER(Result), ctypes.POINTER(Timing)]
        L.armour_reach_armtd_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ArmtdWorld),
                                               ctypes.POINTER(Timing)]
        L.armour_plan_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(World), ctypes.POINTER(Result),
                                        ctypes.POINTER(Timing)]
        L.armour_reach_batch.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(World), ctypes.POINTER(Timing)]
        # (bound where present: an A/B against an older build through ARMOUR_LIB still loads; using a
        # mixed entry on such a build raises)
        for name, args in (("armour_plan_batch_mixed", L.armour_plan_batch.argtypes),
                           ("armour_reach_batch_mixed", L.armour_reach_batch.argtypes),
                           ("armour_world_num_obstacles", [ctypes.c_void_p, ctypes.c_int]),
                           ("armour_eval_candidates", [ctypes.c_void_p, ctypes.c_int, _dp, _dp, _dp,
                                                       ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)])):
            if hasattr(L, name):
                getattr(L, name).argtypes = args
        ip = ctypes.POINTER(ctypes.c_int)
        for name, args in (("armour_check_motion", [ctypes.c_void_p, _dp, ctypes.c_double, ctypes.c_double, ctypes.c_int,
                                                    _dp, ip]),
                           ("armour_episode_begin", [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(World), _dp,
                                                     ctypes.POINTER(EpisodeConfig)]),
                           ("armour_episode_step", [ctypes.c_void_p, ip, ctypes.POINTER(Result), ctypes.POINTER(Timing),
                                                    _dp]),
                           ("armour_episode_get", [ctypes.c_void_p, ctypes.POINTER(EpisodeState)]),
                           ("armour_track", [ctypes.c_void_p, ctypes.c_int, _dp, ctypes.c_int, _dp, _dp, ctypes.c_double,
                                             ctypes.c_double, ctypes.c_int, ctypes.POINTER(TrackOutput)]),
                           ("armour_track_motion", [ctypes.c_void_p, _dp, ctypes.c_int, _dp, _dp, ctypes.c_double,
                                                    ctypes.c_double, ctypes.c_int, ctypes.c_int,
                                                    ctypes.POINTER(TrackMotionOutput)]),
                           ("armour_episode_track", [ctypes.c_void_p, ctypes.POINTER(EpisodeTrackConfig)]),
                           ("armour_episode_get_tracked", [ctypes.c_void_p, ctypes.POINTER(EpisodeTracked), _dp, ip, _dp]),
                           ("armour_roadmap_build", [ctypes.c_void_p, ctypes.POINTER(RoadmapConfig), _dp, _dp,
                                                     ctypes.POINTER(RoadmapStats)]),
                           ("armour_roadmap_get", [ctypes.c_void_p, ctypes.c_int, _dp, ip, ctypes.POINTER(ctypes.c_uint), _dp,
                                                   ip]),
                           ("armour_roadmap_waypoint", [ctypes.c_void_p, _dp, ctypes.c_double, _dp, ip, _dp]),
                           ("armour_episode_roadmap", [ctypes.c_void_p, ctypes.POINTER(RoadmapConfig), _dp]),
                           ("armour_episode_get_roadmap", [ctypes.c_void_p, ip, _dp])):
            if hasattr(L, name):
                getattr(L, name).argtypes = args
        for name, args in (("armour_check_world", [ctypes.POINTER(World), ctypes.c_int]),
                           ("armour_check_armtd_world", [ctypes.POINTER(ArmtdWorld), ctypes.c_int, ctypes.c_int])):
            if hasattr(L, name):
                getattr(L, name).argtypes = args
        L.armour_plan.argtypes = [ctypes.c_void_p, ctypes.POINTER(World), ctypes.POINTER(PlanOutput)]
        L.armour_eval_constraints.argtypes = [ctypes.c_void_p, ctypes.c_int, _dp, _dp, _dp]
        L.armour_get_reach_program.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int), ctypes.c_int]
        L.armour_get_monomial_counts.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                                 ctypes.POINTER(ctypes.c_int)]
        L.armour_get_reach_occupancy.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong),
                                                 ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
        L.armour_get_joint_bounds.argtypes = [ctypes.c_void_p, _dp]
        L.armour_get_plane_cache_stats.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
        L.armour_get_reach_span.argtypes = [ctypes.c_void_p, _dp]
        if hasattr(L, "armour_get_path_counts"):  # absent from older libraries loaded through ARMOUR_LIB
            L.armour_get_path_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_longlong), ctypes.c_int]
            L.armour_path_name.restype = ctypes.c_char_p
            L.armour_path_name.argtypes = [ctypes.c_int]
        if hasattr(L, "armour_set_solver_options"):  # absent from older libraries loaded through ARMOUR_LIB
            L.armour_get_solver_options.argtypes = [ctypes.c_void_p, ctypes.POINTER(SolverOptions)]
            L.armour_set_solver_options.argtypes = [ctypes.c_void_p, ctypes.POINTER(SolverOptions)]
        L.armour_get_reach_dump.argtypes = [ctypes.c_void_p, _dp, ctypes.c_int]
        L.armour_get_reach_profile.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_ulonglong), ctypes.c_int]
        for name in ("armour_get_constraints", "armour_get_link_centers", "armour_get_link_generators",
                     "armour_get_torque_radius"):
            getattr(L, name).argtypes = [ctypes.c_void_p, ctypes.c_int, _dp]
        if hasattr(L, "armour_sq_selfcheck"):  # absent from older libraries loaded through ARMOUR_LIB
            L.armour_sq_selfcheck.argtypes = [ctypes.c_int, ctypes.c_double, ctypes.c_longlong, _dp, ctypes.c_longlong,
                                              _dp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_longlong)]
        _LIB = L
    return _LIB


# every symbol include/armour_hip.h declares (checked by tests/test_abi.py)
ABI_SYMBOLS = ["armour_copy_bandwidth", "armour_create", "armour_create_robot", "armour_robot_builtin", "armour_device_compute_units", "armour_destroy", "armour_last_error", "armour_num_constraints",
               "armour_plan_batch", "armour_reach_batch", "armour_eval_constraints", "armour_get_constraints",
               "armour_get_link_centers", "armour_get_link_generators", "armour_get_torque_radius",
               "armour_num_joints", "armour_get_joint_bounds", "armour_get_reach_program", "armour_get_reach_profile",
               "armour_get_reach_dump", "armour_get_reach_occupancy", "armour_get_monomial_counts",
               "armour_create_armtd", "armour_plan_armtd_batch", "armour_reach_armtd_batch",
               "armour_get_plane_cache_stats", "armour_plan", "armour_get_reach_span",
               "armour_plan_batch_mixed", "armour_reach_batch_mixed", "armour_world_num_obstacles",
               "armour_eval_candidates", "armour_sq_selfcheck", "armour_check_world", "armour_check_armtd_world",
               "armour_check_motion", "armour_episode_begin", "armour_episode_step", "armour_episode_get",
               "armour_track", "armour_track_motion", "armour_episode_track", "armour_episode_get_tracked",
               "armour_roadmap_build", "armour_roadmap_get", "armour_roadmap_waypoint", "armour_episode_roadmap",
               "armour_episode_get_roadmap",
               "armour_get_path_counts", "armour_path_name", "armour_get_solver_options", "armour_set_solver_options"]


def default_batch(T: int, device: int = 0, waves: int = 2) -> int:
    """worlds per step that fill `waves` whole bundle waves of the device (lane_kernel.hip runs one
    64-job bundle per CU at a time): floor(waves * CUs * 64 / T)"""
    n = lib().armour_device_compute_units(device)
    _check(min(0, n))
    return max(1, (waves * n * 64) // T)


def copy_bandwidth(device: int = 0, nbytes: int = 2 << 30, reps: int = 10) -> float:
    """device-to-device copy bandwidth in GB/s (read + write bytes / time) of a 16 B-per-lane
    streaming copy kernel (armour_copy_bandwidth): the achievable HBM figure for roofline fractions"""
    v = lib().armour_copy_bandwidth(device, nbytes, reps)
    if v < 0:
        raise ArmourError(f"armour_copy_bandwidth: {lib().armour_last_error().decode()}")
    return v


def sq_selfcheck(thr: float, half_width: int, values=None, device: int = 0):
    """(S*, valid, mismatches) of armour_sq_selfcheck: the squared form S* of the keep / prune threshold
    thr as the device finds it, whether the device verified it, and how often sqrt(S) against thr and S
    against S* decide differently over the doubles within half_width ulps of S* and over `values`"""
    v = np.ascontiguousarray(values if values is not None else np.zeros(0), dtype=np.float64)
    s, ok, bad = ctypes.c_double(0), ctypes.c_int(0), ctypes.c_longlong(0)
    _check(lib().armour_sq_selfcheck(device, float(thr), int(half_width), _ptr(v) if v.size else None, v.size,
                                     ctypes.byref(s), ctypes.byref(ok), ctypes.byref(bad)))
    return s.value, bool(ok.value), int(bad.value)


def check_world(world, max_obstacles=40):
    """armour_check_world on (q0, qd0, qdd0, q_des, obstacles[O, 12]): None when the world lies inside
    the input domain (include/armour_hip.h), else the library's message, which names the field. Runs
    on the host; no device is touched."""
    w = World()
    for k, f in enumerate(("q0", "qd0", "qdd0", "q_des")):
        getattr(w, f)[:] = [float(v) for v in world[k]]
    obs = np.ascontiguousarray(np.asarray(world[4], dtype=np.float64).reshape(-1, 12))
    w.num_obstacles = obs.shape[0]
    w.obstacles = _ptr(obs) if obs.shape[0] else None
    rc = lib().armour_check_world(ctypes.byref(w), int(max_obstacles))
    return None if rc == 0 else lib().armour_last_error().decode()


def check_armtd_world(world, T, max_obstacles=40):
    """armour_check_armtd_world on (q0, qd0, q_des, jrs_tables[7, 6, T], k_range, obstacles[O, 12])"""
    q0, qd0, q_des, tab, kr, obs = world
    a = ArmtdWorld()
    a.q0[:] = [float(v) for v in q0]
    a.qd0[:] = [float(v) for v in qd0]
    a.q_des[:] = [float(v) for v in q_des]
    a.k_range[:] = [float(v) for v in kr]
    t = np.ascontiguousarray(np.asarray(tab, dtype=np.float64).reshape(NF, 6, T))
    o = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1, 12))
    a.jrs_tables = _ptr(t)
    a.num_obstacles = o.shape[0]
    a.obstacles = _ptr(o) if o.shape[0] else None
    rc = lib().armour_check_armtd_world(ctypes.byref(a), int(max_obstacles), int(T))
    return None if rc == 0 else lib().armour_last_error().decode()


def _check(rc):
    if rc != 0:
        raise ArmourError(f"armour error {rc}: {lib().armour_last_error().decode()}")


def _ptr(a):
    return a.ctypes.data_as(_dp) if a is not None else None


def _iptr(a):
    """as _ptr, for an int32 array"""
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int)) if a is not None else None


def _records(cls, recs):
    """a list of ctypes records of class `cls` as a dict of arrays over the records: float64 for the
    floating-point fields, int64 for the integer ones; an array field of length n gives [len(recs), n]"""
    out = {}
    for k, ctype in cls._fields_:
        n = getattr(ctype, "_length_", None)
        base = ctype._type_ if n is not None else ctype
        vals = [getattr(r, k)[:] if n is not None else getattr(r, k) for r in recs]
        a = np.array(vals, dtype=np.float64 if base is ctypes.c_double else np.int64)
        out[k] = a.reshape(len(recs), n) if n is not None else a
    return out


def candidates_array(x, W):
    """the [W, N, 7] array Planner.eval_candidates hands to the library, from x of that shape or
    [N, 7] (the same candidates for each of the W worlds); ValueError for a wrong shape, a non-finite
    value or one outside [-1, 1] (the box the collision planes are certified for)"""
    x = np.asarray(x, dtype=np.float64)
    if x.ndim == 2 and x.shape[1] == NF and x.shape[0] >= 1:
        if W < 1:
            raise ValueError("eval_candidates: x of shape [N, 7] needs a batch (reach or plan first)")
        x = np.broadcast_to(x, (W,) + x.shape)
    if x.ndim != 3 or x.shape[2] != NF or x.shape[0] < 1 or x.shape[1] < 1 or (W >= 1 and x.shape[0] != W):
        raise ValueError(f"eval_candidates: x must have shape [W, N, {NF}] or [N, {NF}] (W = {W}), got {x.shape}")
    if not np.all(np.isfinite(x)):
        raise ValueError("eval_candidates: x holds a non-finite value")
    if np.abs(x).max() > 1.0:
        raise ValueError("eval_candidates: every candidate must lie in [-1, 1]")
    return np.ascontiguousarray(x)


def uncertainty_samples(tables, S, seed=0):
    """[S, 2, num_joints] mass and inertia scales for armour_track within the tables' stated uncertainty
    d = (mass_uncertainty, inertia_uncertainty): sample 0 nominal, sample 1 every link at 1 + d, sample 2
    every link at 1 - d, the rest uniform in [1 - d, 1 + d] per link (numpy default_rng(seed))"""
    S = int(S)
    if S < 1:
        raise ValueError("uncertainty_samples: S must be at least 1")
    nj = int(tables["num_joints"])
    d = np.array([float(tables["mass_uncertainty"]), float(tables["inertia_uncertainty"])])[None, :, None]
    u = np.random.default_rng(seed).uniform(-1.0, 1.0, (S, 2, nj))
    u[0] = 0.0
    if S > 1:
        u[1] = 1.0
    if S > 2:
        u[2] = -1.0
    return 1.0 + d * u


class Planner:
    """Batched MI355X planner. A world is (q0, qd0, qdd0, q_des, obstacles[O, 12]). plan / reach take
    worlds that all carry the same O; plan_mixed / reach_mixed take any mix of counts."""

    def __init__(self, T=100, max_obstacles=20, max_worlds=1, device=0, max_iter=0, robot=None, _armtd=False, solver=None):
        """robot: None (built-in Kinova Gen3 tables) or a robot-table dict (armour_amd.robot_tables);
        solver: None or a dict of solver options (set_solver_options)"""
        cfg = Config(0, T, max_obstacles, max_worlds, device, max_iter)
        if _armtd:
            self.h = lib().armour_create_armtd(ctypes.byref(cfg))
        elif robot is None:
            self.h = lib().armour_create(ctypes.byref(cfg))
        else:
            from .robot_tables import to_struct
            self._robot = to_struct(robot)
            self.h = lib().armour_create_robot(ctypes.byref(cfg), ctypes.byref(self._robot))
        if not self.h:
            raise ArmourError(f"armour_create failed: {lib().armour_last_error().decode()}")
        self.T = T
        self.NJ = lib().armour_num_joints(self.h)
        self.max_worlds = max_worlds
        self._keep = []
        self.O = 0
        self._W = 0   # worlds of the last batch handed to the library
        if solver:
            self.set_solver_options(**solver)

    def solver_options(self):
        """armour_get_solver_options: dict(mu_strategy=, qf_grid=, lbfgs_history=)"""
        o = SolverOptions()
        _check(lib().armour_get_solver_options(self.h, ctypes.byref(o)))
        return dict(mu_strategy=o.mu_strategy, qf_grid=o.qf_grid, lbfgs_history=o.lbfgs_history)

    def set_solver_options(self, **options):
        """armour_set_solver_options: the named fields change, the others keep their values; from the
        next plan on. mu_strategy 0 monotone, 1 adaptive (default), 2 Ipopt's quality-function pair (with
        lbfgs_history=6 the reference's configuration), 3 that pair with the default's floor and mu grid;
        qf_grid 2..32 sigma candidates; lbfgs_history 0 (damped full BFGS) or 1..6"""
        cur = self.solver_options()
        unknown = set(options) - set(cur)
        if unknown:
            raise TypeError(f"set_solver_options: unknown option(s) {sorted(unknown)}")
        cur.update({k: int(v) for k, v in options.items()})
        o = SolverOptions(cur["mu_strategy"], cur["qf_grid"], cur["lbfgs_history"])
        _check(lib().armour_set_solver_options(self.h, ctypes.byref(o)))

    def close(self):
        if getattr(self, "h", None) and _LIB is not None:  # (module teardown may have cleared _LIB)
            _LIB.armour_destroy(self.h)
        self.h = None

    def __del__(self):
        self.close()

    def num_constraints(self, O):
        return lib().armour_num_constraints(self.h, O)

    def _worlds(self, worlds):
        # the armour_world array filled through a NumPy view of its fields (one vectorised store
        # per field instead of a ctypes assignment per element); obstacles in one contiguous block
        n = len(worlds)
        arr = (World * n)()
        view = np.frombuffer(arr, dtype=_WORLD_DTYPE)
        for k, f in enumerate(("q0", "qd0", "qdd0", "q_des")):
            view[f] = np.asarray([w[k] for w in worlds], dtype=np.float64).reshape(n, NF)
        obs = [np.asarray(w[4], dtype=np.float64).reshape(-1, 12) for w in worlds]
        counts = np.array([o.shape[0] for o in obs], dtype=np.int64)
        block = np.ascontiguousarray(np.concatenate(obs) if counts.sum() else np.zeros((0, 12)))
        self._keep = [block]
        view["num_obstacles"] = counts
        starts = np.concatenate([[0], np.cumsum(counts)[:-1]]) * 12 * 8
        view["obstacles"] = np.where(counts > 0, block.ctypes.data + starts, 0)
        self.O = int(counts[0]) if n else 0
        self._W = n
        return arr

    def plan_one(self, world):
        """armour_plan (the single-world entry): (result dict, timing dict, outputs dict) with the
        payloads of the five .out files"""
        arr = self._worlds([world])
        m = self.num_constraints(np.asarray(world[4]).reshape(-1, 12).shape[0])
        outs = dict(constraints=np.zeros(m), joint_bounds=np.zeros(28), link_centers=np.zeros((self.T, self.NJ, 3)),
                    link_generators=np.zeros((self.T, self.NJ, 3, 6)), torque_radius=np.zeros((self.T, NF)))
        po = PlanOutput()
        for k, v in outs.items():
            setattr(po, k, v.ctypes.data_as(_dp))
        _check(lib().armour_plan(self.h, arr, ctypes.byref(po)))
        r = po.result
        res = dict(k_opt=np.array(r.k_opt[:]), feasible=bool(r.feasible), status=r.solver_status,
                   iterations=r.iterations, evaluations=r.evaluations, cost=r.cost, kkt=r.kkt_error, error=r.error)
        return res, po.timing.as_dict(), outs

    def plan(self, worlds):
        arr = self._worlds(worlds)
        res = (Result * len(worlds))()
        tm = Timing()
        _check(self._plan_call(self.h, len(worlds), arr, res, ctypes.byref(tm)))
        return self._results(res), self._span(tm.as_dict())

    def _plan_call(self, *a):
        return lib().armour_plan_batch(*a)

    def plan_mixed(self, worlds):
        """armour_plan_batch_mixed: one reach launch and one solve for worlds that carry different
        numbers of obstacles (zero included); results and timing as plan()"""
        arr = self._worlds(worlds)
        res = (Result * len(worlds))()
        tm = Timing()
        _check(lib().armour_plan_batch_mixed(self.h, len(worlds), arr, res, ctypes.byref(tm)))
        return self._results(res), self._span(tm.as_dict())

    def reach_mixed(self, worlds):
        """armour_reach_batch_mixed: the reach-set half of plan_mixed (enables eval_constraints)"""
        arr = self._worlds(worlds)
        tm = Timing()
        _check(lib().armour_reach_batch_mixed(self.h, len(worlds), arr, ctypes.byref(tm)))
        return self._span(tm.as_dict())

    def world_obstacles(self, w):
        """obstacle count of world w of the last batch (armour_world_num_obstacles)"""
        n = lib().armour_world_num_obstacles(self.h, w)
        if n < 0:
            _check(n)
        return n

    @staticmethod
    def _results(res):
        out = []
        for r in res:
            out.append(dict(k_opt=np.array(r.k_opt[:]), feasible=bool(r.feasible), status=r.solver_status,
                            iterations=r.iterations, evaluations=r.evaluations, cost=r.cost, kkt=r.kkt_error,
                            error=r.error))
        return out

    def reach(self, worlds):
        arr = self._worlds(worlds)
        tm = Timing()
        _check(self._reach_call(self.h, len(worlds), arr, ctypes.byref(tm)))
        return self._span(tm.as_dict())

    def _span(self, tm):
        # the reach launch's device-clock execution span (armour_get_reach_span; -1 when unknown)
        v = ctypes.c_double(-1.0)
        rc = lib().armour_get_reach_span(self.h, ctypes.byref(v))
        tm["reach_span_ms"] = v.value if rc == 0 else -1.0
        return tm

    def _reach_call(self, *a):
        return lib().armour_reach_batch(*a)

    def _m(self, w):
        # world w's own constraint count (a mixed batch's worlds differ); an invalid w or a missing
        # batch is left to the call that follows, which reports it
        f = getattr(lib(), "armour_world_num_obstacles", None)
        n = f(self.h, w) if f else -1
        return self.num_constraints(n if n >= 0 else self.O)

    def eval_constraints(self, w, x, jac=True):
        m = self._m(w)
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64))
        g = np.zeros(m)
        J = np.zeros((m, NF)) if jac else None
        _check(lib().armour_eval_constraints(self.h, w, _ptr(x), _ptr(g), _ptr(J)))
        return (g, J) if jac else g

    def eval_candidates(self, x, num_worlds=None):
        """armour_eval_candidates: N candidate parameters per world of the last batch, reduced on the
        device. x: [W, N, 7], or [N, 7] for the same candidates in every world (W worlds: num_worlds,
        default the last reach / plan call's). Returns dict(cost [W, N], violation [W, N, 3] (torque,
        collision, extremum rows), feasible [W, N] bool, best [W] (-1: none)). The plan state, the
        getters and the next plan are untouched. Raises ValueError for a wrong shape, a non-finite
        value or one outside [-1, 1], before the library is called."""
        x = candidates_array(x, self._W if num_worlds is None else int(num_worlds))
        Wx, N = x.shape[:2]
        cost = np.zeros((Wx, N))
        viol = np.zeros((Wx, N, 3))
        feas = np.zeros((Wx, N), dtype=np.int32)
        best = np.zeros(Wx, dtype=np.int32)
        _check(lib().armour_eval_candidates(self.h, N, _ptr(x), _ptr(cost), _ptr(viol), _iptr(feas), _iptr(best)))
        return dict(cost=cost, violation=viol, feasible=feas.astype(bool), best=best)

    def check_motion(self, traj, t0=0.0, t1=1.0, samples=11):
        """armour_check_motion: the smallest sampled separation between the arm and the obstacles of each
        world of the last batch. traj [W, 4, 7]: q0, qd0, qdd0 and k (normalised) per world; the
        trajectory is sampled at `samples` evenly spaced times in [t0, t1]. Returns (clearance [W],
        where [W, 3]: sample, link, obstacle of the first minimiser; +inf and -1 without obstacles)."""
        traj = np.ascontiguousarray(np.asarray(traj, dtype=np.float64))
        if traj.ndim != 3 or traj.shape[1:] != (4, NF) or traj.shape[0] != self._W:
            raise ValueError(f"check_motion: traj must have shape [W, 4, {NF}] (W = {self._W}), got {traj.shape}")
        clear = np.zeros(self._W)
        where = np.zeros((self._W, 3), dtype=np.int32)
        _check(lib().armour_check_motion(self.h, _ptr(traj), float(t0), float(t1), int(samples), _ptr(clear), _iptr(where)))
        return clear, where

    def track(self, traj, scale=None, err0=None, t0=0.0, t1=0.5, steps=250):
        """armour_track: the true arm under the robust controller along traj [N, 4, 7] (q0, qd0, qdd0, k
        normalised), for S parameter samples per trajectory: scale [N, S, 2, num_joints] (mass and inertia
        scales; [S, 2, num_joints] is used for every trajectory; None: nominal) and err0 [N, S, 2, 7] (the
        start's offset from the desired state; None: zero), classical RK4 with `steps` steps over [t0, t1].
        Needs no batch. Returns a dict: max_pos_err, max_vel_err, max_torque [N, S, 7], max_V, max_robust
        [N, S], end_state [N, S, 2, 7], status [N, S] (1: the rollout stopped being finite), track_ms, and
        the ultimate bounds qe, qde of the planner's tables the errors are read against."""
        traj, scale, err0, N, S = self._track_inputs("track", traj, scale, err0)
        out, o = self._track_outputs(N, S)
        _check(lib().armour_track(self.h, N, _ptr(traj), S, _ptr(scale), _ptr(err0), float(t0), float(t1), int(steps),
                                  ctypes.byref(o)))
        out["track_ms"] = float(o.track_ms)
        out["qe"], out["qde"] = self._ultimate_bound()
        return out

    def _track_inputs(self, name, traj, scale, err0, N=None, n="N"):
        """the shape checks of the tracking entries: (traj, scale, err0, N, S), contiguous float64. traj None
        (a tracked episode, which brings no trajectories): N worlds, called `n` in the messages"""
        if traj is not None:
            traj = np.ascontiguousarray(np.asarray(traj, dtype=np.float64))
            if traj.ndim != 3 or traj.shape[1:] != (4, NF) or traj.shape[0] < 1 or (N is not None and traj.shape[0] != N):
                raise ValueError(f"{name}: traj must have shape [{'N' if N is None else N}, 4, {NF}], got {traj.shape}")
            N = traj.shape[0]
        S = None
        if scale is not None:
            scale = np.asarray(scale, dtype=np.float64)
            if scale.ndim == 3:
                scale = np.broadcast_to(scale, (N,) + scale.shape)
            if scale.ndim != 4 or scale.shape[0] != N or scale.shape[1] < 1 or scale.shape[2:] != (2, self.NJ):
                raise ValueError(f"{name}: scale must have shape [{n}, S, 2, {self.NJ}] or [S, 2, {self.NJ}] ({n} = {N}), "
                                 f"got {scale.shape}")
            scale = np.ascontiguousarray(scale)
            S = scale.shape[1]
        if err0 is not None:
            err0 = np.ascontiguousarray(np.asarray(err0, dtype=np.float64))
            if err0.ndim != 4 or err0.shape[0] != N or err0.shape[1] < 1 or err0.shape[2:] != (2, NF) or \
                    (S is not None and err0.shape[1] != S):
                raise ValueError(f"{name}: err0 must have shape [{n}, S, 2, {NF}] ({n} = {N}, S = {S}), got {err0.shape}")
            S = err0.shape[1]
        return traj, scale, err0, N, 1 if S is None else S

    @staticmethod
    def _track_outputs(N, S):
        """(dict of the output arrays of armour_track_output, the structure that points at them)"""
        out = dict(max_pos_err=np.zeros((N, S, NF)), max_vel_err=np.zeros((N, S, NF)), max_torque=np.zeros((N, S, NF)),
                   max_V=np.zeros((N, S)), max_robust=np.zeros((N, S)), end_state=np.zeros((N, S, 2, NF)))
        out["status"] = np.zeros((N, S), dtype=np.int32)
        o = TrackOutput(*[_ptr(out[k]) for k in ("max_pos_err", "max_vel_err", "max_torque", "max_V", "max_robust",
                                                  "end_state")], _iptr(out["status"]), 0.0)
        return out, o

    def _ultimate_bound(self):
        """(qe, qde) of the planner's tables, as the library derives them"""
        r = getattr(self, "_robot", None)
        if r is None:
            from .robot_tables import ArmourRobot
            r = ArmourRobot()
            _check(lib().armour_robot_builtin(0, ctypes.byref(r)))
        eps = float(np.sqrt(2 * r.V_m / r.M_min))
        return eps / r.K, 2 * eps

    def track_motion(self, traj, scale=None, err0=None, t0=0.0, t1=0.5, steps=250, check_samples=11):
        """armour_track_motion: Planner.track for one trajectory per world of the last batch (traj [W, 4, 7],
        scale [W, S, 2, num_joints] / [S, 2, num_joints] / None, err0 [W, S, 2, 7] / None), with the true arm's
        states at `check_samples` check points (steps must be a multiple of check_samples - 1) tested
        against the world's own obstacles. Returns track's dict plus clearance [W, S], where [W, S, 3] (check
        point, link, obstacle), flags [W, S] (TRACK_COLLISION, TRACK_INPUT, TRACK_BOUND, TRACK_LIMIT,
        TRACK_NOT_FINITE), world_clearance [W], world_where [W, 4] (sample, check point, link, obstacle)
        and check_ms; +inf and -1 without obstacles."""
        traj, scale, err0, W, S = self._track_inputs("track_motion", traj, scale, err0, N=self._W)
        out, o = self._track_outputs(W, S)
        out.update(clearance=np.zeros((W, S)), where=np.zeros((W, S, 3), dtype=np.int32), flags=np.zeros((W, S), dtype=np.int32),
                   world_clearance=np.zeros(W), world_where=np.zeros((W, 4), dtype=np.int32))
        m = TrackMotionOutput(o, _ptr(out["clearance"]), _iptr(out["where"]), _iptr(out["flags"]), _ptr(out["world_clearance"]),
                              _iptr(out["world_where"]), 0.0)
        _check(lib().armour_track_motion(self.h, _ptr(traj), S, _ptr(scale), _ptr(err0), float(t0), float(t1), int(steps),
                                         int(check_samples), ctypes.byref(m)))
        out["track_ms"], out["check_ms"] = float(m.track.track_ms), float(m.check_ms)
        out["qe"], out["qde"] = self._ultimate_bound()
        return out

    def episode_begin(self, worlds, goals, lookahead=0.1, goal_radius=np.pi / 30, check_samples=11):
        """armour_episode_begin: start receding-horizon episodes of `worlds` (their q_des is ignored) toward
        `goals` [W, 7]; returns the initial states (episode_states)"""
        arr = self._worlds(worlds)
        goals = np.ascontiguousarray(np.asarray(goals, dtype=np.float64))
        if goals.shape != (len(worlds), NF):
            raise ValueError(f"episode_begin: goals must have shape [{len(worlds)}, {NF}], got {goals.shape}")
        cfg = EpisodeConfig(float(lookahead), float(goal_radius), int(check_samples))
        _check(lib().armour_episode_begin(self.h, len(worlds), arr, _ptr(goals), ctypes.byref(cfg)))
        return self.episode_states()

    def episode_step(self, reject=None):
        """armour_episode_step: plan every world from its pending state, execute, check and advance.
        reject [W] (optional): worlds whose new plan the caller vetoes. Returns (running worlds,
        results, timing) with results as plan_mixed's and timing's check_ms / advance_ms added."""
        rj = None
        if reject is not None:
            rj = np.ascontiguousarray(np.asarray(reject).astype(np.int32))
            if rj.shape != (self._W,):
                raise ValueError(f"episode_step: reject must have shape [{self._W}], got {rj.shape}")
        res = (Result * max(self._W, 1))()
        tm = Timing()
        ems = np.zeros(2)
        n = lib().armour_episode_step(self.h, _iptr(rj), res, ctypes.byref(tm), _ptr(ems))
        if n < 0:
            _check(n)
        t = self._span(tm.as_dict())
        t["check_ms"], t["advance_ms"] = float(ems[0]), float(ems[1])
        return n, self._results(res)[:self._W], t

    def episode_track(self, scale=None, err0=None, num_samples=None, steps=250, stop_on_input=True, stop_on_bound=True,
                      stop_on_limit=False):
        """armour_episode_track, after episode_begin and before the first step: from then on every step also
        rolls S true arms per world along what the world executes. scale [W, S, 2, num_joints] /
        [S, 2, num_joints] / None (nominal), err0 [W, S, 2, 7] / None (the first start's offset from the
        episode's start state); S comes from them, or from num_samples when both are None. steps must be a
        multiple of the episode's check_samples - 1. The stops default to the reference's (input and
        ultimate bound, not the joint limits)."""
        _, scale, err0, _, S = self._track_inputs("episode_track", None, scale, err0, N=self._W, n="W")
        if scale is None and err0 is None:
            S = 1 if num_samples is None else int(num_samples)
        elif num_samples is not None and int(num_samples) != S:
            raise ValueError(f"episode_track: num_samples = {num_samples} but the arrays carry {S} samples")
        cfg = EpisodeTrackConfig(S, _ptr(scale), _ptr(err0), int(steps), int(bool(stop_on_input)), int(bool(stop_on_bound)),
                                 int(bool(stop_on_limit)))
        _check(lib().armour_episode_track(self.h, ctypes.byref(cfg)))
        self._track_S = S

    def episode_tracked(self):
        """armour_episode_get_tracked: dict of arrays over the worlds: clearance [W], clearance_at [W, 4] (step,
        sample, link, obstacle), max_pos_err, max_vel_err, max_torque [W, 7], max_V, max_robust [W], flags
        [W], flag_step [W, 5]; and true_state [W, S, 2, 7], last_flags [W, S], rollout_ms, check_ms"""
        W, S = self._W, getattr(self, "_track_S", 1)
        rec = (EpisodeTracked * max(W, 1))()
        true = np.zeros((W, S, 2, NF))
        flags = np.zeros((W, S), dtype=np.int32)
        ms = np.zeros(2)
        _check(lib().armour_episode_get_tracked(self.h, rec, _ptr(true), _iptr(flags), _ptr(ms)))
        out = _records(EpisodeTracked, rec[:W])
        out.update(true_state=true, last_flags=flags, rollout_ms=float(ms[0]), check_ms=float(ms[1]))
        return out

    def _roadmap_inputs(self, name, nodes, connect_radius, edge_step, margin):
        nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        if nodes.ndim != 3 or nodes.shape[0] != self._W or nodes.shape[2] != NF:
            raise ValueError(f"{name}: nodes must have shape [{self._W}, N, {NF}], got {nodes.shape}")
        self._roadmap_N = nodes.shape[1]
        return nodes, RoadmapConfig(nodes.shape[1], float(connect_radius), float(edge_step), float(margin))

    def roadmap_build(self, nodes, goals, connect_radius=1.0, edge_step=0.05, margin=0.02):
        """armour_roadmap_build on the worlds of the last batch: nodes [W, N, 7], goals [W, 7] (each world's
        goal becomes vertex N); returns the stats as a dict (build_ms: the four passes' device milliseconds)"""
        nodes, cfg = self._roadmap_inputs("roadmap_build", nodes, connect_radius, edge_step, margin)
        goals = np.ascontiguousarray(goals, dtype=np.float64)
        if goals.shape != (self._W, NF):
            raise ValueError(f"roadmap_build: goals must have shape [{self._W}, {NF}], got {goals.shape}")
        st = RoadmapStats()
        _check(lib().armour_roadmap_build(self.h, ctypes.byref(cfg), _ptr(nodes), _ptr(goals), ctypes.byref(st)))
        out = {k: int(getattr(st, k)) for k, _ in RoadmapStats._fields_ if k != "build_ms"}
        out["build_ms"] = np.array(st.build_ms[:])
        return out

    def roadmap(self, w):
        """armour_roadmap_get: world w's graph as a dict: clearance, is_free, togo, next [N + 1] and adjacency
        [N + 1, 32] uint32 words (bit j of row i: the edge exists)"""
        V = getattr(self, "_roadmap_N", ROADMAP_MAX_NODES) + 1   # (before any build the library says so)
        clr, togo = np.zeros(V), np.zeros(V)
        free, nxt = np.zeros(V, dtype=np.int32), np.zeros(V, dtype=np.int32)
        adj = np.zeros((V, 32), dtype=np.uint32)
        _check(lib().armour_roadmap_get(self.h, int(w), _ptr(clr), _iptr(free), adj.ctypes.data_as(ctypes.POINTER(ctypes.c_uint)),
                                        _ptr(togo), _iptr(nxt)))
        return dict(clearance=clr, is_free=free, adjacency=adj, togo=togo, next=nxt)

    def roadmap_waypoint(self, q, lookahead=0.1):
        """armour_roadmap_waypoint at q [W, 7]: (q_des [W, 7], entry [W] (-1: the straight-line waypoint),
        path_left [W])"""
        q = np.ascontiguousarray(q, dtype=np.float64)
        if q.shape != (self._W, NF):
            raise ValueError(f"roadmap_waypoint: q must have shape [{self._W}, {NF}], got {q.shape}")
        q_des, left = np.zeros((self._W, NF)), np.zeros(self._W)
        entry = np.zeros(self._W, dtype=np.int32)
        _check(lib().armour_roadmap_waypoint(self.h, _ptr(q), float(lookahead), _ptr(q_des), _iptr(entry), _ptr(left)))
        return q_des, entry, left

    def episode_roadmap(self, nodes, connect_radius=1.0, edge_step=0.05, margin=0.02):
        """armour_episode_roadmap, after episode_begin and before the first step: from then on every waypoint
        comes from the roadmap of nodes [W, N, 7] and the episode's goals; returns the states (episode_states)"""
        nodes, cfg = self._roadmap_inputs("episode_roadmap", nodes, connect_radius, edge_step, margin)
        _check(lib().armour_episode_roadmap(self.h, ctypes.byref(cfg), _ptr(nodes)))
        return self.episode_states()

    def episode_roadmap_state(self):
        """armour_episode_get_roadmap: (entry [W], path_left [W]) of each world's last waypoint"""
        entry, left = np.zeros(self._W, dtype=np.int32), np.zeros(self._W)
        _check(lib().armour_episode_get_roadmap(self.h, _iptr(entry), _ptr(left)))
        return entry, left

    def episode_states(self):
        """armour_episode_get: dict of arrays over the worlds (q, qd, qdd, q_des [W, 7], status, mode, steps,
        failed_plans, failed_streak [W], clearance [W], clearance_at [W, 3], goal_distance [W])"""
        st = (EpisodeState * max(self._W, 1))()
        _check(lib().armour_episode_get(self.h, st))
        return _records(EpisodeState, st[:self._W])

    def constraints(self, w):
        g = np.zeros(self._m(w))
        _check(lib().armour_get_constraints(self.h, w, _ptr(g)))
        return g

    def link_centers(self, w):
        c = np.zeros((self.T, self.NJ, 3))
        _check(lib().armour_get_link_centers(self.h, w, _ptr(c)))
        return c

    def link_generators(self, w):
        """[T, NJ, 3, 6] (the armour_joint_position_radius.out payload)"""
        g = np.zeros((self.T, self.NJ, 3, 6))
        _check(lib().armour_get_link_generators(self.h, w, _ptr(g)))
        return g

    def joint_bounds(self):
        """the 28 trailing values of armour_constraints.out: per joint [lb + qe, ub - qe], then
        per joint [-v + qde, v - qde]"""
        b = np.zeros(28)
        _check(lib().armour_get_joint_bounds(self.h, _ptr(b)))
        return b

    def reach_program(self):
        """op codes of the reach kernel's program (diagnostics)"""
        n = lib().armour_get_reach_program(self.h, None, 0)
        codes = (ctypes.c_int * n)()
        lib().armour_get_reach_program(self.h, codes, n)
        return np.array(codes[:])

    def reach_dump(self):
        """[nops, 8] op-by-op state of job 0; needs ARMOUR_DUMP_OPS at creation"""
        n = lib().armour_get_reach_dump(self.h, None, 0)
        if n < 0:
            _check(n)
        d = np.zeros((n, 8))
        _check(min(0, lib().armour_get_reach_dump(self.h, _ptr(d), n)))
        return d

    def reach_profile(self):
        """([nops, 2] accumulated (cycles, terms) per op, [16] phase cycles);
        needs ARMOUR_PROFILE_OPS at creation"""
        n = lib().armour_get_reach_profile(self.h, None, 0)
        if n < 0:
            _check(n)
        buf = (ctypes.c_ulonglong * (2 * n + 16))()
        _check(min(0, lib().armour_get_reach_profile(self.h, buf, n + 8)))
        a = np.array(buf[:], dtype=np.uint64)
        return a[:2 * n].reshape(n, 2), a[2 * n:]

    def monomial_counts(self, w):
        """(link [T, NJ], torque [T, 7]) k-only monomial counts of world w"""
        lk = np.zeros((self.T, self.NJ), dtype=np.int32)
        tq = np.zeros((self.T, NF), dtype=np.int32)
        _check(lib().armour_get_monomial_counts(self.h, w, _iptr(lk), _iptr(tq)))
        return lk, tq

    OCCUPANCY = ("arena_hashes", "arena_rows", "operator_terms", "link_monomials", "torque_monomials",
                 "worlds_retried", "worlds_failed")

    def occupancy(self):
        """{name: (largest use in the last reach, capacity)} (armour_get_reach_occupancy)"""
        n = len(self.OCCUPANCY)
        used = (ctypes.c_longlong * n)()
        caps = (ctypes.c_longlong * n)()
        rc = lib().armour_get_reach_occupancy(self.h, used, caps, n)
        _check(min(0, rc))
        return {k: (int(used[i]), int(caps[i])) for i, k in enumerate(self.OCCUPANCY)}

    def reach_span_ms(self):
        """device-clock execution span of the last batch's first reach launch, ms (armour_get_reach_span;
        a capacity retry's launch is not included)"""
        v = ctypes.c_double()
        _check(lib().armour_get_reach_span(self.h, ctypes.byref(v)))
        return v.value

    def path_counts(self):
        """{name: launches or iterations since creation} of every host-side dispatch branch
        (armour_get_path_counts, with the library's own names: armour_path_name)"""
        L = lib()
        n = L.armour_get_path_counts(self.h, None, 0)
        _check(min(0, n))
        out = (ctypes.c_longlong * n)()
        _check(min(0, L.armour_get_path_counts(self.h, out, n)))
        return {L.armour_path_name(i).decode(): int(out[i]) for i in range(n)}

    def plane_cache_stats(self):
        """certified plane cache of the current reach sets (armour_get_plane_cache_stats)"""
        keys = ("planes_kept", "pairs", "blocks_cached", "blocks", "max_per_pair", "pool_records", "box_misses")
        out = (ctypes.c_longlong * len(keys))()
        _check(min(0, lib().armour_get_plane_cache_stats(self.h, out, len(keys))))
        return {k: int(out[i]) for i, k in enumerate(keys)}

    def torque_radius(self, w):
        r = np.zeros((self.T, NF))
        _check(lib().armour_get_torque_radius(self.h, w, _ptr(r)))
        return r


def roadmap_nodes(robot, q_start, goal, N, spread, rng):
    """One recipe for the nodes of a roadmap, [N, 7]: node n is q_start + u_n Delta(q_start -> goal) +
    spread g_n with u uniform on [0, 1] and g standard normal (Delta angle-wrapped on continuous joints,
    state_lb <= -1000); limited joints are clipped to their limits. Uniform sampling of the
    seven-dimensional box is hopeless at a thousand nodes, so this samples a tube round the straight
    line: `spread` (radians) is how far it looks for a way round. robot: a table dict with state_lb and
    state_ub (robot_tables); rng: a numpy Generator."""
    q_start, goal = np.asarray(q_start, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    lb, ub = np.asarray(robot["state_lb"], dtype=np.float64)[:NF], np.asarray(robot["state_ub"], dtype=np.float64)[:NF]
    cont = lb <= -1000.0
    d = goal - q_start
    d[cont] = (d[cont] + np.pi) % (2 * np.pi) - np.pi
    nodes = q_start + rng.uniform(0.0, 1.0, (N, 1)) * d + spread * rng.standard_normal((N, NF))
    nodes[:, ~cont] = np.clip(nodes[:, ~cont], lb[~cont], ub[~cont])
    return nodes


def run_episodes(planner, worlds, goals, max_steps, track=None, roadmap=None, **config):
    """Drive `worlds` toward `goals` [W, 7] with receding-horizon episodes on `planner` (episode_begin,
    then episode_step until no world runs or max_steps steps were taken; config: lookahead,
    goal_radius, check_samples). track (optional): the arguments of Planner.episode_track as a dict; the
    true arms are then rolled along every executed segment. roadmap (optional): the arguments of
    Planner.episode_roadmap as a dict (nodes [W, N, 7], connect_radius, edge_step, margin); the waypoints then
    come from that roadmap instead of the straight line. Returns dict(status, steps, clearance: [W]
    each), and with track also tracked: the records (Planner.episode_tracked)."""
    st = planner.episode_begin(worlds, goals, **config)
    if track is not None:
        planner.episode_track(**track)
    if roadmap is not None:
        st = planner.episode_roadmap(**roadmap)
    running = int(np.sum(st["status"] == 0))
    for _ in range(int(max_steps)):
        if running == 0:
            break
        running, _, _ = planner.episode_step()
    st = planner.episode_states()
    out = dict(status=st["status"], steps=st["steps"], clearance=st["clearance"])
    if track is not None:
        out["tracked"] = planner.episode_tracked()
    return out


class ArmtdPlanner(Planner):
    """The ARMTD comparison planner (armour_create_armtd). A world is the content of one armtd.in:
    (q0, qd0, q_des, jrs_tables[7, 6, T], k_range[7], obstacles[O, 12]) with the tables per joint
    c_cos, g_cos, r_cos, c_sin, g_sin, r_sin (ACMP/armtd_main.cu:37-102)."""

    def __init__(self, T=100, max_obstacles=20, max_worlds=1, device=0, max_iter=0, solver=None):
        super().__init__(T=T, max_obstacles=max_obstacles, max_worlds=max_worlds, device=device, max_iter=max_iter,
                         _armtd=True, solver=solver)

    def _worlds(self, worlds):
        n = len(worlds)
        arr = (ArmtdWorld * n)()
        keep = []
        for k, (q0, qd0, q_des, tab, kr, obs) in enumerate(worlds):
            a = arr[k]
            a.q0[:] = [float(v) for v in q0]
            a.qd0[:] = [float(v) for v in qd0]
            a.q_des[:] = [float(v) for v in q_des]
            a.k_range[:] = [float(v) for v in kr]
            t = np.ascontiguousarray(np.asarray(tab, dtype=np.float64).reshape(NF, 6, self.T))
            o = np.ascontiguousarray(np.asarray(obs, dtype=np.float64).reshape(-1, 12))
            keep += [t, o]
            a.jrs_tables = _ptr(t)
            a.num_obstacles = o.shape[0]
            a.obstacles = _ptr(o) if o.shape[0] else None
        self._keep = keep
        self.O = arr[0].num_obstacles if n else 0
        self._W = n
        return arr

    def _plan_call(self, *a):
        return lib().armour_plan_armtd_batch(*a)

    def _reach_call(self, *a):
        return lib().armour_reach_armtd_batch(*a)


__all__ = ["ArmtdPlanner", "Planner", "ArmourError", "ARMOUR_E_CAPACITY", "ARMOUR_E_INTERNAL", "copy_bandwidth", "default_batch", "make_world", "example_world", "csv_world", "straight_line_waypoint", "KINOVA", "LIB_PATH", "ABI_SYMBOLS", "candidates_array", "check_world", "check_armtd_world", "run_episodes", "EpisodeConfig", "EpisodeState", "T_PLAN", "EPISODE_STATUS", "TrackMotionOutput", "EpisodeTrackConfig", "EpisodeTracked", "RoadmapConfig", "RoadmapStats", "roadmap_nodes"]
