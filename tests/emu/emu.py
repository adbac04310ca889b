"""TEST HARNESS — ctypes wrapper of tests/emu/libreach_emu.so (sequential host emulation of the
reach kernel's op program, armour-dev_amd/csrc/reach.h)."""
import ctypes
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NJ, CAP_LM, CAP_UM = 7, 64, 256
_L = None


def lib():
    global _L
    if _L is None:
        _L = ctypes.CDLL(os.path.join(HERE, "libreach_emu.so"))
    return _L


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def set_robot(robot_struct=None):
    """robot tables (armour_amd.robot_tables.to_struct) for the following reach_job calls; None:
    the built-in Kinova Gen3"""
    global NJ
    if lib().emu_set_robot(ctypes.byref(robot_struct) if robot_struct is not None else None) != 0:
        raise ValueError("invalid robot tables")
    NJ = int(robot_struct.num_joints) if robot_struct is not None else 7


def program(robot_struct=None, fused=True):
    """[nops, 6] int array (code, o, a, b, c, i) of the reach program ProgramBuilder builds for the
    robot tables (None: the built-in Kinova Gen3)"""
    r = ctypes.byref(robot_struct) if robot_struct is not None else None
    n = lib().emu_program_robot(r, 0 if fused else 1, None, 0)
    if n < 0:
        raise ValueError("invalid robot tables")
    out = np.zeros((n, 6), np.int32)
    lib().emu_program_robot(r, 0 if fused else 1, _p(out), n)
    return out


MAX_SLOTS = 96       # pz_engine.h: handle slots of a reach program
POOL_DOUBLES = 1024  # reach_kernel.hip: the per-job engine's LDS payload pool


def program_size(robot_struct=None):
    """(handle slots, payload doubles) the reach program of the robot tables needs; a planner is
    refused above MAX_SLOTS, and on the per-job engine above POOL_DOUBLES (planner.hip)"""
    r = ctypes.byref(robot_struct) if robot_struct is not None else None
    ns, pool = ctypes.c_int(), ctypes.c_int()
    if lib().emu_program_size(r, ctypes.byref(ns), ctypes.byref(pool)) != 0:
        raise ValueError("invalid robot tables")
    return ns.value, pool.value


def reach_job(world, T, t, fused=True):
    """Outputs of job (world, t) as the kernel writes them (fused: the program's cross products
    as single ops, else composed from views / products / differences / stack)."""
    lib().emu_set_unfused(0 if fused else 1)
    q0, qd0, qdd0 = [np.ascontiguousarray(np.asarray(a, dtype=np.float64)) for a in world[:3]]
    o = dict(link_gens=np.zeros((NJ, 18)), link_center=np.zeros((NJ, 3)), link_rad=np.zeros((NJ, 3)),
             link_cnt=np.zeros(NJ, np.int32), link_hash=np.zeros((NJ, CAP_LM), np.uint16),
             link_coef=np.zeros((NJ, CAP_LM, 3)), tq_center=np.zeros(7), tq_rad=np.zeros(7),
             tq_cnt=np.zeros(7, np.int32), tq_hash=np.zeros((7, CAP_UM), np.uint16), tq_coef=np.zeros((7, CAP_UM)),
             torque_radius=np.zeros(7))
    used, bts, nops, nsl = ctypes.c_long(), ctypes.c_double(), ctypes.c_int(), ctypes.c_int()
    order = ["link_gens", "link_center", "link_rad", "link_cnt", "link_hash", "link_coef", "tq_center", "tq_rad",
             "tq_cnt", "tq_hash", "tq_coef", "torque_radius"]
    err = lib().emu_reach(T, t, _p(q0), _p(qd0), _p(qdd0), *[_p(o[k]) for k in order], ctypes.byref(used),
                          ctypes.byref(bts), ctypes.byref(nops), ctypes.byref(nsl))
    o.update(err=err, arena=used.value, bytes=bts.value, nops=nops.value, nslots=nsl.value)
    return o
