"""Robot tables beyond the two the suite grew up on (tests/robot_variants.py): reversed joint axes,
nine joints, fixed frames with a generic roll / pitch / yaw — on the CPU: the point models, the
oracle and the host emulation of the reach program.

A joint with axis code -a turns about -e_a: R = Rot(e_a, -q), its angular rates are -qd e_a, its
generalised torque is -n[a] + armature qdd + damping qd (include/armour_hip.h). The checks:

  * the point models alone: Rodrigues' rotation about -e_a against the substitution q -> -q, and the
    point RNEA of a reversed robot at the mirrored state against sigma o RNEA of the base robot;
  * containment: the oracle's and the emulated reach program's sliced sets enclose the point models
    (test_oracle_containment.containment, at its SLACK) for all four variants;
  * the emulated program against the oracle at tests/test_emu.py's tolerances, monomial structure
    included;
  * the mirror identity (robot_variants.mirror_rows) on the oracle: every line at TOL = 1e-9, plans
    at the bar of robot_variants.assert_mirror_plan;
  * a robot without a reversed joint gets the op program it had before reversed axes were honoured
    (tests/golden/reach_program_parent.json, recorded from that code);
  * from_urdf on a URDF with <axis xyz="0 0 -1"/>.
"""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.join(os.path.dirname(__file__), "emu"))
import emu  # noqa: E402

import armour_amd as A  # noqa: E402
import point_model as PM  # noqa: E402
import robot_variants as RV  # noqa: E402
from armour_amd import robot_tables as RT  # noqa: E402
from oracle import OraclePlanner  # noqa: E402
from test_oracle_containment import SLACK, containment, oracle_sets  # noqa: E402

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TOL = 1e-9   # the parity tests' tolerance on reach outputs, constraints and Jacobians
T = 10
SEEDS = (40, 41)


# ---- the point models alone ----------------------------------------------------------------------
@pytest.mark.parametrize("a", [1, 2, 3])
def test_rot_axis_of_a_reversed_axis(a):
    q = np.array([0.0, 0.3, -1.2, 2.9, np.pi / 2])
    Rn, Rp = PM.rot_axis(-a, q), PM.rot_axis(a, q)
    np.testing.assert_allclose(Rn, PM.rot_axis(a, -q), rtol=0, atol=1e-15)
    np.testing.assert_allclose(Rn, np.swapaxes(Rp, -1, -2), rtol=0, atol=1e-15)
    u = PM.axis_vector(-a)
    assert u[a - 1] == -1.0 and np.abs(u).sum() == 1.0
    np.testing.assert_allclose(Rn @ u, np.broadcast_to(u, (len(q), 3)), rtol=0, atol=1e-15)   # the axis is fixed
    # a small positive turn about u moves a vector v towards u x v
    v = np.roll(np.abs(u), 1)
    np.testing.assert_allclose((PM.rot_axis(-a, np.array(1e-6)) @ v - v) / 1e-6, np.cross(u, v), rtol=0, atol=1e-6)


@pytest.mark.parametrize("name,joints", [("kinova", (0, 3, 6)), ("fetch", (1, 2, 5)), ("KINOVA_9", (1,)),
                                         ("FETCH_9", (0, 4))])
def test_point_rnea_mirror(name, joints):
    """RNEA of the reversed robot at the mirrored state = sigma o RNEA of the base robot, and its link
    points are the base robot's"""
    base = {"kinova": RV.kinova, "fetch": RV.fetch, "KINOVA_9": lambda: RV.base_of("KINOVA_9"),
            "FETCH_9": lambda: RV.base_of("FETCH_9_REV")}[name]()
    rev = RV.reversed_robot(base, joints)
    s = RV.sigma(joints)
    rng = np.random.default_rng(5)
    q, qd, qda, qdd = (rng.uniform(-1.5, 1.5, (6, 7)) for _ in range(4))
    u = PM.rnea(base, q, qd, qda, qdd)
    ur = PM.rnea(rev, s * q, s * qd, s * qda, s * qdd)
    assert np.abs(u).max() > 1.0
    np.testing.assert_allclose(ur, s * u, rtol=0, atol=1e-12 * max(1.0, np.abs(u).max()))
    np.testing.assert_allclose(PM.link_points(rev, s * q), PM.link_points(base, q), rtol=0, atol=1e-14)
    # and reversing a joint without mirroring the state is another arm: the check can fail
    assert np.abs(PM.link_points(rev, q) - PM.link_points(base, q)).max() > 1e-2


def test_variant_tables():
    kin, fet = RV.kinova(), RV.fetch()
    kr, fr, k9, f9 = (RV.variant(n) for n in RV.NAMES)
    assert list(kr["axes"]) == [-3, 3, 3, -3, 3, 3, -3] and int(kr["num_joints"]) == 7
    assert list(fr["axes"]) == [3, -2, -1, 2, 1, -2, 1, 0]
    # Fetch joint 1 has asymmetric limits: the swap shows
    assert (fet["state_lb"][1], fet["state_ub"][1]) == (-1.221, 1.518)
    assert (fr["state_lb"][1], fr["state_ub"][1]) == (-1.518, 1.221)
    assert (fr["state_lb"][2], fr["state_ub"][2]) == (-1000.0, 1000.0)
    assert int(k9["num_joints"]) == 9 and list(k9["axes"]) == [3] * 7 + [0, 0]
    assert int(f9["num_joints"]) == 9 and list(f9["axes"]) == [-3, 2, 1, 2, -1, 2, 1, 0, 0]
    for r, base, n in ((k9, kin, 2), (f9, fet, 1)):
        nj = int(base["num_joints"])
        assert r["trans"].shape == (nj + n + 1, 3) and np.all(r["trans"][-1] == 0)
        assert np.array_equal(r["trans"][:nj], base["trans"][:nj])
        for i in range(nj, nj + n):
            assert np.all(r["trans"][i] != 0) and r["mass"][i] > 0 and np.all(r["com"][i] != 0)
            assert np.all(r["inertia"][i] != 0) and np.array_equal(r["inertia"][i], r["inertia"][i].T)
            assert np.all(r["link_generators"][i] > 0)
            # generic: no entry of the frame's rotation matrix is 0 or +-1
            Rm = PM.rpy(*r["rots"][i])
            assert np.all(np.abs(Rm) > 1e-3) and np.all(np.abs(Rm) < 1 - 1e-3)
    w = (np.arange(7.0), -np.arange(7.0), np.ones(7), np.full(7, 2.0), np.zeros((2, 12)))
    m = RV.mirror_world(w, (1, 5))
    assert np.array_equal(m[0], [0, -1, 2, 3, 4, -5, 6]) and np.array_equal(m[3], [2, -2, 2, 2, 2, -2, 2])


# ---- the oracle and the emulated program on the variants -----------------------------------------
def monomials(hashes, x):
    """value at x of each k-only monomial hash (common.h: 2 bits of degree per factor)"""
    h = np.asarray(hashes, dtype=np.int64)
    deg = (h[..., None] >> (2 * np.arange(7))) & 3
    return np.prod(np.asarray(x)[None, :] ** deg, axis=-1)


def emulated_jobs(world):
    """the emulated reach program's outputs of every job (world, t) for the robot set in emu"""
    jobs = [emu.reach_job(world, T, t) for t in range(T)]
    assert all(o["err"] == 0 for o in jobs)
    return jobs


@pytest.fixture(scope="module", params=RV.NAMES)
def variant_runs(request):
    """one variant: its tables, two survey worlds, their oracles after reach() and the emulated
    program's outputs of every job (computed once, shared, left unchanged)"""
    name = request.param
    robot = RV.variant(name)
    worlds = [A.make_world(s, 4, robot=RT.geometry(robot), profile="survey") for s in SEEDS]
    oracles = []
    for w in worlds:
        R = OraclePlanner(*w, T=T, threads=8, robot=RT.to_struct(robot))
        R.reach()
        oracles.append(R)
    emu.set_robot(RT.to_struct(robot))
    try:
        jobs = [emulated_jobs(w) for w in worlds]
    finally:
        emu.set_robot(None)
    return dict(name=name, robot=robot, worlds=worlds, oracles=oracles, jobs=jobs)


def _points(rng):
    return np.zeros(7), rng.uniform(-1, 1, 7), np.sign(rng.uniform(-1, 1, 7))


def test_oracle_sets_contain_point_models(variant_runs):
    v = variant_runs
    for w, (world, R) in enumerate(zip(v["worlds"], v["oracles"])):
        rng = np.random.default_rng(11 + w)
        for x in _points(rng):
            lw, tw, _ = containment(v["robot"], world, T, x, *oracle_sets(R, x), rng, n_t=4)
            print(f"{v['name']} world {w}: link excess {lw:.3e} m, torque excess {tw:.3e} N m")
            assert lw <= SLACK, f"link point outside its zonotope by {lw:.3e} m at x={x}"
            assert tw <= SLACK, f"torque outside centre +- radius by {tw:.3e} N m at x={x}"


def _slice_jobs(robot, jobs, x):
    """(centres [T, NJ, 3], gens [T, NJ, 3, 6], torque centres [T, 7], torque radius [T, 7]) of the
    emulated outputs sliced at x"""
    NJ = int(robot["num_joints"])
    lc, tc = np.zeros((T, NJ, 3)), np.zeros((T, 7))
    for t, o in enumerate(jobs):
        for l in range(NJ):
            n = o["link_cnt"][l]
            lc[t, l] = o["link_center"][l] + monomials(o["link_hash"][l, :n], x) @ o["link_coef"][l, :n]
        for j in range(7):
            n = o["tq_cnt"][j]
            tc[t, j] = o["tq_center"][j] + monomials(o["tq_hash"][j, :n], x) @ o["tq_coef"][j, :n]
    lg = np.stack([o["link_gens"].reshape(NJ, 6, 3).transpose(0, 2, 1) for o in jobs])
    tr = np.stack([o["torque_radius"] for o in jobs])
    return lc, lg, tc, tr


def test_emulated_sets_contain_point_models(variant_runs):
    v = variant_runs
    for w, (world, jobs) in enumerate(zip(v["worlds"], v["jobs"])):
        rng = np.random.default_rng(11 + w)
        for x in _points(rng):
            lw, tw, _ = containment(v["robot"], world, T, x, *_slice_jobs(v["robot"], jobs, x), rng, n_t=4)
            print(f"{v['name']} world {w}: link excess {lw:.3e} m, torque excess {tw:.3e} N m")
            assert lw <= SLACK, f"link point outside its zonotope by {lw:.3e} m at x={x}"
            assert tw <= SLACK, f"torque outside centre +- radius by {tw:.3e} N m at x={x}"


def test_emulated_program_matches_oracle(variant_runs):
    """tests/test_emu.py's comparison (same monomials, values to rounding) on every link of the variants"""
    v = variant_runs
    NJ = int(v["robot"]["num_joints"])
    for R, jobs in zip(v["oracles"], v["jobs"]):
        lg_o = R.get(0).reshape(T, NJ, 18)
        tr_o = R.torque_radius()
        for t in (0, 4, 9):
            o = jobs[t]
            np.testing.assert_allclose(o["link_gens"], lg_o[t], rtol=0, atol=1e-14)
            np.testing.assert_allclose(o["torque_radius"], tr_o[t], rtol=0, atol=1e-12)
            for l in range(NJ):
                pz = R.pz(0, l * T + t)
                n = o["link_cnt"][l]
                assert n == len(pz["hashes"])
                np.testing.assert_array_equal(o["link_hash"][l, :n], pz["hashes"])
                np.testing.assert_allclose(o["link_coef"][l, :n], pz["coeffs"], rtol=0, atol=1e-14)
                np.testing.assert_allclose(o["link_center"][l], pz["center"], rtol=0, atol=1e-14)
                np.testing.assert_allclose(o["link_rad"][l], pz["indep"], rtol=0, atol=1e-14)
            for j in range(7):
                pz = R.pz(1, j * T + t)
                n = o["tq_cnt"][j]
                assert n == len(pz["hashes"])
                np.testing.assert_array_equal(o["tq_hash"][j, :n], pz["hashes"])
                np.testing.assert_allclose(o["tq_coef"][j, :n], pz["coeffs"][:, 0], rtol=0, atol=1e-13)
                np.testing.assert_allclose(o["tq_center"][j], pz["center"][0], rtol=0, atol=1e-12)
                np.testing.assert_allclose(o["tq_rad"][j], pz["indep"][0], rtol=0, atol=1e-12)
        # the slicing used by the containment test is the oracle's own
        x = np.linspace(-0.9, 0.8, 7)
        g, lc = R.eval(x, jac=False, centers=True)
        lce, _, tce, _ = _slice_jobs(v["robot"], jobs, x)
        np.testing.assert_allclose(lce, lc, rtol=0, atol=1e-13)
        np.testing.assert_allclose(tce, g[:7 * T].reshape(T, 7), rtol=0, atol=1e-11)


def test_program_is_unchanged_without_a_reversed_joint():
    """Kinova and Fetch: the op program, operand for operand, recorded before reversed axes were
    honoured; a reversed joint changes one view's scale flag and no op"""
    with open(os.path.join(GOLD, "reach_program_parent.json")) as f:
        want = json.load(f)
    assert np.array_equal(emu.program(None), np.array(want["kinova"]))
    assert np.array_equal(emu.program(RT.to_struct(RV.fetch())), np.array(want["fetch"]))
    for name, base in (("KINOVA_REV", "kinova"), ("FETCH_REV", "fetch")):
        p = emu.program(RT.to_struct(RV.variant(name)))
        q = np.array(want[base])
        assert np.array_equal(p[:, :3], q[:, :3]) and np.array_equal(p[:, 4:], q[:, 4:])   # code, o, a, c, i
        # per reversed joint, the view that picks the torque's moment carries a scale (-1)
        assert 0 < np.count_nonzero(p != q) == len(RV.SPECS[name][2])
        assert set(p[p[:, 3] != q[:, 3], 0]) == {6}   # OP_VIEW (reach.h)


def _fits(robot):
    return emu.program_size(RT.to_struct(robot))[1] <= emu.POOL_DOUBLES


def test_per_job_engine_fit():
    """a Kinova with reversed joints keeps the per-job engine (the single-plan drop-in's); 8 and 9
    joints do not fit it"""
    assert emu.program_size(RT.to_struct(RV.variant("KINOVA_REV"))) == emu.program_size(None)
    assert _fits(RV.variant("KINOVA_REV"))
    assert not any(_fits(RV.variant(n)) for n in ("FETCH_REV", "KINOVA_9", "FETCH_9_REV"))
    assert all(emu.program_size(RT.to_struct(RV.variant(n)))[0] <= emu.MAX_SLOTS for n in RV.NAMES)


# ---- the mirror identity on the oracle -----------------------------------------------------------
def _oracle_eval(R, x):
    g, J, lc = R.eval(x, centers=True)
    return dict(centers=lc, gens=R.link_gens(), radius=R.torque_radius(), g=g, J=J)


@pytest.mark.parametrize("case", list(RV.MIRROR_CASES))
def test_mirror_identity_on_the_oracle(case):
    """every line of the identity on the checker alone, at the seeds the GPU test uses"""
    build, joints, seeds = RV.MIRROR_CASES[case]
    Ar = build()
    Br = RV.reversed_robot(Ar, joints)
    s = RV.sigma(joints)
    NJ = int(Ar["num_joints"])
    feas = []
    for seed in seeds:
        wA = A.make_world(seed, RV.MIRROR_O, robot=RT.geometry(Ar))
        wB = RV.mirror_world(wA, joints)
        RA = OraclePlanner(*wA, T=RV.MIRROR_T, threads=8, robot=RT.to_struct(Ar))
        RB = OraclePlanner(*wB, T=RV.MIRROR_T, threads=8, robot=RT.to_struct(Br))
        RA.reach()
        RB.reach()
        for x in RV.MIRROR_X:
            d = RV.mirror_eval_diffs(_oracle_eval(RA, x), _oracle_eval(RB, s * x), RV.MIRROR_T, NJ, RV.MIRROR_O, joints)
            print(case, seed, {k: f"{v:.1e}" for k, v in d.items()})
            assert max(d.values()) <= TOL, (case, seed, d)
        ra, rb = RA.plan(), RB.plan()
        print(case, seed, ra["feasible"], ra["status"], ra["iterations"], np.abs(rb["k_opt"] - s * ra["k_opt"]).max())
        RV.assert_mirror_plan(ra, rb, joints, (case, seed))
        assert ra["status"] == 0 or not ra["feasible"]
        feas.append(ra["feasible"])
    # two feasible worlds and one infeasible per robot; Fetch has no infeasible world in the default
    # profile (robot_variants.MIRROR_FEASIBLE)
    assert tuple(feas) == RV.MIRROR_FEASIBLE[case] and sum(feas) >= 2, feas
    assert case == "fetch" or len(feas) - sum(feas) >= 1, feas


# ---- from_urdf -----------------------------------------------------------------------------------
URDF = """<robot name="three">
 <link name="base"/><link name="l1"/><link name="l2"/><link name="l3"/>
 <joint name="j1" type="revolute"><parent link="base"/><child link="l1"/><origin xyz="0 0 0.1" rpy="0 0 0"/><axis xyz="0 0 -1"/><limit lower="-1.0" upper="2.0" velocity="1" effort="10"/></joint>
 <joint name="j2" type="revolute"><parent link="l1"/><child link="l2"/><origin xyz="0.2 0 0" rpy="0.1 0 0"/><axis xyz="0 -1 0"/><limit lower="-1.5" upper="0.5" velocity="1" effort="10"/></joint>
 <joint name="j3" type="continuous"><parent link="l2"/><child link="l3"/><origin xyz="0 0.3 0" rpy="0 0 0"/><axis xyz="1 0 0"/><limit velocity="1" effort="10"/></joint>
</robot>
"""


def test_from_urdf_reads_a_reversed_axis(tmp_path):
    path = tmp_path / "three.urdf"
    path.write_text(URDF)
    t = RT.from_urdf(str(path), 3)
    assert list(t["axes"]) == [-3, -2, 1]
    assert list(t["state_lb"]) == [-1.0, -1.5, -1000.0] and list(t["state_ub"]) == [2.0, 0.5, 1000.0]
    # the world generator's point FK of these tables puts the links where the point model does
    robot = dict(num_joints=3, axes=t["axes"], rots=t["rots"], trans=t["trans"], link_center=t["link_center"],
                 link_generators=t["link_generators"])
    geo = RT.geometry(t)
    q = np.array([0.7, -0.4, 1.1])
    cs, _ = A.worlds.link_spheres(geo, q)
    pm = PM.link_points(robot, q[None, :], box_coords=np.zeros((1, 3)))[:, 0, 0, :]
    np.testing.assert_allclose(cs, pm, rtol=0, atol=1e-15)
    # against the reversal ignored: a different arm
    wrong = dict(robot, axes=np.abs(t["axes"]))
    assert np.abs(PM.link_points(wrong, q[None, :], box_coords=np.zeros((1, 3)))[:, 0, 0, :] - cs).max() > 0.05
