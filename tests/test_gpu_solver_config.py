"""The optional solver configurations on the device (armour_solver_options: the quality-function barrier
oracle with the obj-constr-filter globalisation, strategies 2 and 3, the sigma grid and the limited-memory
BFGS) against the oracle's plans frozen in tests/golden/solver_config.npz (tests/make_solver_config.py).

Bar against the fixture, per world: status and feasibility identical. A converged or feasible world:
iterations and evaluations identical when the oracle's own plans under noise kept theirs (dit_noise 0),
k_opt within max(1e-8, 10 dk_noise[w]) (the tenfold margin over the oracle's own movement under noise is
tests/test_domain_edges.py's), cost within rtol 1e-8 where k_opt is held to 1e-8. An infeasible status-4
world: iterations within max(5, 2 dit_noise[w]) (tests/test_gpu_boundary.py's rule), k_opt not compared.
At most one world per set may miss its per-world bars (a sigma tie the three noise levels did not
sample); it must keep status and feasibility and lie within 10 iterations, and is printed.

Every test asserts its paths: a variant planner shows solve_quality / qf_sigma / hess_lbfgs as its
configuration says and no solve_adaptive; a default planner the reverse."""
import numpy as np
import pytest

import armour_amd as A
import make_solver_config as M
from paths import assert_paths, taken
from test_gpu_plane_cache import env

pytestmark = pytest.mark.gpu
REF = M.REFERENCE
_sets = {}


def fixture():
    if "fx" not in _sets:
        _sets["fx"] = dict(np.load(M.OUT))
    return _sets["fx"]


def worlds_of(name):
    """(T, O, worlds, armtd) of a set, built once and left unchanged"""
    if name not in _sets:
        _sets[name] = M.set_worlds(name)
    return _sets[name]


def options(cfg):
    return dict(mu_strategy=cfg[0], qf_grid=cfg[1], lbfgs_history=cfg[2])


def planner(name, W, cfg=None, **kw):
    T, O, _, armtd = worlds_of(name)
    return (A.ArmtdPlanner if armtd else A.Planner)(T=T, max_obstacles=O, max_worlds=W, solver=options(cfg) if cfg else None, **kw)


def variant_paths(cfg):
    """assert_paths' arguments for a planner that only ever solved under cfg"""
    ran, not_ran = [], []
    (ran if cfg[0] >= 2 else not_ran).extend(["solve_quality", "qf_sigma"])
    (ran if cfg[0] == 1 else not_ran).append("solve_adaptive")
    (ran if cfg[2] > 0 else not_ran).append("hess_lbfgs")
    return dict(ran=tuple(ran), not_ran=tuple(not_ran) + ("solve_monotone",))


DEFAULT_PATHS = dict(ran=("solve_adaptive",), not_ran=("solve_quality", "qf_sigma", "hess_lbfgs", "solve_monotone"))


def tolerances(fx, name, cfg, w):
    """(k_opt tolerance, iterations must be identical) of world w's converged or feasible plan"""
    pre = f"{name}/{M.key(cfg)}/"
    return max(1e-8, 10.0 * float(fx[pre + "dk_noise"][w])), int(fx[pre + "dit_noise"][w]) == 0


def compare(name, cfg, res, n=None):
    """the bar of the module's docstring on the first n worlds of a set"""
    fx = fixture()
    pre = f"{name}/{M.key(cfg)}/"
    n = len(res) if n is None else n
    missed, loose = [], 0
    for w in range(n):
        r = res[w]
        st, feas, it, ev = (int(fx[pre + k][w]) for k in ("status", "feasible", "iterations", "evaluations"))
        dk = float(np.abs(r["k_opt"] - fx[pre + "k_opt"][w]).max())
        tol, exact = tolerances(fx, name, cfg, w)
        print(f"{name} {M.key(cfg)} world {w}: status {r['status']}/{st} feasible {int(r['feasible'])}/{feas} iterations "
              f"{r['iterations']}/{it} evaluations {r['evaluations']}/{ev} |dk_opt| {dk:.1e} (tol {tol:.1e}) error {r['error']}")
        assert r["error"] == 0, w
        assert (r["status"], bool(r["feasible"])) == (st, bool(feas)), (name, cfg, w, r["status"], st, r["feasible"], feas)
        why = []
        if st == 0 or feas:
            loose += tol > 1e-6 or not exact
            if exact and (r["iterations"], r["evaluations"]) != (it, ev):
                why.append(f"iterations {r['iterations']} evaluations {r['evaluations']}, not {it} {ev}")
            if dk > tol:
                why.append(f"|dk_opt| {dk:.2e} > {tol:.1e}")
            if tol == 1e-8 and not np.isclose(r["cost"], float(fx[pre + "cost"][w]), rtol=1e-8, atol=0):
                why.append(f"cost {r['cost']!r}, not {float(fx[pre + 'cost'][w])!r}")
        elif st == 4:
            lim = max(5, 2 * int(fx[pre + "dit_noise"][w]))
            if abs(r["iterations"] - it) > lim:
                why.append(f"iterations {r['iterations']}, not within {lim} of {it}")
        if why:
            assert abs(r["iterations"] - it) <= 10, (name, cfg, w, why)
            missed.append((w, why))
    for w, why in missed:
        print(f"{name} {M.key(cfg)} world {w} misses its bars (the one-world allowance): {'; '.join(why)}")
    assert 10 * loose <= n, (name, cfg, "loose worlds", loose, n)
    assert len(missed) <= 1, (name, cfg, missed)


def assert_bitwise(P, Q, ra, rb):
    for w, (a, b) in enumerate(zip(ra, rb)):
        assert np.array_equal(a["k_opt"], b["k_opt"]) and a["cost"] == b["cost"], w
        assert (a["iterations"], a["evaluations"], a["status"], a["feasible"], a["error"]) == \
            (b["iterations"], b["evaluations"], b["status"], b["feasible"], b["error"]), w
        assert np.array_equal(P.constraints(w), Q.constraints(w)), w


# ---- 1. the reference's configuration -------------------------------------------------------------
def test_reference_configuration_survey():
    """48 survey worlds at T = 20, O = 8 (1295 rows, two row blocks)"""
    _, _, worlds, _ = worlds_of("survey_T20_O8")
    P = planner("survey_T20_O8", 48, REF)
    res, _ = P.plan(worlds[:48])
    compare("survey_T20_O8", REF, res, 48)
    assert_paths(P.path_counts(), **variant_paths(REF))
    P.close()


def test_reference_configuration_boundary():
    """the small boundary set (12 worlds, all inside the sync-free tail); the default planner beside it
    shows the reverse census"""
    _, _, worlds, _ = worlds_of("boundary_small_T20_O6")
    P = planner("boundary_small_T20_O6", len(worlds), REF)
    res, _ = P.plan(worlds)
    compare("boundary_small_T20_O6", REF, res)
    c = P.path_counts()
    assert_paths(c, ran=variant_paths(REF)["ran"] + ("ipm_iter_tail",), not_ran=variant_paths(REF)["not_ran"])
    assert c["qf_sigma"] == c["ipm_iter_sync"] + c["ipm_iter_tail"], c  # one search launch per iteration
    D = planner("boundary_small_T20_O6", len(worlds))
    D.plan(worlds)
    assert_paths(D.path_counts(), **DEFAULT_PATHS)
    P.close()
    D.close()


def test_reference_configuration_armtd():
    """the ARMTD planner's eight worlds (7035 rows, seven row blocks); world 2 restarts the interior
    point after a restoration phase at iteration 7: the reset of the option state"""
    fx = fixture()
    _, _, worlds, _ = worlds_of("armtd_T100_O10")
    assert int(fx[f"armtd_T100_O10/{M.key(REF)}/restart_iter"][2]) == 7
    P = planner("armtd_T100_O10", len(worlds), REF)
    res, _ = P.plan(worlds)
    compare("armtd_T100_O10", REF, res)
    assert_paths(P.path_counts(), ran=variant_paths(REF)["ran"] + ("ipm_restarts", "eval_armtd_f64"), not_ran=variant_paths(REF)["not_ran"])
    P.close()


# ---- 2. each knob alone ---------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", [(3, 16, 0), (1, 16, 6), (2, 8, 6)], ids=M.key)
def test_each_knob_alone(cfg):
    """(3, 16, 0) the oracle pair with the default's floor and grid; (1, -, 6) L-BFGS alone, worlds 1, 8
    and 9 restart (the history reset); (2, 8, 6) an eight-point grid, world 8 restarts"""
    fx = fixture()
    name = "boundary_small_T20_O6"
    _, _, worlds, _ = worlds_of(name)
    restarts = [w for w, r in enumerate(fx[f"{name}/{M.key(cfg)}/restart_iter"]) if r >= 0]
    assert restarts == {(3, 16, 0): [], (1, 16, 6): [1, 8, 9], (2, 8, 6): [8]}[cfg]
    P = planner(name, len(worlds), cfg)
    assert P.solver_options() == options(cfg)
    res, _ = P.plan(worlds)
    compare(name, cfg, res)
    v = variant_paths(cfg)
    assert_paths(P.path_counts(), ran=v["ran"] + (("ipm_restarts",) if restarts else ()), not_ran=v["not_ran"])
    P.close()


# ---- 3. mixed batch -------------------------------------------------------------------------------
def test_mixed_batch_is_bitwise_the_uniform_batches():
    """12 survey worlds at O in {0, 3, 8}, cycling, under the reference's configuration: each world's plan
    is bitwise the plan of a uniform batch of its count (O = 0 leaves only torque and extremum rows)"""
    T, _, worlds, _ = worlds_of("survey_T20_O8")
    counts = [(0, 3, 8)[w % 3] for w in range(12)]
    mixed = [worlds[w][:4] + (worlds[w][4][:c],) for w, c in enumerate(counts)]
    P = A.Planner(T=T, max_obstacles=8, max_worlds=12, solver=options(REF))
    rm, _ = P.plan_mixed(mixed)
    gm = [P.constraints(w) for w in range(12)]
    assert_paths(P.path_counts(), ran=variant_paths(REF)["ran"] + ("batch_mixed",), not_ran=variant_paths(REF)["not_ran"] + ("batch_uniform",))
    assert len({r["iterations"] for r in rm}) > 2 and all(r["error"] == 0 for r in rm)
    for c in (0, 3, 8):
        idx = [w for w in range(12) if counts[w] == c]
        U = A.Planner(T=T, max_obstacles=8, max_worlds=len(idx), solver=options(REF))
        ru, _ = U.plan([mixed[w] for w in idx])
        assert_paths(U.path_counts(), ran=variant_paths(REF)["ran"] + ("batch_uniform",), not_ran=variant_paths(REF)["not_ran"] + ("batch_mixed",))
        for k, w in enumerate(idx):
            a, b = rm[w], ru[k]
            assert np.array_equal(a["k_opt"], b["k_opt"]) and a["cost"] == b["cost"], (c, w)
            assert (a["iterations"], a["evaluations"], a["status"], a["feasible"]) == (b["iterations"], b["evaluations"], b["status"], b["feasible"]), (c, w)
            assert np.array_equal(gm[w], U.constraints(k)), (c, w)
        U.close()
    P.close()


# ---- 4. loop forms --------------------------------------------------------------------------------
LOOP_FORMS = {
    "ARMOUR_TAIL_WORLDS=0": dict(ran=("ipm_iter_sync",), not_ran=("ipm_iter_tail", "ls_one_round")),
    "ARMOUR_TAIL_WORLDS=1000": dict(ran=("ipm_iter_tail", ("ls_one_round", "ls_speculative"))),
    "ARMOUR_TAIL_SEARCH=one": dict(ran=("ipm_iter_tail", "ls_one_round")),
    "ARMOUR_NO_SPEC=1": dict(ran=("ls_sequential", "ipm_iter_sync"), not_ran=("ls_speculative", "ls_one_round", "ipm_iter_tail")),
    "ARMOUR_RESTO_INLINE=0": dict(ran=("resto_after_loop",), not_ran=("resto_inline",)),
}


def test_loop_forms_are_bitwise_the_default():
    """the 48 survey worlds under the reference's configuration: plans, constraints, iterations and
    evaluations of every loop form are bitwise the default loop's (the sigma search runs unchanged in the
    synchronised loop, the sync-free tail and the one-round tail)"""
    _, _, worlds, _ = worlds_of("survey_T20_O8")
    worlds = worlds[:48]
    P = planner("survey_T20_O8", 48, REF)
    ra, _ = P.plan(worlds)
    c = P.path_counts()
    v = variant_paths(REF)
    assert_paths(c, ran=v["ran"] + ("ipm_iter_sync", "ipm_iter_tail", "resto_inline", ("ls_one_round", "ls_speculative")),
                 not_ran=v["not_ran"] + ("ls_sequential",))
    assert c["qf_sigma"] == c["ipm_iter_sync"] + c["ipm_iter_tail"], c
    assert sum(r["status"] == 4 for r in ra) >= 8 and sum(r["evaluations"] - r["iterations"] > 1 for r in ra) > 0
    for setting, paths in LOOP_FORMS.items():
        with env(*setting.split("=")):
            Q = planner("survey_T20_O8", 48, REF)
        rb, _ = Q.plan(worlds)
        cq = Q.path_counts()
        assert_paths(cq, ran=v["ran"] + paths["ran"], not_ran=v["not_ran"] + paths.get("not_ran", ()))
        assert cq["qf_sigma"] == cq["ipm_iter_sync"] + cq["ipm_iter_tail"], (setting, cq)
        assert_bitwise(P, Q, ra, rb)
        Q.close()
    P.close()


# ---- 5. hygiene -----------------------------------------------------------------------------------
def test_replan_and_back_to_the_default():
    """a second plan of the same batch on one planner is bitwise the first; a planner set to the reference's
    configuration and back plans bitwise what a fresh default planner plans"""
    _, _, worlds, _ = worlds_of("boundary_small_T20_O6")
    P = planner("boundary_small_T20_O6", len(worlds))
    D = planner("boundary_small_T20_O6", len(worlds))
    assert P.solver_options() == dict(mu_strategy=1, qf_grid=16, lbfgs_history=0)
    rd, _ = D.plan(worlds)
    assert_paths(D.path_counts(), **DEFAULT_PATHS)
    P.set_solver_options(**options(REF))
    with taken(P) as d1:
        r1, _ = P.plan(worlds)
    g1 = [P.constraints(w) for w in range(len(worlds))]
    with taken(P) as d2:
        r2, _ = P.plan(worlds)
    assert_paths(d1, **variant_paths(REF))
    assert d1 == d2
    for w, (a, b) in enumerate(zip(r1, r2)):
        assert np.array_equal(a["k_opt"], b["k_opt"]) and a["cost"] == b["cost"] and a["iterations"] == b["iterations"], w
        assert np.array_equal(g1[w], P.constraints(w)), w
    assert any(not np.array_equal(a["k_opt"], b["k_opt"]) for a, b in zip(r1, rd))  # the options change plans
    P.set_solver_options(mu_strategy=1, lbfgs_history=0)
    with taken(P) as d3:
        r3, _ = P.plan(worlds)
    assert_paths(d3, **DEFAULT_PATHS)
    assert_bitwise(P, D, r3, rd)
    P.close()
    D.close()


def test_bad_options_and_episodes():
    """an out-of-range field is ARMOUR_E_ARG and names the field; a set during an episode is ARMOUR_E_STATE;
    a refused set leaves the options as they were"""
    _, _, worlds, _ = worlds_of("boundary_small_T20_O6")
    P = planner("boundary_small_T20_O6", 4, REF)
    for bad, field in ((dict(mu_strategy=4), "mu_strategy"), (dict(mu_strategy=-1), "mu_strategy"), (dict(qf_grid=1), "qf_grid"),
                       (dict(qf_grid=33), "qf_grid"), (dict(lbfgs_history=7), "lbfgs_history"), (dict(lbfgs_history=-1), "lbfgs_history")):
        with pytest.raises(A.ArmourError, match=f"error {A.ARMOUR_E_ARG}: .*{field}"):
            P.set_solver_options(**bad)
        assert P.solver_options() == options(REF)
    with pytest.raises(TypeError):
        P.set_solver_options(history=3)
    with pytest.raises(A.ArmourError, match="qf_grid"):
        A.Planner(T=20, max_obstacles=6, max_worlds=1, solver=dict(qf_grid=64))
    P.episode_begin(worlds[:4], np.array([w[3] for w in worlds[:4]]), check_samples=6)
    with pytest.raises(A.ArmourError, match=f"error {A.ARMOUR_E_STATE}: .*episode"):
        P.set_solver_options(mu_strategy=1)
    assert P.solver_options() == options(REF)
    P.episode_step()  # the episode plans under the configuration it began with
    assert_paths(P.path_counts(), **variant_paths(REF))
    P.plan(worlds[:4])  # a plan entry ends the episode
    P.set_solver_options(mu_strategy=1, lbfgs_history=0)
    assert P.solver_options() == dict(mu_strategy=1, qf_grid=16, lbfgs_history=0)
    P.close()


def test_evaluations_after_a_plan_are_those_after_a_reach():
    """armour_eval_candidates and armour_eval_constraints after a plan under the reference's configuration
    are bitwise those after a reach alone (the sigma search borrows dslo / dshi only)"""
    _, _, worlds, _ = worlds_of("boundary_small_T20_O6")
    W = len(worlds)
    x = np.random.default_rng(5).uniform(-1, 1, (W, 9, 7))
    P = planner("boundary_small_T20_O6", W, REF)
    R = planner("boundary_small_T20_O6", W)
    P.plan(worlds)
    R.reach(worlds)
    assert_paths(P.path_counts(), **variant_paths(REF))
    assert_paths(R.path_counts(), not_ran=("solve_quality", "qf_sigma", "hess_lbfgs", "solve_adaptive"))
    a, b = P.eval_candidates(x), R.eval_candidates(x)
    for k in ("cost", "violation", "feasible", "best"):
        assert np.array_equal(a[k], b[k]), k
    for w in range(W):
        (ga, Ja), (gb, Jb) = P.eval_constraints(w, x[w, 0]), R.eval_constraints(w, x[w, 0])
        assert np.array_equal(ga, gb) and np.array_equal(Ja, Jb), w
    P.close()
    R.close()
