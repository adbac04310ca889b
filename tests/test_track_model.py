"""Properties of tests/track_model.py, the yardstick of the armour_track tests, on the Kinova tables of
tests/golden/robot_kinova_urdf.json, one random start, window [0, 0.5], 50 steps. They keep the
yardstick honest: a model that did not integrate to fourth order, or whose robust term never acted or
always acted, would fail here. Measured with this file (the figures are printed):

  nominal parameters, zero err0   largest position error 2.0e-9 at 50 steps, 1.2e-10 at 100: ratio 16.07
  every link at 1 +- 0.03         max V 3.0e-3 < V_m = 1e-2, max |e| 2.4e-3 < qe = 1.25e-2, lambda 0
  the same, |err0| = 0.6 qe       lambda 0.46 / 0.15 > 0, max V 8.4e-3 / 7.4e-3 < V_m
  every link at 1.2               max V 2.8e-2 > V_m: the check is sensitive

and the admission condition of the case list (tests/track_cases.py) on one perturbation draw.
"""
import numpy as np
import pytest

import robot_variants as RV
import track_cases as TC
import track_model as TM


@pytest.fixture(scope="module")
def runs():
    tb = RV.kinova_urdf()
    nj = int(tb["num_joints"])
    qe = TC.qe_of(tb)
    traj = TC.trajectories(1, 100)
    d = np.random.default_rng(300).normal(size=7)
    d /= np.linalg.norm(d)
    kinds = [(1.0, 0.0), (1.03, 0.0), (0.97, 0.0), (1.03, 1.0), (0.97, 1.0), (1.2, 0.0)]
    scale = np.array([np.full((2, nj), s) for s, _ in kinds])
    err0 = np.zeros((len(kinds), 2, 7))
    for i, (_, e) in enumerate(kinds):
        err0[i, 0] = e * 0.6 * qe * d
    R = TM.Rollouts(tb, np.repeat(traj, len(kinds), axis=0), scale, err0)
    return tb, qe, R.run(0.0, 0.5, 50), R.run(0.0, 0.5, 100)


def test_nominal_error_is_truncation_of_a_fourth_order_scheme(runs):
    tb, qe, o50, o100 = runs
    e50, e100 = o50["max_pos_err"][0].max(), o100["max_pos_err"][0].max()
    print(f"nominal: max |e| {e50:.3e} at 50 steps, {e100:.3e} at 100, ratio {e50 / e100:.2f}")
    assert e50 < 1e-6 and 12 <= e50 / e100 <= 20
    assert o50["max_robust"][0] == 0 and not o50["status"].any() and not o100["status"].any()


def test_inside_the_stated_uncertainty_the_bound_holds_without_the_robust_term(runs):
    tb, qe, o50, _ = runs
    for i in (1, 2):
        print(f"scale {(1.03, 0.97)[i - 1]}: max V {o50['max_V'][i]:.3e}, max |e| {o50['max_pos_err'][i].max():.3e}, "
              f"lambda {o50['max_robust'][i]:.3e}")
        assert o50["max_V"][i] < tb["V_m"]
        assert o50["max_pos_err"][i].max() < qe
        assert o50["max_robust"][i] == 0


def test_a_start_off_the_trajectory_wakes_the_robust_term(runs):
    tb, qe, o50, _ = runs
    for i in (3, 4):
        print(f"err0 0.6 qe, scale {(1.03, 0.97)[i - 3]}: lambda {o50['max_robust'][i]:.3e}, max V {o50['max_V'][i]:.3e}")
        assert o50["max_robust"][i] > 0
        assert o50["max_V"][i] < tb["V_m"]


def test_outside_the_stated_uncertainty_the_bound_fails(runs):
    tb, qe, o50, _ = runs
    print(f"scale 1.2: max V {o50['max_V'][5]:.3e}")
    assert o50["max_V"][5] > tb["V_m"]


@pytest.mark.parametrize("robot", TC.ROBOTS)
def test_listed_cases_meet_the_admission_condition(robot):
    w = TC.measure_spread(draws=1, robots=(robot,), windows=TC.WINDOWS[:1])
    for k, v in w.items():
        assert v < TC.ADMISSION, (robot, k, v)
    assert all(TC.TOL[k] == 100 * TC.SPREAD[k] and 0 < TC.SPREAD[k] < TC.ADMISSION for k in TC.FIELDS)
