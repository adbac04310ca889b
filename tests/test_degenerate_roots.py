"""The interior critical points of the desired trajectory on and next to the surface
6 T qd0 + T^2 qdd0 = 12 k, where the quadratic that gives them loses its leading coefficient (reach.h
q_roots / qd_roots / qdd_roots_k0 and their restatement in oracle/src/traj.cpp), against exact values
(tests/golden/degenerate_roots.npz, mpmath at 100 digits; tests/degenerate_roots.py). The oracle and the
device share the formula, so no parity test can see an error in it.

  * the JRS scalars of the host build (jrs_joint at k = 0) enclose the exact trajectory at its critical
    times, the interval's ends and its midpoint, with the inequality and slack of tests/jrs_unit.py;
  * the oracle's extremum rows of g are the exact minima and maxima over [0, 1] within
    16 * 2^-52 * S (S = max(1, sum |control points|), for the velocity max(1, 5 sum |control
    differences|) / D), and their Jacobian entries the envelope-theorem derivatives within 1e-9;
  * the cancellation guard of the fix fires at k = 0 for five joints of the committed plan fixtures, none
    near the surface: the census, and why the committed reach fixtures stay within their last bit.

Measured (host build and oracle, x86-64; the device build and the HIP rows give the same figures,
tests/test_gpu_degenerate_roots.py), with (p +- disc) / den as the reference writes it -> with the
cancelling root from the product of the roots:
  JRS excess over the enclosure: qd 1.88e-2 rad/s -> 5.1e-16 (0.03 of the slack), qdd 2.03e-2 rad/s^2 ->
    3.5e-15 (0.21); cos and sin stayed enclosed (the Taylor remainder absorbs the lost extremum). Misses
    before: 21 cases at delta = 0, 15 at +2^-50, 12 at -2^-50 (qd 1.33e-2), none after. Twelve of each
    delta's, delta = 1e-3 included, were the middle interval of T = 7, 4.96e-3 rad/s at khat = +-1: the
    slope of the desired velocity in k peaks at s = 1/2, inside that interval, and was bounded by its
    values at the ends (jrs_joint Part 2; the planners take even T only, where 1/2 is an end).
  row value error: 1.04e-1 at delta = 0 (the extremum is dropped), 2.5e-2 at +-2^-50, 4.4e-6 at +-2^-44,
    6.6e-11 at +-2^-36 -> 9.1e-16, 0.063 of the bar, everywhere.
  Jacobian error: 9.7e-2, 5.6e-2, 1.2e-3, 4.7e-6 at the same deltas and 1.8e-8 at +-2^-28 ->
    4.6e-12 (at delta = 2^-16, outside the guard, as before).
"""
import glob

import numpy as np
import pytest

import degenerate_roots as DR
import jrs_unit as U
from oracle import OraclePlanner


def test_fixture_is_what_the_generator_writes():
    """shapes, the case lists of the generator and what it promises of them"""
    fx = DR.fixture()
    n, m = 3 * 4 * 13 * 5, 4 * (13 + 5) + 2 + 1
    assert fx["start_cases"].shape == (n, 5) and fx["start_exact"].shape == (n, 6, 3, 6, 2)
    assert fx["row_cases"].shape == (m, 4) and fx["row_exact"].shape == (m, 2, 2, 3, 2)
    assert np.all(np.abs(fx["row_cases"][:, 3]) <= 1)
    assert fx["row_flags"].any(axis=(1, 2)).mean() <= 0.15
    # every start-state interval holds a critical time strictly inside
    sc, ts = fx["start_cases"], fx["start_times"]
    assert np.all(fx["start_ncrit"] >= 1)
    assert np.all(ts[:, 0] > sc[:, 4] / sc[:, 3]) and np.all(ts[:, 0] < (sc[:, 4] + 1) / sc[:, 3])
    import sys

    sys.path.insert(0, U.os.path.join(U.HERE, "golden"))
    import make_degenerate_roots as G

    np.testing.assert_array_equal(G.start_cases(), sc)
    np.testing.assert_array_equal(G.row_cases()[0], fx["row_cases"])


@pytest.fixture(scope="module")
def host_outputs():
    return DR.start_outputs(U.Lib(device=False))


def test_host_jrs_scalars_enclose_the_trajectory_on_the_surface(host_outputs):
    worst = DR.check_start_enclosure(host_outputs, print)
    d = DR.start_delta()
    for lo, hi in ((0, 2.0 ** -49), (2.0 ** -49, 2.0 ** -35), (2.0 ** -35, 1)):
        m = (d >= lo) & (d < hi)
        print(f"relative distance in [{lo:.1e}, {hi:.1e}): {int(m.sum())} cases, worst excess cos / sin / qd / qdd "
              f"{worst[m].max(axis=0)}")


def test_oracle_extremum_rows_on_the_surface():
    worlds, X, index = DR.row_worlds()
    misses, wv, wu, wj = [], 0.0, 0.0, 0.0
    for w, world in enumerate(worlds):
        R = OraclePlanner(*world, T=DR.T, threads=4)
        R.reach()
        g, J = R.eval(X[w])
        v, u, j, bad = DR.check_rows(g, J, index[w])
        wv, wu, wj = max(wv, v), max(wu, u), max(wj, j)
        misses += bad
    fin = lambda what: max([b[3] for b in misses if b[0] == what and np.isfinite(b[3])], default=0.0)
    print(f"oracle rows: worst |row - exact| {wv:.3e} ({wu:.3g} of its bar), worst Jacobian error {wj:.3e}; "
          f"misses {len(misses)} (worst finite value miss {fin('value'):.3e}, Jacobian {fin('jacobian'):.3e})")
    assert not misses, (len(misses), sorted({b[1] for b in misses}), misses[:8])


# ---- the guard at k = 0 on the committed start states ------------------------------------------------
def guard_k0(qd0, qdd0, D=1.0):
    """reach.h root_pair's condition |p - sign(p) disc| < 2^-16 |p + sign(p) disc| for q_roots, qd_roots
    and qdd_roots_k0 at k = 0, in the kernels' own order of operations: ([..., 3] bool, [..., 3] the other
    root |big / den|)"""
    a, b = np.asarray(qd0) * D, np.asarray(qdd0) * D * D
    with np.errstate(invalid="ignore", divide="ignore"):
        pdd = [(2 * a + b, np.sqrt(64 * a * a + 14 * a * b - 120 * 0.0 * a + b * b), 5 * (6 * a - 12 * 0.0 + b)),
               (18 * a - 30 * 0.0 + 4 * b, np.sqrt(6 * (150 * 0.0 * 0.0 - 180 * 0.0 * a - 20 * 0.0 * b + 54 * a * a + 14 * a * b + b * b)),
                10 * (6 * a - 12 * 0.0 + b)),
               (32 * a + 6 * b, np.sqrt(2 * (152 * a * a + 42 * a * b + 3 * b * b)), 10 * (6 * a + b))]
        fired, other = [], []
        for p, disc, den in pdd:
            hi, lo = p + disc, p - disc
            big, sm = np.where(p >= 0, hi, lo), np.where(p >= 0, lo, hi)
            fired.append(np.abs(sm) < 2.0 ** -16 * np.abs(big))
            other.append(np.abs(big / den))
    return np.stack(fired, axis=-1), np.stack(other, axis=-1)


def committed_start_states():
    """(name, qd0 [n, 7], qdd0 [n, 7]) of the plan fixtures: the bench step's worlds, the saved worlds and
    the boundary sets"""
    import armour_amd as A
    from test_bench_worlds import load_step
    from test_saved_worlds import saved_worlds

    fx = load_step()
    ws = [A.make_world(int(s), int(fx["O"]), profile="survey") for s in fx["seed"]]
    yield "bench step", np.array([w[1] for w in ws]), np.array([w[2] for w in ws])
    _, ws, _ = saved_worlds()
    yield "saved worlds", np.array([w[1] for w in ws]), np.array([w[2] for w in ws])
    for path in sorted(glob.glob(U.os.path.join(U.HERE, "golden", "boundary_*.npz"))):
        b = np.load(path)
        yield U.os.path.basename(path)[:-4], b["qd0"], b["qdd0"]


# (world, joint) of the bench step inside the guard of qd_roots at k = 0: |qdd0| below 2e-4 rad/s^2, the
# root T^2 qdd0 / big within 2^-16 of zero, the other root 0.6
BENCH_IN_GUARD = [(347, 3), (1363, 6), (1434, 2), (2784, 2), (3496, 3)]


def test_guard_census_of_the_committed_start_states():
    """Which committed start states the guard touches at k = 0 (the reach sets), and that none of them is
    near the surface. The guard also holds the far side of cancellation: a root next to 0 beside a root
    of order 1, which is T^2 qdd0 -> 0 for qd_roots. Five joints of the bench step's 27 468 are there, and
    nothing of the saved worlds (at rest: p = disc = 0, the guard's strict < does not fire) or the
    boundary sets. For those five the legacy root was off by at most 4 * 2^-52 * |big / den| <= 5.4e-16 in
    t, at a critical point, where the value moves with the square of that: the host build's JRS scalars
    of worlds 347 and 3496 differ from the parent's in the last bit of six doubles (1.1e-16), the other
    three worlds' and every other fixture's not at all."""
    f, other = guard_k0(0.25, -1.5)
    assert f.all() and not np.isfinite(other).any()            # the model sees the surface
    assert guard_k0(0.6, -3.6 * (1 + 2.0 ** -20))[0].all() and not guard_k0(0.6, -0.8)[0].any()
    total = 0
    for name, qd0, qdd0 in committed_start_states():
        fired, other = guard_k0(qd0, qdd0)
        total += qd0.size
        assert np.all(other[fired] <= 1.0), (name, np.argwhere(fired & (other > 1.0))[:5].tolist())
        want = BENCH_IN_GUARD if name == "bench step" else []
        assert [tuple(int(v) for v in r) for r in np.argwhere(fired)] == [(w, j, 1) for w, j in want], name
    assert total >= 7 * (3924 + 100 + 16)
    print(f"{total} start states, {len(BENCH_IN_GUARD)} inside the guard at k = 0, none with a root beyond 1")
