"""armour_eval_candidates on the GPU: N candidate parameters per world reduced on the device to the
cost, the largest excess per row class, finalize_solution's verdict and the per-world arg-min,
against the oracle's g at every candidate and against the library's own full evaluation.

Candidates (deterministic): point n of world w has coordinate i = s_n (2 halton(n + 97 w, base_i) - 1)
with bases 2, 3, 5, 7, 11, 13, 17 and s_n cycling through 1.0, 0.5, 0.1; point 0 is zero and the last
two points are all -1 and all +1 (the corners of the box the plane cache is certified for).

Tolerances: cost and violations within 1e-9 of the oracle's (the project's g tolerance: a class
maximum moves by at most its rows' error); feasible identical wherever the oracle's margin to every
threshold exceeds that 1e-9, and the tests assert that no candidate falls inside the margin."""
import contextlib
import ctypes
import os

import numpy as np
import pytest

import armour_amd as A
import boundary_worlds as B
from armour_amd.robots import KINOVA
from conftest import engine
from oracle import OraclePlanner
from paths import assert_paths, engine_paths
from test_boundary import load, world

pytestmark = pytest.mark.gpu
TOL = 1e-9
TV, CV = 1e-2, 1e-4   # torque / collision violation thresholds (KPR/Parameters.h:37-38)
COST_SCALE = 10.0     # COST_FUNCTION_OPTIMALITY_SCALE: armour_result.cost is the objective over it
KC = 32               # candidates per block of cand_rows (nlp_kernels.hip CAND_KC)
BASES = (2, 3, 5, 7, 11, 13, 17)


def halton(i, b):
    f, r = 1.0, 0.0
    while i > 0:
        f /= b
        r += f * (i % b)
        i //= b
    return r


def candidates(w, N):
    X = np.zeros((N, 7))
    for n in range(N):
        s = (1.0, 0.5, 0.1)[n % 3]
        X[n] = [s * (2.0 * halton(n + 97 * w, b) - 1.0) for b in BASES]
    X[0] = 0.0
    if N >= 3:
        X[N - 2] = -1.0
        X[N - 1] = 1.0
    return X


def oracle_candidates(R, X):
    """the oracle's cost, class excesses, verdict and margin at every row of X for one world"""
    T, NJ, O = R.T, R.NJ, R.O
    nt, nc = 7 * T, NJ * T * O
    gl, gu = R.bounds()
    N = len(X)
    cost, viol, feas = np.zeros(N), np.zeros((N, 3)), np.zeros(N, dtype=bool)
    for n, x in enumerate(X):
        g = R.eval(x, jac=False)
        cost[n] = R.cost(x)[0] / COST_SCALE
        viol[n, 0] = np.maximum(gl[:nt] - TV - g[:nt], g[:nt] - gu[:nt] - TV).max()
        viol[n, 1] = (g[nt:nt + nc] - CV).max() if nc else -np.inf
        viol[n, 2] = np.maximum(gl[nt + nc:] - g[nt + nc:], g[nt + nc:] - gu[nt + nc:]).max()
        feas[n] = R.feasible(g)
        assert feas[n] == bool((viol[n] <= 0).all()), (n, viol[n])   # the three classes are the whole re-check
    margin = np.abs(viol).min(axis=1)   # distance of the nearest class maximum from its threshold
    return dict(cost=cost, violation=viol, feasible=feas, margin=margin)


def check_against_oracle(out, w, ref, tag=""):
    """one world's outputs against oracle_candidates; returns the smallest margin"""
    np.testing.assert_allclose(out["cost"][w], ref["cost"], rtol=0, atol=TOL, err_msg=f"{tag} cost w={w}")
    fin = np.isfinite(ref["violation"])
    np.testing.assert_array_equal(out["violation"][w][~fin], ref["violation"][~fin])
    np.testing.assert_allclose(out["violation"][w][fin], ref["violation"][fin], rtol=0, atol=TOL,
                               err_msg=f"{tag} violation w={w}")
    assert (ref["margin"] > TOL).all(), (tag, w, "a candidate within 1e-9 of a threshold", ref["margin"].min())
    np.testing.assert_array_equal(out["feasible"][w], ref["feasible"], err_msg=f"{tag} feasible w={w}")
    check_best(out, w, ref)
    return ref["margin"].min()


def own_best(cost, feas):
    idx = np.flatnonzero(feas)
    return int(idx[np.argmin(cost[idx])]) if len(idx) else -1   # argmin: the first of equal minima


def check_best(out, w, ref=None):
    assert out["best"][w] == own_best(out["cost"][w], out["feasible"][w]), w
    if ref is not None:
        fc = np.sort(ref["cost"][ref["feasible"]])
        if len(fc) == 0:
            assert out["best"][w] == -1
        elif len(fc) == 1 or fc[1] - fc[0] > TOL:
            assert out["best"][w] == own_best(ref["cost"], ref["feasible"]), w


def assert_same(a, b, sel_a=slice(None), sel_b=slice(None), tag=""):
    """bitwise equality of cost / violation / feasible of candidates sel_a of a and sel_b of b"""
    for k in ("cost", "violation", "feasible"):
        x, y = a[k][:, sel_a], b[k][:, sel_b]
        assert x.tobytes() == y.tobytes(), (tag, k, np.argwhere(x != y)[:4])


@contextlib.contextmanager
def env(name, value):
    prev = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if prev is None:
            os.environ.pop(name, None)
        else:
            os.environ[name] = prev


N1 = 64


@pytest.fixture(scope="module")
def small():
    """boundary_small_T20_O6 after reach() only, its oracles and the oracle's answers at the N1
    candidates of every world (computed once, shared and left unchanged)"""
    fx = load("boundary_small_T20_O6")
    T, W, O = int(fx["T"]), len(fx["kinds"]), fx["obstacles"].shape[1]
    assert (T, W, O) == (20, 12, 6)
    worlds = [world(fx, w) for w in range(W)]
    X = np.stack([candidates(w, N1) for w in range(W)])
    refs, oracles = [], []
    for w in range(W):
        R = OraclePlanner(*worlds[w], T=T, threads=8)
        R.reach()
        oracles.append(R)
        refs.append(oracle_candidates(R, X[w]))
    P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    P.reach(worlds)
    out = P.eval_candidates(X)
    yield dict(fx=fx, T=T, W=W, O=O, worlds=worlds, X=X, refs=refs, oracles=oracles, P=P, out=out)
    P.close()


def test_oracle_parity_at_the_decision_boundary(small):
    refs, out, W = small["refs"], small["out"], small["W"]
    counts = [int(r["feasible"].sum()) for r in refs]
    print("oracle feasible candidates per world:", counts)
    assert sum(0 < c < N1 for c in counts) >= 3 and sum(c == 0 for c in counts) >= 1
    assert out["cost"].shape == (W, N1) and out["violation"].shape == (W, N1, 3)
    assert out["feasible"].shape == (W, N1) and out["best"].shape == (W,)
    margin = min(check_against_oracle(out, w, refs[w], "small") for w in range(W))
    print(f"smallest oracle margin to a threshold over {W * N1} candidates: {margin:.3e}")
    for k in range(3):
        err = np.abs(out["violation"][..., k] - np.stack([r["violation"][:, k] for r in refs]))
        print(f"violation[{k}] largest error {np.nanmax(err):.3e}")


def test_same_value_path_as_the_evaluation(small):
    """every class maximum is bitwise the one formed, in the kernels' own order, from the g of
    armour_eval_constraints: collision max(g) - cv; torque max((Lb - tv) - v, (v - Ub) - tv) with
    Lb = -limit + radius, Ub = limit - radius; extremum max(L - v, v - U) over the last 28 rows
    (minima and maxima of the 7 positions, then of the 7 velocities) against joint_bounds()"""
    T, W, O, worlds = small["T"], small["W"], small["O"], small["worlds"]
    X = candidates(0, 18)   # the same points for every world: [N, 7]
    P = A.Planner(T=T, max_obstacles=O, max_worlds=W)   # a planner of its own: that call resets plan state
    P.reach(worlds)
    out = P.eval_candidates(X)
    cs = B.collision_slice(T, P.NJ, O)
    lim = KINOVA.torque_limits
    jb = P.joint_bounds()   # per joint [L, U] of its position rows, then of its velocity rows
    Lx = np.concatenate([jb[0:14:2], jb[0:14:2], jb[14:28:2], jb[14:28:2]])
    Ux = np.concatenate([jb[1:14:2], jb[1:14:2], jb[15:28:2], jb[15:28:2]])
    want = np.zeros((W, len(X), 3))
    for w in range(W):
        tr = P.torque_radius(w)   # [T, 7]
        Lb, Ub = -lim + tr, lim - tr
        for n, x in enumerate(X):
            g = P.eval_constraints(w, x, jac=False)
            v = g[:7 * T].reshape(T, 7)
            want[w, n, 0] = np.maximum((Lb - TV) - v, (v - Ub) - TV).max()
            want[w, n, 1] = g[cs].max() - CV
            want[w, n, 2] = np.maximum(Lx - g[-28:], g[-28:] - Ux).max()
    assert out["violation"][..., 1].tobytes() == want[..., 1].tobytes()
    assert out["violation"][..., 0].tobytes() == want[..., 0].tobytes()
    assert out["violation"][..., 2].tobytes() == want[..., 2].tobytes()
    P.close()


def test_independent_of_n_chunking_and_position(small):
    P, X, out, W = small["P"], small["X"], small["out"], small["W"]
    for n in range(N1):
        assert_same(P.eval_candidates(X[:, n:n + 1]), out, slice(None), slice(n, n + 1), f"N=1 n={n}")
    for k in (KC, KC + 1):
        for a in list(range(0, N1 - k, k)) + [N1 - k]:
            assert_same(P.eval_candidates(X[:, a:a + k]), out, slice(None), slice(a, a + k), f"N={k} at {a}")
    rev = P.eval_candidates(X[:, ::-1])
    assert_same(rev, out, slice(None), slice(None, None, -1), "reversed")
    for w in range(W):
        check_best(rev, w)


def test_mixed_batch(small):
    T, worlds = small["T"], small["worlds"]
    counts = [0, 3, 6, 6, 1]
    N = 17
    mixed = [w[:4] + (w[4][:c],) for w, c in zip(worlds, counts)]
    X = np.stack([candidates(w, N) for w in range(len(counts))])
    P = A.Planner(T=T, max_obstacles=6, max_worlds=len(counts))
    P.reach_mixed(mixed)
    out = P.eval_candidates(X)
    for w, c in enumerate(counts):
        R = OraclePlanner(*mixed[w], T=T, threads=8)
        R.reach()
        check_against_oracle(out, w, oracle_candidates(R, X[w]), "mixed")
    # no obstacles: no collision rows; the verdict is the torque and extremum rows'
    assert (out["violation"][0, :, 1] == -np.inf).all()
    np.testing.assert_array_equal(out["feasible"][0], (out["violation"][0][:, [0, 2]] <= 0).all(axis=1))
    P.close()
    # bitwise the uniform batches of each count
    for c in sorted(set(counts)):
        idx = [i for i, k in enumerate(counts) if k == c]
        Q = A.Planner(T=T, max_obstacles=c, max_worlds=len(idx))
        Q.reach([mixed[i] for i in idx])
        uni = Q.eval_candidates(X[idx])
        for k in ("cost", "violation", "feasible", "best"):
            assert uni[k].tobytes() == out[k][idx].tobytes(), (c, k)
        Q.close()


def test_full_size_and_both_variants():
    T, O, N = 100, 20, 33
    w0 = A.make_world(3, O, profile="survey")
    X = candidates(0, N)[None]
    R = OraclePlanner(*w0, T=T, threads=8)
    R.reach()
    ref = oracle_candidates(R, X[0])
    outs = []
    for full in ("0", "1"):
        with env("ARMOUR_EVAL_FULL", full):
            P = A.Planner(T=T, max_obstacles=O, max_worlds=1)
        P.reach([w0])
        outs.append(P.eval_candidates(X))
        # 33 candidates: two chunks of 32, on the small kernels unless ARMOUR_EVAL_FULL asks for the full ones
        mine, other = ("cand_small", "cand_full") if full == "0" else ("cand_full", "cand_small")
        assert_paths(P.path_counts(), exactly={mine: 1, other: 0, "cand_chunks": 2, "pc_builds": 1})
        P.close()
        check_against_oracle(outs[-1], 0, ref, f"full={full}")
    for k in ("cost", "violation", "feasible", "best"):
        assert outs[0][k].tobytes() == outs[1][k].tobytes(), k


def test_fetch_links():
    """the Fetch arm's tables (8 joints: more links than the Kinova's 7)"""
    fx = load("boundary_fetch_T100_O20")
    _, rstruct, tables = B.robot_of("fetch")
    T, N = 20, 8
    worlds = [world(fx, w) for w in range(2)]
    O = fx["obstacles"].shape[1]
    X = np.stack([candidates(w, N) for w in range(2)])
    with engine("lane"):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=2, robot=tables)
    P.reach(worlds)
    assert P.NJ > 7
    out = P.eval_candidates(X)
    assert_paths(P.path_counts(), ran=(("cand_small", "cand_full"),) + engine_paths("lane")["ran"],
                 not_ran=engine_paths("lane")["not_ran"])
    for w in range(2):
        R = OraclePlanner(*worlds[w], T=T, threads=8, robot=rstruct)
        R.reach()
        check_against_oracle(out, w, oracle_candidates(R, X[w]), "fetch")
    P.close()


def test_no_disturbance(small):
    T, W, O, worlds = small["T"], small["W"], small["O"], small["worlds"]
    P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    res, _ = P.plan(worlds)
    assert all(r["error"] == 0 for r in res)
    before = [(P.constraints(w), P.link_centers(w), P.torque_radius(w), P.link_generators(w)) for w in range(W)]
    X = np.stack([candidates(w, 5) for w in range(W)])
    X[:, 0] = [r["k_opt"] for r in res]
    out = P.eval_candidates(X)
    np.testing.assert_array_equal(out["feasible"][:, 0], [r["feasible"] for r in res])
    cost = np.array([r["cost"] for r in res])
    np.testing.assert_allclose(out["cost"][:, 0], cost, rtol=0, atol=1e-12)
    print("cost at k_opt bitwise the plan's:", out["cost"][:, 0].tobytes() == cost.tobytes())
    for w in range(W):
        after = (P.constraints(w), P.link_centers(w), P.torque_radius(w), P.link_generators(w))
        for a, b in zip(before[w], after):
            assert a.tobytes() == b.tobytes(), w
    res2, _ = P.plan(worlds)
    for a, b in zip(res, res2):
        assert a["k_opt"].tobytes() == b["k_opt"].tobytes()
        assert all(a[k] == b[k] for k in ("feasible", "status", "iterations", "evaluations", "cost", "kkt", "error"))
    P.close()


def _raw(P, N, x, W):
    ip = ctypes.POINTER(ctypes.c_int)
    cost, best = np.zeros((W, max(N, 1))), np.zeros(W, dtype=np.int32)
    xp = A._ptr(np.ascontiguousarray(x)) if x is not None else None
    return A.lib().armour_eval_candidates(P.h, N, xp, A._ptr(cost), None, None, best.ctypes.data_as(ip))


def test_errors(small):
    T, W, O, worlds = small["T"], small["W"], small["O"], small["worlds"]
    X = small["X"][:, :4].copy()
    P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    assert _raw(P, 4, X, W) == A.ARMOUR_E_STATE          # before any batch
    P.reach(worlds)
    assert A.lib().armour_eval_candidates(None, 4, A._ptr(X), None, None, None, None) == A.ARMOUR_E_ARG
    assert _raw(P, 4, None, W) == A.ARMOUR_E_ARG
    assert _raw(P, 0, X, W) == A.ARMOUR_E_ARG
    for bad in (np.nan, np.inf, 1.0 + 1e-12, -1.5):
        Y = X.copy()
        Y[W - 1, 3, 6] = bad
        assert _raw(P, 4, Y, W) == A.ARMOUR_E_ARG, bad
    assert _raw(P, 4, X, W) == 0                          # every output optional
    P.close()
    with env("ARMOUR_EVAL_F32", "1"):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    P.reach(worlds)
    assert _raw(P, 4, X, W) == A.ARMOUR_E_ARG
    P.close()
    P = A.ArmtdPlanner(T=T, max_obstacles=O, max_worlds=W)
    assert _raw(P, 4, X, W) == A.ARMOUR_E_ARG
    P.close()
    with env("ARMOUR_PLANE_CACHE", "0"):
        P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    P.reach(worlds)
    assert _raw(P, 4, X, W) == A.ARMOUR_E_STATE
    with pytest.raises(A.ArmourError, match="plane cache is unavailable"):
        P.eval_candidates(X)
    assert_paths(P.path_counts(), not_ran=("pc_builds", "cand_small", "cand_full", "cand_chunks"))  # refused before any launch
    # without obstacles there is nothing to cache: the call works
    free = [w[:4] + (w[4][:0],) for w in worlds[:2]]
    P.reach(free)
    assert (P.eval_candidates(X[:2])["violation"][..., 1] == -np.inf).all()
    P.close()


def test_world_with_a_reach_error():
    """arenas shrunk as test_gpu_capacity.py shrinks them: the heavy world still overflows after the
    retry; it reports NaN / 0 / -1 and the other worlds are bitwise a clean batch's"""
    from test_gpu_capacity import _planner, debug_world, rest_world

    T, O, N = 64, 8, 5
    worlds = [rest_world(O), debug_world(O), rest_world(O)]
    X = np.stack([candidates(w, N) for w in range(3)])
    P = _planner(T, O, 3)
    P.reach(worlds)
    clean = P.eval_candidates(X)
    use = []
    for w in worlds[:2]:
        P.reach([w])
        use.append(P.occupancy()["arena_rows"][0])
    P.close()
    light, heavy = use
    c = (light + heavy) // 8
    assert 4 * c >= light and 4 * c < heavy
    P = _planner(T, O, 3, ccap=c)
    P.reach(worlds)
    assert P.occupancy()["worlds_failed"][0] == 1
    out = P.eval_candidates(X)
    assert np.isnan(out["cost"][1]).all() and np.isnan(out["violation"][1]).all()
    assert not out["feasible"][1].any() and out["best"][1] == -1
    for w in (0, 2):
        for k in ("cost", "violation", "feasible", "best"):
            assert out[k][w].tobytes() == clean[k][w].tobytes(), (w, k)
    P.close()
