"""Candidate evaluation against the only older way to the same answers (run on the GPU).

One planner, 327 survey worlds (T = 100, O = 20), N = 256 candidates per world. Side A is one
Planner.eval_candidates call: cost, class violations, feasible and best of all W x N candidates.
Side B is what the library offered before: armour_eval_constraints evaluates every world of the batch
at one shared x and hands back one world's g, so N calls (one per candidate, jac skipped) plus the
host reduction of each returned g to the same three class maxima. That is B's lower bound: it yields
the answers of one world per candidate, W x N calls would be needed for all of them, and it cannot
take a different x per world at all. The planner is built and both sides are warmed up before any
timing; then the sides alternate for `repeats` rounds. Every call ends in a host wait for its
results, so the host clock around it is the call's time.

Printed: medians and ranges, candidates per second of side A, side A as a multiple of one
armour_eval_constraints call (one full-grid eval_kernel launch of the same batch plus that call's
host round trip; the launch alone is read from a kernel trace of this script, see
profiles/candidates_ab.txt), and the bytes cand_rows has to read if every block reads its inputs
once: the plane records once per chunk of 32 candidates (CAND_KC), not once per candidate (to be held against
the FETCH_SIZE counter of a run of its own).

usage: python tools/candidates_ab.py [repeats=7] [worlds=327] [candidates=256]"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "armour-dev_amd"))

import armour_amd as A  # noqa: E402

T, O, KC = 100, 20, 32
TV, CV = 1e-2, 1e-4


def halton(i, b):
    f, r = 1.0, 0.0
    while i > 0:
        f /= b
        r += f * (i % b)
        i //= b
    return r


def points(N):
    X = np.array([[(1.0, 0.5, 0.1)[n % 3] * (2.0 * halton(n, b) - 1.0) for b in (2, 3, 5, 7, 11, 13, 17)] for n in range(N)])
    X[0] = 0.0
    return X


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 7
    W = int(sys.argv[2]) if len(sys.argv) > 2 else 327
    N = int(sys.argv[3]) if len(sys.argv) > 3 else 256
    worlds = [A.make_world(s, O, profile="survey") for s in range(W)]
    P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
    P.reach(worlds)
    X = points(N)
    XW = np.ascontiguousarray(np.broadcast_to(X, (W, N, 7)))
    nt, nc = 7 * T, P.NJ * T * O
    jb = P.joint_bounds()
    tr = [P.torque_radius(w).reshape(-1) for w in range(W)]
    lim = np.tile(A.KINOVA.torque_limits, T)
    exL = np.concatenate([np.tile(jb[0:14:2], 2), np.tile(jb[14:28:2], 2)])
    exU = np.concatenate([np.tile(jb[1:14:2], 2), np.tile(jb[15:28:2], 2)])

    def side_a():
        t0 = time.perf_counter()
        out = P.eval_candidates(XW)
        return out, (time.perf_counter() - t0) * 1e3

    def side_b():
        viol = np.zeros((N, 3))
        calls = np.zeros(N)
        t0 = time.perf_counter()
        for n in range(N):
            w = n % W
            c0 = time.perf_counter()
            g = P.eval_constraints(w, X[n], jac=False)
            calls[n] = (time.perf_counter() - c0) * 1e3
            L, U = -lim + tr[w], lim - tr[w]
            viol[n, 0] = np.maximum(L - TV - g[:nt], g[:nt] - U - TV).max()
            viol[n, 1] = g[nt:nt + nc].max() - CV
            viol[n, 2] = np.maximum(exL - g[nt + nc:], g[nt + nc:] - exU).max()
        return viol, (time.perf_counter() - t0) * 1e3, calls

    out, _ = side_a()   # warm-up of both sides: code objects, first-use allocations, the plane cache
    vb, _, _ = side_b()
    pick = (np.arange(N) % W, np.arange(N))
    dv = np.abs(out["violation"][pick] - vb)
    ta, tb, tc = [], [], []
    for _ in range(repeats):
        ta.append(side_a()[1])
        _, t, calls = side_b()
        tb.append(t)
        tc.append(np.median(calls))
    ta, tb, tc = np.array(ta), np.array(tb), np.array(tc)
    st = P.plane_cache_stats()
    lk = tq = 0
    for w in range(W):
        a, b = P.monomial_counts(w)
        lk += int(a.sum())
        tq += int(b.sum())
    chunks = (N + KC - 1) // KC
    rec_b = st["planes_kept"] * 40 + st["pairs"] * 4            # records [5] doubles, pcoff words
    mono_b = lk * 26 + tq * 10                                   # hash + coefficients of the staged monomials
    print(f"{W} survey worlds, T={T}, O={O}, N={N} candidates per world ({W * N} candidates), {repeats} alternating rounds")
    print(f"agreement of the two sides at world n % W of candidate n: max |violation difference| "
          f"torque {dv[:, 0].max():.3e}, collision {dv[:, 1].max():.3e}, extremum {dv[:, 2].max():.3e}")
    print(f"feasible candidates: {int(out['feasible'].sum())} of {W * N}; worlds with a feasible candidate: "
          f"{int((out['best'] >= 0).sum())} of {W}")
    print("median [min, max], ms")
    print(f"  A  one eval_candidates call (all {W} worlds x {N}):              {np.median(ta):10.3f} [{ta.min():10.3f}, {ta.max():10.3f}]")
    print(f"  B  {N} armour_eval_constraints calls + host reduction (1 world/call): {np.median(tb):10.3f} [{tb.min():10.3f}, {tb.max():10.3f}]")
    print(f"     one such call (a full-grid evaluation of the batch + host round trip): {np.median(tc):8.3f} [{tc.min():8.3f}, {tc.max():8.3f}]")
    print("     A by round: " + " ".join(f"{v:.2f}" for v in ta))
    a, b, c = np.median(ta), np.median(tb), np.median(tc)
    print(f"  B / A = {b / a:.2f}x for B's {N} answers against A's {W * N}; spread of A {ta.max() - ta.min():.3f} ms, of B {tb.max() - tb.min():.3f} ms")
    print(f"  A: {W * N / (a * 1e-3):.3e} candidates/s; A = {a / c:.2f} x one armour_eval_constraints call, "
          f"which evaluates {W} candidates: {W * N / a / (W / c):.2f}x its candidates per second")
    print(f"plane cache: {st['planes_kept']} records over {st['pairs']} pairs ({st['planes_kept'] / st['pairs']:.2f} per pair)")
    print(f"bytes cand_rows reads if every block reads its inputs once ({chunks} chunks of {KC} per (world, t)):")
    print(f"  records {rec_b * chunks / 1e6:.1f} MB + monomials {mono_b * chunks / 1e6:.1f} MB per launch; "
          f"records per candidate {rec_b / W / KC / 1e3:.2f} kB (once per chunk) against {rec_b / W / 1e3:.2f} kB (once per candidate)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
