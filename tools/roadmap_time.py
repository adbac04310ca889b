"""What the roadmap high-level planner costs at the bench's planner size (profiles/roadmap_time.txt):
1308 survey worlds at rest, O = 20, T = 100, nodes from armour_amd.roadmap_nodes (spread 0.5), N = 512 and 1023.

  * armour_episode_step without a roadmap (the yardstick) and with one: the waypoint's share of a step, from
    episode_ms[1] (choose + advance + waypoint kernels, HIP events on the planner's stream);
  * armour_roadmap_build three times: build_ms per pass (HIP events) and the wall time;
  * the edge-sample pass in (sample, link, obstacle) tests per second against armour_check_motion on the same
    number of tests (the block-per-sample shape; wall time of the call, best of three).

    python tools/roadmap_time.py [output file]
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "armour-dev_amd")]
import armour_amd as A  # noqa: E402
from armour_amd import robot_tables as RT  # noqa: E402

out = open(sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "roadmap_time.txt"), "w")


def say(*a):
    s = " ".join(str(x) for x in a)
    print(s, flush=True)
    out.write(s + "\n"); out.flush()

W, O, T = 1308, 20, 100
robot = RT._shaped(RT.builtin(0))
rng = np.random.default_rng(0)
t = time.time()
worlds = [A.make_world(i, O, profile="survey") for i in range(W)]
z = np.zeros(7)
worlds = [(w[0], z, z, w[3], w[4]) for w in worlds]   # at rest
q0 = np.array([w[0] for w in worlds])
off = rng.standard_normal((W, 7))
goals = q0 + 1.5 * off / np.linalg.norm(off, axis=1, keepdims=True)
say(f"# {W} worlds, O = {O}, T = {T}; nodes: roadmap_nodes(spread 0.5); connect_radius 1.0, edge_step 0.05, margin 0.02 (worlds made in {time.time()-t:.0f}s)")
P = A.Planner(T=T, max_obstacles=O, max_worlds=W)
cfg = dict(connect_radius=1.0, edge_step=0.05, margin=0.02)

def steps(n):
    wall, ems = [], []
    for _ in range(n):
        t = time.perf_counter()
        running, res, tm = P.episode_step()
        wall.append((time.perf_counter() - t) * 1e3)
        ems.append((tm["check_ms"], tm["advance_ms"], tm["reach_ms"], tm["nlp_ms"]))
    return np.array(wall), np.array(ems)

P.episode_begin(worlds, goals)
wall, ems = steps(4)
say("episode_step without a roadmap: wall ms", np.round(wall, 1), "check/advance/reach/nlp ms (per step)", np.round(ems, 3).tolist())
base_adv = np.median(ems[1:, 1])
base_wall = np.median(wall[1:])
for N in (512, 1023):
    nodes = np.array([A.roadmap_nodes(robot, q0[w], goals[w], N, 0.5, rng) for w in range(W)])
    P.episode_begin(worlds, goals)
    t = time.perf_counter()
    P.episode_roadmap(nodes, **cfg)
    say(f"N = {N}: episode_roadmap (build + first waypoints) wall {(time.perf_counter()-t)*1e3:.1f} ms")
    wall, ems = steps(4)
    adv = np.median(ems[1:, 1])
    say(f"N = {N}: episode_step with the roadmap: wall ms", np.round(wall, 1), "advance ms (choose + advance + waypoint)", np.round(ems[:, 1], 3),
        f"-> waypoint {adv - base_adv:.3f} ms a step = {100 * (adv - base_adv) / base_wall:.2f} % of a step ({base_wall:.1f} ms)")
    fb = P.episode_roadmap_state()[0]
    say(f"N = {N}: entries found {int((fb >= 0).sum())} of {W}")
    # the build alone, on the planned batch (the episode's roadmap must be over first)
    P.plan_mixed(worlds)
    for rep in range(3):
        t = time.perf_counter()
        st = P.roadmap_build(nodes, goals, **cfg)
        wl = (time.perf_counter() - t) * 1e3
        say(f"N = {N}: roadmap_build rep {rep}: wall {wl:.1f} ms, build_ms [vertices, candidates, samples + fold, cost-to-go] {np.round(st['build_ms'], 3)}",
            {k: v for k, v in st.items() if k != "build_ms"})
    tests = st["edge_samples"] * 7 * O
    say(f"N = {N}: edge samples: {st['edge_samples']} samples x 7 links x {O} obstacles = {tests:.3e} tests in {st['build_ms'][2]:.3f} ms = {tests / st['build_ms'][2] / 1e6:.1f} G tests/s (lane per configuration)")
    S = min(65535, max(1, st["edge_samples"] // W))
    traj = np.zeros((W, 4, 7))
    traj[:, 0] = q0
    traj[:, 3] = 0.5
    best = 1e30
    for rep in range(3):
        t = time.perf_counter()
        P.check_motion(traj, 0.0, 1.0, S)
        best = min(best, (time.perf_counter() - t) * 1e3)
    say(f"N = {N}: armour_check_motion, {S} samples x {W} worlds = {S * W * 7 * O:.3e} tests in {best:.3f} ms wall (best of 3) = {S * W * 7 * O / best / 1e6:.1f} G tests/s (block per sample)")
    del nodes
