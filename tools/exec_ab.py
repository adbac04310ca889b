"""Bitwise A/B of the execution layer between two library builds (development tool, in the style of
tools/plan_ab.py): one child process per library (the in-tree one, and another loaded through ARMOUR_LIB),
every output array saved and compared with np.array_equal. Each child runs

  check_motion      a mixed batch of 6 worlds with 0, 40, 1, 7, 40 and 0 obstacles (T = 10), three
                    trajectories per world, 1, 11 and 130 samples;
  track             every (robot, shape, window) of tests/track_cases.py, with ARMOUR_TRACK_KERNEL unset and
                    "serial";
  track_motion      every (robot, shape) of tests/tracked_cases.py on [0, 0.5] with 2, 11 and 51 check points,
                    the long record (65 and 129 check points) and the flag cases, both kernels;
  episodes          saved worlds 0-3 at T = 20, an untracked and a tracked episode (3 samples, 50 steps) of 5
                    steps with world 1's plan vetoed at steps 2 and 3: the states, the results and the tracked
                    records after every step, both kernels for the tracked one;
  eval_candidates   40 candidates per world on the planned batch of the episodes' worlds.

usage: python tools/exec_ab.py <path of the other library>"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("armour-dev_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, d))


def child(out):
    import armour_amd as A
    import track_cases as TC
    import tracked_cases as KC
    from test_episode_model import saved

    rec = {}

    def keep(tag, d):
        for k, v in d.items():
            if isinstance(v, np.ndarray):
                rec[f"{tag}/{k}"] = v

    def kernels():
        for name in (None, "serial"):
            os.environ.pop("ARMOUR_TRACK_KERNEL", None)
            if name:
                os.environ["ARMOUR_TRACK_KERNEL"] = name
            yield name or "row"
        os.environ.pop("ARMOUR_TRACK_KERNEL", None)

    # check_motion
    counts = (0, 40, 1, 7, 40, 0)
    worlds = [A.make_world(100 + i, n) for i, n in enumerate(counts)]
    P = A.Planner(T=10, max_obstacles=40, max_worlds=len(worlds))
    P.reach_mixed(worlds)
    rng = np.random.default_rng(1)
    for draw in range(3):
        traj = np.array([np.stack([w[0], rng.uniform(-0.5, 0.5, 7), rng.uniform(-1, 1, 7), rng.uniform(-1, 1, 7)]) for w in worlds])
        for samples in (1, 11, 130):
            clear, where = P.check_motion(traj, 0.0, 1.0, samples)
            keep(f"check_motion/{draw}/{samples}", dict(clearance=clear, where=where))
    P.close()

    # track
    for robot in TC.ROBOTS:
        P = A.Planner(T=10, max_obstacles=1, max_worlds=1, robot=None if robot == "kinova" else TC.tables(robot))
        for shape in TC.SHAPES:
            _, traj, scale, err0 = TC.case_inputs(robot, shape)
            for t0, t1 in TC.WINDOWS:
                for kern in kernels():
                    keep(f"track/{robot}/{shape}/{t0}/{kern}", P.track(traj, scale, err0, t0, t1, TC.STEPS))
        P.close()

    # track_motion
    def tracked(tag, tables, traj, scale, err0, obs, window, steps, checks):
        P = A.Planner(T=10, max_obstacles=3, max_worlds=len(obs), robot=tables)
        P.reach_mixed(KC.worlds(traj, obs))
        for C in checks:
            for kern in kernels():
                keep(f"track_motion/{tag}/{C}/{kern}", P.track_motion(traj, scale, err0, window[0], window[1], steps, C))
        P.close()

    for robot in KC.ROBOTS:
        for shape in KC.SHAPES:
            tb, traj, scale, err0, obs = KC.case_inputs(robot, shape)
            tracked(f"{robot}/{shape}", None if robot == "kinova" else tb, traj, scale, err0, obs, (0.0, 0.5), KC.STEPS, KC.CHECKS)
    tb, traj, scale, err0, obs = KC.long_inputs()
    tracked("long", None, traj, scale, err0, obs, KC.LONG_WINDOW, KC.LONG_STEPS, KC.LONG_CHECKS)
    for name in KC.FLAG_CASES:
        c = KC.flag_case(name)
        tracked(f"flag/{name}", c["tables"] if name == "input" else None, c["traj"], c["scale"], c["err0"], c["obstacles"],
                c["window"], KC.STEPS, (c["C"],))

    # episodes
    pairs = [saved(i) for i in range(4)]
    worlds, goals = [p[0] for p in pairs], np.array([p[1] for p in pairs])
    O = max(len(w[4]) for w in worlds)
    scale = A.uncertainty_samples(TC.tables("kinova"), 3)
    runs = [("untracked", False, "row")] + [("tracked", True, kern) for kern in kernels()]
    for name, track, kern in runs:
        if kern == "serial":
            os.environ["ARMOUR_TRACK_KERNEL"] = "serial"
        P = A.Planner(T=20, max_obstacles=O, max_worlds=4)
        keep(f"episode/{name}/{kern}/begin", P.episode_begin(worlds, goals, check_samples=11))
        if track:
            P.episode_track(scale=scale, steps=50)
        for step in range(5):
            reject = np.zeros(4, dtype=int)
            reject[1] = step in (2, 3)
            _, res, _ = P.episode_step(reject)
            tag = f"episode/{name}/{kern}/{step}"
            keep(tag, P.episode_states())
            keep(tag + "/res", dict(k_opt=np.array([r["k_opt"] for r in res]), cost=np.array([r["cost"] for r in res]),
                                    feasible=np.array([r["feasible"] for r in res]), it=np.array([r["iterations"] for r in res])))
            if track:
                keep(tag + "/tracked", P.episode_tracked())
        P.close()
        os.environ.pop("ARMOUR_TRACK_KERNEL", None)

    # eval_candidates
    P = A.Planner(T=20, max_obstacles=O, max_worlds=4)
    P.plan_mixed(worlds)
    keep("eval_candidates", P.eval_candidates(np.random.default_rng(2).uniform(-1.0, 1.0, (4, 40, 7))))
    P.close()
    np.savez(out, **rec)


if __name__ == "__main__":
    if sys.argv[1] == "--child":
        child(sys.argv[2])
        sys.exit(0)
    OUT = tempfile.mkdtemp(prefix="exec_ab_")  # the children's arrays; the verdict is what is printed
    outs = []
    for name, lib in (("tree", None), ("other", os.path.abspath(sys.argv[1]))):
        env = dict(os.environ)
        env.pop("ARMOUR_LIB", None)
        if lib:
            env["ARMOUR_LIB"] = lib
        o = os.path.join(OUT, f"exec_ab_{name}.npz")
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", o], check=True, env=env)
        outs.append(dict(np.load(o)))
    a, b = outs
    assert sorted(a) == sorted(b)
    # (array_equal with equal_nan: a failed world's cost; timings are floats, not arrays, and are not kept)
    bad = [k for k in sorted(a) if a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k], equal_nan=a[k].dtype.kind == "f")]
    groups = {}
    for k in a:
        groups[k.split("/")[0]] = groups.get(k.split("/")[0], 0) + 1
    print("arrays compared: " + ", ".join(f"{g} {n}" for g, n in sorted(groups.items())) + f"; {sum(v.size for v in a.values())} values")
    print("arrays differing: " + (", ".join(bad) if bad else "none"))
    sys.exit(1 if bad else 0)
