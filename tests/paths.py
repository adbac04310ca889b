"""The path census in tests (Planner.path_counts, armour_get_path_counts): which kernels and loop forms
the host chose. An A/B test that sets a path-selecting variable asserts with these that the variant's
path ran on the variant's planner and did not run on the other one; a comparison whose setting was not
honoured, or whose inputs never reach the path, then fails instead of comparing default with default.

The counters are cumulative since a planner was created, so for a planner the test created itself
P.path_counts() is already the difference over the test; taken(P) gives it over a part."""
import contextlib
import os

LANE = ("reach_lane_wide", "reach_lane_dense")
JOB = ("reach_job_256", "reach_job_128")
TRACK_ROW = ("track_row", "track_row_rec", "track_row_episode")
TRACK_SERIAL = ("track_serial", "track_serial_rec", "track_serial_episode")


@contextlib.contextmanager
def taken(P):
    """with taken(P) as d: ...; afterwards the dict d = path_counts() after the body minus before it"""
    before = P.path_counts()
    d = {}
    try:
        yield d
    finally:
        after = P.path_counts()
        d.update({k: after[k] - before[k] for k in after})


def _count(delta, name):
    # a name, or a tuple of names whose counts are summed ("any of these")
    names = (name,) if isinstance(name, str) else tuple(name)
    for n in names:
        assert n in delta, f"unknown path counter {n!r}; the library has {sorted(delta)}"
    return sum(delta[n] for n in names)


def assert_paths(delta, ran=(), not_ran=(), exactly=None):
    """every entry of `ran` counted above zero and every entry of `not_ran` zero in `delta` (path_counts()
    of a fresh planner, or taken()'s difference); an entry is a counter's name or a tuple of names (their
    sum); exactly: {entry: count}. The failure message prints the whole delta."""
    nonzero = {k: v for k, v in delta.items() if v}
    print("paths:", os.environ.get("PYTEST_CURRENT_TEST", ""), nonzero)
    bad = [f"{n} did not run" for n in ran if _count(delta, n) <= 0]
    bad += [f"{n} ran {_count(delta, n)} times" for n in not_ran if _count(delta, n) != 0]
    bad += [f"{n} ran {_count(delta, n)} times, not {c}" for n, c in (exactly or {}).items() if _count(delta, n) != c]
    assert not bad, "; ".join(bad) + f"\npath counts (non-zero): {nonzero}"


def engine_paths(name):
    """assert_paths' arguments for a planner created under conftest.engine(name) after a reach"""
    if name == "lane":
        return dict(ran=(LANE,), not_ran=JOB)
    if name == "job":
        return dict(ran=(JOB,), not_ran=LANE)
    if name == "narrow":
        return dict(ran=("reach_job_128",), not_ran=LANE + ("reach_job_256",))
    assert name is None, name
    return dict(ran=((LANE + JOB),), not_ran=())
