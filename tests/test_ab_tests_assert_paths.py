"""Every GPU test that sets a path-selecting setting also asserts, from the library's path census
(tests/paths.py assert_paths), which paths ran: a setting does not decide alone (batch size, capacities,
the plane cache and the CU count do too), so an A/B comparison that asserts no path can turn into
default against default and still pass.

The tests are found by their syntax tree: a test function of tests/test_gpu_*.py that names one of the
variables below (as a string constant or a keyword argument, its decorators included) or calls
conftest.engine, in its own body, in a fixture it takes, or in a helper or class it uses from its own
file or from another module of tests/. Each such test must reach a call of assert_paths the same way.
A new path-selecting setting is added to SETTINGS here."""
import ast
import glob
import os

HERE = os.path.dirname(os.path.abspath(__file__))

# the settings that choose between kernels or loop forms with the same results
SETTINGS = {
    "ARMOUR_NO_SPEC", "ARMOUR_RESTO_ROUNDS", "ARMOUR_RESTO_INLINE", "ARMOUR_RESTO_CONCURRENT", "ARMOUR_TAIL_WORLDS",
    "ARMOUR_TAIL_SEARCH", "ARMOUR_DA_REGS", "ARMOUR_EVAL_FULL", "ARMOUR_PLANE_CACHE", "ARMOUR_PC_K",
    "ARMOUR_PC_GROW_FAIL", "ARMOUR_REACH_CU_RESERVE", "ARMOUR_SOLVER_PRIORITY", "ARMOUR_LANE_SHAPE",
    "ARMOUR_SQ_THRESHOLD", "ARMOUR_MU_STRATEGY", "ARMOUR_ROW_CHUNK", "ARMOUR_TRACK_KERNEL",
    "ARMOUR_ENGINE", "ARMOUR_REACH_WIDE", "ARMOUR_JOB_ENGINE_JOBS",
}
ENGINE = "engine"          # conftest.engine(name): ARMOUR_ENGINE / ARMOUR_REACH_WIDE
ASSERTION = "assert_paths"


class Module:
    """a module of tests/: its top-level functions and classes, and what its imported names refer to"""

    def __init__(self, name):
        self.name = name
        self.tree = ast.parse(open(os.path.join(HERE, name + ".py")).read())
        self.defs = {n.name: n for n in self.tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
        self.names = {}    # local name -> (module, name in it) for `from M import a as b`
        self.aliases = {}  # local name -> module for `import M as C`
        for n in self.tree.body:
            if isinstance(n, ast.ImportFrom) and n.level == 0 and is_local(n.module):
                for a in n.names:
                    self.names[a.asname or a.name] = (n.module, a.name)
            elif isinstance(n, ast.Import):
                for a in n.names:
                    if is_local(a.name):
                        self.aliases[a.asname or a.name] = a.name


def is_local(module):
    return bool(module) and "." not in module and module != "conftest" and os.path.exists(os.path.join(HERE, module + ".py"))


_modules = {}


def module(name):
    if name not in _modules:
        _modules[name] = Module(name)
    return _modules[name]


def used_definitions(mod, node):
    """(module, definition) of every function or class of tests/ that `node` refers to: by name, as a
    fixture argument, or as an attribute of an imported module"""
    out = []

    def local(m, name):
        if name in m.defs:
            out.append((m, m.defs[name]))
        elif name in m.names:
            src, orig = m.names[name]
            local(module(src), orig)

    for n in ast.walk(node):
        if isinstance(n, ast.Name):
            local(mod, n.id)
        elif isinstance(n, ast.arg):
            local(mod, n.arg)
        elif isinstance(n, ast.Attribute) and isinstance(n.value, ast.Name) and n.value.id in mod.aliases:
            local(module(mod.aliases[n.value.id]), n.attr)
    return out


def reach(mod, node):
    """every (module, definition) reachable from `node`, itself included"""
    seen, stack = {}, [(mod, node)]
    while stack:
        m, d = stack.pop()
        if (m.name, id(d)) in seen:
            continue
        seen[m.name, id(d)] = (m, d)
        stack.extend(used_definitions(m, d))
    return list(seen.values())


def selects_a_path(node):
    """the settings `node` names, and "engine" when it calls conftest.engine"""
    found = set()
    for n in ast.walk(node):
        if isinstance(n, ast.Constant) and isinstance(n.value, str) and n.value in SETTINGS:
            found.add(n.value)
        elif isinstance(n, ast.keyword) and n.arg in SETTINGS:
            found.add(n.arg)
        elif isinstance(n, ast.Call):
            f = n.func
            if (isinstance(f, ast.Name) and f.id == ENGINE) or (isinstance(f, ast.Attribute) and f.attr == ENGINE):
                found.add(ENGINE)
    return found


def asserts_paths(node):
    for n in ast.walk(node):
        if isinstance(n, ast.Call):
            f = n.func
            if (isinstance(f, ast.Name) and f.id == ASSERTION) or (isinstance(f, ast.Attribute) and f.attr == ASSERTION):
                return True
    return False


def survey():
    """{test id: (settings it reaches, whether it reaches assert_paths)} over tests/test_gpu_*.py"""
    out = {}
    for path in sorted(glob.glob(os.path.join(HERE, "test_gpu_*.py"))):
        mod = module(os.path.splitext(os.path.basename(path))[0])
        for name, d in mod.defs.items():
            if not (isinstance(d, ast.FunctionDef) and name.startswith("test_")):
                continue
            defs = reach(mod, d)
            settings = set().union(*[selects_a_path(x) for _, x in defs])
            out[f"{mod.name}::{name}"] = (settings, any(asserts_paths(x) for _, x in defs))
    return out


def test_every_test_that_selects_a_path_asserts_it():
    found = survey()
    selecting = {k: v for k, v in found.items() if v[0]}
    # the scan itself works: the A/B tests of the solver's loop forms are among what it finds
    for known in ("test_gpu_edge::test_concurrent_restoration_matches_serial", "test_gpu_eval_small::test_eval_small_survey_worlds",
                  "test_gpu_track::test_row_kernel_is_bitwise_the_serial_kernel_and_reruns",
                  "test_gpu_lane_onepass::test_equals_parent_recording", "test_gpu_parity::test_config2_batch"):
        assert known in selecting, known
    missing = {k: sorted(v[0]) for k, v in selecting.items() if not v[1]}
    assert not missing, "tests that set a path-selecting setting and assert no path:\n" + \
        "\n".join(f"  {k}: {v}" for k, v in sorted(missing.items()))


def test_the_scan_sees_settings_fixtures_helpers_and_classes():
    """the scan on a module written here: a setting in a decorator, through a fixture, through a helper
    and through a context-manager class is found; a test that names none is not"""
    src = '''
import os
import pytest
class kernel:
    def __enter__(self):
        os.environ["ARMOUR_TRACK_KERNEL"] = "serial"
def helper():
    with env("ARMOUR_PC_K", "1"):
        pass
def checked():
    assert_paths({}, ran=())
@pytest.fixture
def fx():
    with engine("lane"):
        pass
@pytest.mark.parametrize("v", ["ARMOUR_RESTO_ROUNDS"])
def test_decorator(v):
    os.environ[v] = "1"
def test_fixture(fx):
    checked()
def test_helper():
    helper()
def test_class():
    with kernel():
        pass
def test_keyword():
    with C.env(ARMOUR_LANE_SHAPE="wide"):
        P.assert_paths(1)
def test_plain():
    os.environ["ARMOUR_LANE_CCAP"] = "1"
'''
    m = Module.__new__(Module)
    m.name, m.tree = "sample", ast.parse(src)
    m.defs = {n.name: n for n in m.tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
    m.names, m.aliases = {}, {}
    got = {}
    for name, d in m.defs.items():
        if name.startswith("test_"):
            defs = reach(m, d)
            got[name] = (set().union(*[selects_a_path(x) for _, x in defs]), any(asserts_paths(x) for _, x in defs))
    assert got == {"test_decorator": ({"ARMOUR_RESTO_ROUNDS"}, False), "test_fixture": ({"engine"}, True),
                   "test_helper": ({"ARMOUR_PC_K"}, False), "test_class": ({"ARMOUR_TRACK_KERNEL"}, False),
                   "test_keyword": ({"ARMOUR_LANE_SHAPE"}, True), "test_plain": (set(), False)}
