"""INTEGRATION.md's environment-variable tables against the sources (text only, no device): every
ARMOUR_* name the native code passes to getenv is documented, every documented variable is read
somewhere, and planner.hip reads the environment only where it says it does: in Settings::from_env
and at the three per-call test hooks. (That ARMOUR_ROW_CHUNK no longer reaches a live planner needs
a device: tests/test_gpu_regrow.py.)"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "armour-dev_amd", "csrc")
GETENV = re.compile(r'getenv\(\s*"(ARMOUR_[A-Z0-9_]+)"')
PER_CALL = {"ARMOUR_TRACK_KERNEL", "ARMOUR_DUMP_LANE", "ARMOUR_PC_GROW_FAIL"}


def read(path):
    with open(path, encoding="utf-8", errors="replace") as f:
        return f.read()


def documented():
    """the ARMOUR_* names in the first column of the tables under "Environment variables read by the library\""""
    text = read(os.path.join(ROOT, "INTEGRATION.md"))
    section = text.split("### Environment variables read by the library", 1)[1].split("\n## ", 1)[0]
    names = set()
    for line in section.splitlines():
        if line.startswith("| `"):
            names.update(re.findall(r"ARMOUR_[A-Z0-9_]+", line.split("|")[1]))
    return names


def native_sources():
    return sorted(p for ext in ("*.hip", "*.cpp", "*.h") for p in glob.glob(os.path.join(CSRC, ext)))


def test_every_variable_the_native_code_reads_is_documented():
    read_by = {}
    for path in native_sources():
        for name in GETENV.findall(read(path)):
            read_by.setdefault(name, os.path.basename(path))
    assert len(read_by) >= 30, sorted(read_by)   # the search itself found the reads
    missing = {n: f for n, f in read_by.items() if n not in documented()}
    assert not missing, missing


def test_every_documented_variable_is_read_somewhere():
    files = native_sources() + [os.path.join(ROOT, "bench.py")]
    for sub, ext in (("armour-dev_amd/armour_amd", "*.py"), ("tools", "*"), ("tests", "*.py")):
        files += [p for p in glob.glob(os.path.join(ROOT, sub, ext)) if os.path.isfile(p) and p != os.path.abspath(__file__)]
    text = "\n".join(read(p) for p in files if not p.endswith((".so", ".pyc")))
    names = documented()
    assert len(names) >= 30, sorted(names)      # the tables were found
    # a read: getenv("X"), os.environ.get("X"), os.environ["X"] not being assigned, "X" in os.environ, $X in a script
    reads = (r'getenv\(\s*"{0}"|environ\.get\(\s*["\']{0}["\']|environ\[["\']{0}["\']\](?!\s*=[^=])|'
             r'["\']{0}["\']\s+in\s+os\.environ|\$\{{?{0}\b')
    unread = sorted(n for n in names if not re.search(reads.format(n), text))
    assert not unread, unread


def test_planner_reads_the_environment_in_one_place():
    src = read(os.path.join(CSRC, "planner.hip"))
    body = src.split("static Settings from_env() {", 1)[1].split("\n    }\n", 1)[0]
    inside = GETENV.findall(body)
    outside = GETENV.findall(src.replace(body, ""))
    assert sorted(outside) == sorted(PER_CALL), outside
    assert not PER_CALL & set(inside)
    assert src.replace(body, "").count("getenv") == len(PER_CALL)   # (no read that the pattern does not see)
