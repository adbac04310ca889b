"""The solver's launch sequence from a rocprofv3 --kernel-trace CSV (development tool): one line per
dispatch after the last reach kernel, in dispatch order, with the short kernel name, the grid in
workgroups, the workgroup size and the queue (numbered by first appearance, since queue ids differ
from process to process). Two builds that sequence the same launches print the same text, e.g. the
two libraries of `tools/gpu.sh 'libab ...'`:

    python tools/launch_seq.py A/run_kernel_trace.csv > a.txt; python tools/launch_seq.py B/... > b.txt; diff a.txt b.txt

usage: launch_seq.py <kernel_trace.csv>"""
import csv
import re
import sys


def short(name):
    """armour::eval_kernel_t<double, false, true>(armour::NlpDev, armour::Round, int) -> eval_kernel_t<double, false, true>"""
    name = re.sub(r"\.kd$", "", name)
    name = re.sub(r"^void\s+", "", name)
    depth = 0
    for i, c in enumerate(name):   # cut the argument list: the first '(' outside template brackets
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            name = name[:i]
            break
    return re.sub(r"\b(armour|lane)::", "", name)


def sequence(path):
    rows = list(csv.DictReader(open(path)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    reach = [i for i, r in enumerate(rows) if "reach_kernel" in r["Kernel_Name"]]
    rows = rows[reach[-1] + 1:] if reach else rows
    queues = {}
    out = []
    for r in rows:
        q = queues.setdefault(r["Queue_Id"], len(queues))
        wg = [int(r["Workgroup_Size_" + a]) for a in "XYZ"]
        grid = [int(r["Grid_Size_" + a]) // max(w, 1) for a, w in zip("XYZ", wg)]   # the trace counts work-items
        out.append("%-44s grid %-14s block %-12s q%d" % (short(r["Kernel_Name"]), "x".join(map(str, grid)),
                                                          "x".join(map(str, wg)), q))
    return out


if __name__ == "__main__":
    print("\n".join(sequence(sys.argv[1])))
