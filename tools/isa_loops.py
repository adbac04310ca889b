"""Scratch (spill) traffic of a kernel's loops, from its assembly (development tool, build container).

Compile one kernel to assembly with line tables, e.g. the dense bundle reach kernel:
    printf '#include "reach_kernel.hip"\\n#include "lane_kernel.hip"\\nnamespace armour { namespace lane {\\n'\\
'template __global__ void lane_reach_kernel<LaneDense>(const RobotParams*, LaneArgs, ReachOut);\\n}}\\n' > /tmp/lane_only.hip
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -gline-tables-only --cuda-device-only -S \\
        -I armour-dev_amd/csrc -o /tmp/lane.s /tmp/lane_only.hip
then
    python tools/isa_loops.py /tmp/lane.s [SOURCE_FILE LAST_LINE]
lists the loops (back edges) with the most scratch_load / scratch_store instructions, and with
SOURCE_FILE and LAST_LINE (e.g. lane_engine.h and the line of `base += __popcll(km);`) the loops whose
last source line of that file is LAST_LINE: the simplify round loops, with their spill sites.

    python tools/isa_loops.py --round-waits /tmp/lane.s [SOURCE_FILE]
prints, for each loop that contains exactly one barrier and global stores after it (the compacting
rounds of simplify() and cross_const()): the vmcnt waits between the first store after the barrier
and the back edge (each also waits for the stores issued before it to be acknowledged), the vmcnt
waits between the loop header and the first LDS read (they hold the next round's index reads behind
the last round's stores; where no LDS read precedes the barrier, as in cross_const(), up to the
round's first load from memory), and the scratch accesses in the loop. Loops are taken from the
compiler's block comments (Loop Header / in Loop / Parent Loop), since the layout may put a loop's
latch blocks ahead of its header. A loop is named by its kernel and by the lines of SOURCE_FILE
(default lane_engine.h) its instructions come from. It counts waits and nothing else.

    python tools/isa_loops.py --mix /tmp/lane.s [SOURCE_FILE]
prints for the same loops (the compacting rounds) the instruction count by class: f64 VALU, other
VALU, SALU, lane moves (v_readlane / v_writelane / v_readfirstlane / v_permlane), loads (global, flat,
scratch, scalar), stores, LDS, waits (s_waitcnt, s_barrier) and nops, and the number of v_rsq_f64:
each marks one expanded fp64 square root (none is left in a round once the keep / prune decisions
compare squared norms). Whole bodies, inner loops included. It counts and classifies."""
import collections
import re
import sys

mix = sys.argv[1:2] == ["--mix"]
round_waits = mix or sys.argv[1:2] == ["--round-waits"]
if round_waits:
    del sys.argv[1]
lines = open(sys.argv[1]).read().split("\n")
files, loc, cur, labels = {}, [None] * len(lines), None, {}
for i, l in enumerate(lines):
    m = re.match(r'\s*\.file\s+(\d+)\s+"([^"]*)"\s*"([^"]*)"', l)
    if m:
        files[m.group(1)] = m.group(3).split("/")[-1]
    m = re.match(r"\s*\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        cur = (files.get(m.group(1), m.group(1)), int(m.group(2)))
    loc[i] = cur
    m = re.match(r"^(\.LBB\d+_\d+):", l)
    if m:
        labels[m.group(1)] = i
loops = []
for i, l in enumerate(lines):
    m = re.match(r"\s*s_(cbranch_\w+|branch)\s+(\.LBB\d+_\d+)", l)
    if m and m.group(2) in labels and labels[m.group(2)] < i:
        loops.append((labels[m.group(2)], i))


def count(a, b, what):
    return sum(what in x for x in lines[a:b + 1])


def instr(j):
    return lines[j].split(";")[0].strip()


def vm_wait(j):
    return instr(j).startswith("s_waitcnt") and "vmcnt" in instr(j)


CLASSES = ("f64 VALU", "other VALU", "SALU", "lane moves", "loads", "stores", "LDS", "waits", "nops")


def classify(op):
    if re.match(r"v_(readlane|writelane|readfirstlane|permlane)", op):
        return "lane moves"
    if op.startswith("v_"):
        return "f64 VALU" if "_f64" in op else "other VALU"
    if op.startswith("ds_"):
        return "LDS"
    if re.match(r"(global|flat|scratch|buffer)_load|s_(buffer_)?load", op):
        return "loads"
    if re.match(r"(global|flat|scratch|buffer)_(store|atomic)", op):
        return "stores"
    if op.startswith("s_waitcnt") or op.startswith("s_barrier"):
        return "waits"
    if op.startswith("s_nop"):
        return "nops"
    if op.startswith("s_"):
        return "SALU"
    return None


def loop_blocks():
    """Loops by the compiler's own block comments: header label -> sorted (start, end) line ranges of
    its blocks, nested loops' blocks included (blocks of one loop need not be contiguous)."""
    starts = [i for i, l in enumerate(lines) if re.match(r"^\.LBB\d+_\d+:", l)]
    funcs = [i for i, l in enumerate(lines) if ".cfi_endproc" in l or l.startswith(".Lfunc_end")]
    own, parents = {}, {}
    for k, i in enumerate(starts):
        end = min([f for f in funcs if f > i][:1] + starts[k + 1:k + 2] + [len(lines)])
        name = lines[i].split(":")[0][2:]
        cm, j = [lines[i].split(";", 1)[1] if ";" in lines[i] else ""], i + 1
        while j < len(lines) and lines[j].lstrip().startswith(";"):
            cm.append(lines[j])
            j += 1
        cm = "\n".join(cm)
        m = re.search(r"in Loop: Header=(BB\d+_\d+)", cm)
        if m:
            own.setdefault(m.group(1), []).append((i, end - 1))
        elif "Loop Header" in cm:
            own.setdefault(name, []).append((i, end - 1))
            parents[name] = re.findall(r"Parent Loop (BB\d+_\d+)", cm)
    full = {h: list(r) for h, r in own.items()}
    for h, ps in parents.items():
        for q in ps:
            full.setdefault(q, []).extend(own.get(h, []))
    return {h: sorted(r) for h, r in full.items()}, parents


if round_waits:
    src = sys.argv[2] if len(sys.argv) > 2 else "lane_engine.h"
    blocks, parents = loop_blocks()
    kernels = [(i, l.split(":")[0]) for i, l in enumerate(lines) if re.match(r"^[A-Za-z_]\w*:", l)]
    n, tot, kern = 0, [0, 0], None
    for h, rs in sorted(blocks.items(), key=lambda kv: kv[1][0]):
        body = [j for a, b in rs for j in range(a, b + 1)]  # in layout order
        bar = [k for k, j in enumerate(body) if instr(j).startswith("s_barrier")]
        if len(bar) != 1:
            continue
        st = [k for k in range(bar[0], len(body)) if re.match(r"(global|flat)_store", instr(body[k]))]
        if not st:
            continue
        # the round's first read: an LDS read ahead of the barrier, else the first load from memory
        rd = [k for k in range(bar[0]) if re.match(r"ds_read", instr(body[k]))]
        what = "LDS read"
        if not rd:
            rd = [k for k in range(bar[0]) if re.match(r"(global|flat)_load", instr(body[k]))]
            what = "load (no LDS read ahead of the barrier)"
        # the layout may put the latch blocks ahead of the header: walk the round from the header
        hd = next(k for k, j in enumerate(body) if lines[j].startswith(".L" + h + ":"))
        order = body[hd:] + body[:hd]
        pos = {j: k for k, j in enumerate(order)}
        first_st = min(pos[body[k]] for k in st)
        after = sum(vm_wait(j) for j in order[first_st:])
        before = sum(vm_wait(j) for j in order[:min(pos[body[k]] for k in rd)]) if rd else 0
        ln = sorted({loc[j][1] for j in body if loc[j] and loc[j][0] == src and loc[j][1] > 0})
        sl = sum("scratch_load" in instr(j) for j in body)
        ss = sum("scratch_store" in instr(j) for j in body)
        k = [nm for i, nm in kernels if i < rs[0][0]][-1:]
        if k and k[0] != kern:
            kern = k[0]
            print(f"kernel {kern}")
        n += 1
        if mix:
            ops = [instr(j).split()[0] for j in body if instr(j) and re.match(r"[a-z]", instr(j))]
            cnt = collections.Counter(c for c in map(classify, ops) if c)
            rsq = sum(o.startswith("v_rsq_f64") for o in ops)
            tot[0] += sum(cnt.values())
            tot[1] += rsq
            print(f"  loop {h} (depth {len(parents.get(h, [])) + 1}, {src}:{ln[0]}-{ln[-1]}): {sum(cnt.values())} instructions: "
                  + ", ".join(f"{c} {cnt[c]}" for c in CLASSES) + f"; v_rsq_f64 {rsq}")
            continue
        tot[0] += after
        tot[1] += before
        print(f"  loop {h} (depth {len(parents.get(h, [])) + 1}, {src}:{ln[0]}-{ln[-1]}, {len(body)} lines, {len(st)} stores to memory): "
              f"vmcnt waits after the first store {after}, before the first {what} {before}; "
              f"scratch loads {sl}, stores {ss}")
    if mix:
        print(f"{n} round loops: {tot[0]} instructions, v_rsq_f64 {tot[1]}")
    else:
        print(f"{n} round loops: vmcnt waits after the first store {tot[0]}, before the first read {tot[1]}")
elif len(sys.argv) > 3:
    src, last = sys.argv[2], int(sys.argv[3])
    for a, b in sorted(set(loops)):
        own = [loc[j][1] for j in range(a, b + 1) if loc[j] and loc[j][0] == src]
        if not own or max(own) != last:
            continue
        sites = collections.Counter(loc[a + k] for k, x in enumerate(lines[a:b + 1]) if "scratch_" in x)
        print(f"loop at asm line {a}: {b - a} lines, scratch loads {count(a, b, 'scratch_load')}, "
              f"stores {count(a, b, 'scratch_store')}, global loads {count(a, b, 'global_load')}, "
              f"flat {count(a, b, 'flat_')}; spill sites {dict(sites.most_common(5))}")
else:
    for a, b in sorted(loops, key=lambda ab: -count(ab[0], ab[1], "scratch_"))[:30]:
        print(f"loop at asm line {a}: {b - a} lines, scratch loads {count(a, b, 'scratch_load')}, "
              f"stores {count(a, b, 'scratch_store')}, flat {count(a, b, 'flat_')}")
