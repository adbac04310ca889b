"""Static size of the row passes' block reduction (development tool): per row kernel of a gfx950
assembly listing of nlp_kernels.hip, the instruction count, the count inside the basic blocks that
hold cross-lane moves (DPP or permlane: the wave reductions; a row loop has none) and the number
of cross-lane moves; and, from the compiler's resource remarks, registers, scratch, LDS and waves
per SIMD. Two listings print side by side (profiles/row_reduce_isa.txt, row_reduce_resources.txt).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off --cuda-device-only -S \
        -Rpass-analysis=kernel-resource-usage -o new.s nlp_kernels.hip 2> new.txt
usage: python tools/row_reduce_isa.py isa parent.s new.s | res parent.txt new.txt"""
import re
import sys

ROW = re.compile(r"^_ZN6armour\d+((?:ipm|resto)_rows_\w+?)ENS_6NlpDevENS_5RoundE$")
CROSS = re.compile(r"_dpp|permlane| row_sh[lr]:| quad_perm:")


def isa(path):
    out, name, blocks = {}, None, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(\S+):\s*(;.*)?$", s)
        if m and not s.startswith("."):
            k = ROW.match(m.group(1))
            if k:
                name, blocks = k.group(1), [[]]
                out[name] = blocks
            continue
        if name is None:
            continue
        if s.startswith(".Lfunc_end"):
            name = None
        elif re.match(r"^\.LBB\d+_\d+:", s):
            blocks.append([])
        elif s and not s.startswith((".", ";")):
            blocks[-1].append(s)
    res = {}
    for k, bl in out.items():
        red = [b for b in bl if any(CROSS.search(i) for i in b)]
        res[k] = (sum(len(b) for b in bl), sum(len(b) for b in red), sum(1 for b in red for i in b if CROSS.search(i)))
    return res


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            k = ROW.match(m.group(1))
            name = k.group(1) if k else None
            if name:
                out[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?)(?: \[[^\]]*\])?: (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1)] = m.group(2)
    return out


if __name__ == "__main__":
    mode, pa, pb = sys.argv[1:4]
    if mode == "isa":
        a, b = isa(pa), isa(pb)
        print(f"{'kernel':24s} {'parent: instr':>13s} {'in red. blocks':>14s} {'cross-lane':>10s}   {'change: instr':>13s} "
              f"{'in red. blocks':>14s} {'cross-lane':>10s}  {'red. ratio':>10s}")
        for k in sorted(b):
            x, y = a.get(k, (0, 0, 0)), b[k]
            print(f"{k:24s} {x[0]:13d} {x[1]:14d} {x[2]:10d}   {y[0]:13d} {y[1]:14d} {y[2]:10d}  {y[1] / max(x[1], 1):10.2f}")
    else:
        a, b = resources(pa), resources(pb)
        keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize", "VGPRs Spill", "LDS Size", "Occupancy")
        print(f"{'kernel':24s} " + " ".join(f"{k:>12s}" for k in keys) + "   (parent -> change)")
        for k in sorted(b):
            print(f"{k:24s} " + " ".join(f"{a.get(k, {}).get(q, '?') + '->' + b[k].get(q, '?'):>12s}" for q in keys))
