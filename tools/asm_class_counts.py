#!/usr/bin/env python3
"""Static instruction counts of one kernel in a device assembly listing (hipcc --cuda-device-only -S), by class:
FP64 arithmetic, other VALU, SALU, branches, memory -- for the whole kernel, per basic block, or for a range of blocks
(the trip loop of the RK4 trace kernels is read off the listing: from the loop's header to its back edge).

  tools/asm_class_counts.py LISTING.s KERNEL_SUBSTRING [--blocks] [--range FIRST_LABEL LAST_LABEL] [--grep REGEX]
"""
import argparse
import re
import sys
from collections import OrderedDict

FP64 = re.compile(r"^v_(add|mul|fma|fmac|min|max|div_scale|div_fmas|div_fixup|rcp|rsq|sqrt|fract|floor|ceil|trunc|rndne|"
                  r"ldexp|frexp_mant|trig_preop|cvt_f64|cvt_i32|cvt_u32|cvt_f32)_f64|^v_(cvt_f64_|frexp_exp_i32_f64|cmp\w*_f64|"
                  r"cmpx\w*_f64|cvt_\w+_f64)")
CLASSES = ("fp64", "valu", "salu", "branch", "mem", "other")


def classify(op):
    if op.startswith(("s_branch", "s_cbranch", "s_setpc", "s_swappc", "s_endpgm")):
        return "branch"
    if op.startswith(("s_load", "s_buffer_load", "global_", "flat_", "scratch_", "ds_", "buffer_")):
        return "mem"
    if op.startswith(("s_waitcnt", "s_nop", "s_sleep", "s_barrier", "s_setprio", "s_inst_prefetch", "s_code_end")):
        return "other"
    if op.startswith("s_"):
        return "salu"
    if op.startswith("v_"):
        return "fp64" if FP64.match(op) else "valu"
    return "other"


def kernel_blocks(path, needle):
    blocks, cur, inside = OrderedDict(), None, False
    for line in open(path):
        t = line.split(";")[0].strip()
        if not inside:
            if t.endswith(":") and needle in t and not t.startswith("."):
                inside, cur = True, "entry"
                blocks[cur] = []
            continue
        if t.startswith(".Lfunc_end") or t.startswith(".section"):
            break
        if not t or t.startswith("//"):
            continue
        if t.endswith(":") and t.startswith(".LBB"):
            cur = t[:-1]
            blocks[cur] = []
            continue
        if t.startswith("."):
            continue
        blocks[cur].append(t)
    if not blocks:
        sys.exit(f"no kernel matching {needle!r} in {path}")
    return blocks


def count(instrs):
    c = dict.fromkeys(CLASSES, 0)
    for i in instrs:
        c[classify(i.split()[0])] += 1
    return c


def show(name, instrs):
    c = count(instrs)
    print(f"{name:>14}: total {len(instrs):5d}  " + "  ".join(f"{k} {c[k]:4d}" for k in CLASSES))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--blocks", action="store_true")
    ap.add_argument("--range", nargs=2, metavar=("FIRST", "LAST"))
    ap.add_argument("--grep", help="list the instructions of the selection that match this regular expression")
    a = ap.parse_args()
    blocks = kernel_blocks(a.listing, a.kernel)
    names = list(blocks)
    if a.range:
        i0, i1 = names.index(a.range[0]), names.index(a.range[1])
        names = names[i0:i1 + 1]
    if a.blocks:
        for n in names:
            show(n, blocks[n])
    sel = [i for n in names for i in blocks[n]]
    show("selection" if a.range else "kernel", sel)
    if a.grep:
        rx = re.compile(a.grep)
        for n in names:
            for i in blocks[n]:
                if rx.search(i):
                    print(f"  {n}: {i}")


if __name__ == "__main__":
    main()
