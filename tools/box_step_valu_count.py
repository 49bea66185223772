#!/usr/bin/env python3
"""VALU instructions of one plane step of sdia_box2_kernel, counted in the device assembly of csrc/kernels.hip
(profiles/div_window_instruction_counts.txt).

  cd sparsh_amg_amd/csrc
  hipcc --offload-arch=gfx950 -std=c++17 -O3 -fPIC -fopenmp -ffp-contract=off --cuda-device-only -S kernels.hip -o kernels.s
  python tools/box_step_valu_count.py [tag=]kernels.s [[tag=]other.s ...]

For the instances <512, 3, 0, false> and <1024, 4, 1, false> (or those named with --instance BS,Q,TAG,ZERO[,XF]; XF, the exact-FMA
parameter, defaults to 1 and is ignored for an assembly file from before the kernels had it): the plane loop is the
loop of the function with the most basic blocks (the compiler marks them "in Loop: Header=..."); its blocks that hold a v_rcp_f64
are the plain-division fallback of div_const and are counted apart.  Counted: all instructions, those whose mnemonic starts with v_
(VALU), and of those the ones on fp64 operands (mnemonic contains f64).  Static counts of the loop's code, not executed instructions.
"""
import argparse
import collections
import re


def function_lines(path, symbol):
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(symbol + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    return lines[start:end + 1]


def basic_blocks(lines):
    blocks, cur = [], None
    for l in lines:
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", l):
            cur = {"head": l, "ins": []}
            blocks.append(cur)
        elif cur is not None and l.startswith("\t") and not l.strip().startswith((".", ";")):
            cur["ins"].append(l.split()[0])
    return blocks


def plane_loop(blocks):
    heads = collections.Counter(m.group(1) for b in blocks for m in [re.search(r"in Loop: Header=(BB\d+_\d+)", b["head"])] if m)
    h = heads.most_common(1)[0][0]
    return [b for b in blocks if f"Header={h} " in b["head"] or b["head"].startswith(f".L{h}:")]


def report(tag, path, inst):
    bs, q, t, zero, xf = inst
    symbol = f"_ZN6sparsh12_GLOBAL__N_116sdia_box2_kernelILi{bs}ELi{q}ELi{t}ELb{zero}ELb{xf}EEEvNS0_7BoxArgsEPKdS4_Pd"
    name = f"<{bs}, {q}, {t}, {'true' if zero else 'false'}, {'true' if xf else 'false'}>"
    try:
        lines = function_lines(path, symbol)
    except StopIteration:  # an assembly file from before the exact-FMA parameter
        lines = function_lines(path, symbol.replace(f"ELb{zero}ELb{xf}EEEv", f"ELb{zero}EEEv"))
        name = f"<{bs}, {q}, {t}, {'true' if zero else 'false'}>"
    loop = plane_loop(basic_blocks(lines))
    fallback = [b for b in loop if "v_rcp_f64_e32" in b["ins"]]
    ins = [x for b in loop if b not in fallback for x in b["ins"]]
    valu = [x for x in ins if x.startswith("v_")]
    f64 = collections.Counter(x for x in valu if "f64" in x)
    fb_valu = sum(x.startswith("v_") for b in fallback for x in b["ins"])
    print(f"{tag:8s} {name}: plane step without the plain-division fallback: {len(ins)} instructions, "
          f"{len(valu)} VALU, {sum(f64.values())} of them fp64-class; fallback: {len(fallback)} blocks, {fb_valu} VALU")
    print(f"{'':8s} fp64-class by opcode: " + ", ".join(f"{k} {f64[k]}" for k in sorted(f64)))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm", nargs="+", help="[tag=]path of a device assembly file of kernels.hip")
    ap.add_argument("--instance", action="append", help="BS,Q,TAG,ZERO[,XF] (ZERO, XF 0 or 1; XF defaults to 1); default 512,3,0,0 and 1024,4,1,0")
    args = ap.parse_args()
    insts = [(tuple(int(v) for v in s.split(",")) + (1,))[:5] for s in (args.instance or ["512,3,0,0", "1024,4,1,0"])]
    for inst in insts:
        for a in args.asm:
            tag, _, path = a.rpartition("=")
            report(tag or path, path, inst)


if __name__ == "__main__":
    main()
