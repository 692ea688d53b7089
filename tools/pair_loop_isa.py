#!/usr/bin/env python3
"""Instruction counts of a pair-mode kernel's innermost loop, offline (needs hipcc, no GPU).

    python tools/pair_loop_isa.py mandelbrot [-D name=value ...] [--asm] [--all]

Emits the specialised kernel text of the filter under the current environment (so MMHIP_PAIR_EXIT=0 and the
other generator switches apply), compiles it to gfx950 assembly with the option list of the JIT (runtime.cpp
jit_source; hiprtc includes the HIP runtime header by itself, here it is named), finds the innermost loop of
mm_pixels (with --all: every innermost loop, in program order) and prints VALU / SALU / branch counts of

  * its likely path: from the loop header to the first branch back to it, and
  * its exit block: what follows, up to the next branch back to the header or out (for the exit-driven loops:
    the block that writes the exit copies; for the per-iteration form there is none, the block shown is
    whatever follows the loop).

s_nop and s_waitcnt are listed but not counted.  The counts are those of the compiler that is installed; its
version is printed first."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

JIT_OPTIONS = ["--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-std=c++17", "-fno-slp-vectorize"]


def hipcc():
    for c in (os.environ.get("HIPCC"), os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "bin", "hipcc"), "hipcc"):
        if c and (os.path.sep not in c or os.path.exists(c)):
            return c
    return "hipcc"


def assembly(source, to_object=False):
    """The kernel text's gfx950 assembly; with `to_object` it is assembled too (inline asm operands are only checked then)
    and the compiler's error text, empty on success, is returned instead."""
    with tempfile.TemporaryDirectory() as d:
        src, asm = os.path.join(d, "k.hip"), os.path.join(d, "k.o" if to_object else "k.s")
        with open(src, "w") as f:
            f.write(source)
        cmd = [hipcc(), "-x", "hip", "-include", "hip/hip_runtime.h", "--cuda-device-only", "-c" if to_object else "-S", "-o", asm, src] + JIT_OPTIONS
        r = subprocess.run(cmd, capture_output=True, text=True)
        if to_object:
            return r.stderr[-4000:] if r.returncode != 0 else ""
        if r.returncode != 0:
            sys.exit("compilation failed:\n" + r.stderr[-4000:])
        with open(asm) as f:
            return f.read()


def kernel_lines(asm, name):
    lines = asm.split("\n")
    start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
    return lines[start:end]


def classify(op):
    if op in ("s_nop", "s_waitcnt"):
        return "wait"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("s_"):
        return "salu"
    return "mem"


def instructions(lines):
    """[(label or None, opcode, text)] without comments and directives"""
    out, label = [], None
    for l in lines:
        t = l.split(";")[0].rstrip()
        if not t.strip():
            continue
        m = re.match(r"^(\.?[A-Za-z_][\w.$]*):", t)
        if m:
            label = m.group(1)
            continue
        t = t.strip()
        if t.startswith("."):
            continue
        out.append((label, t.split()[0], t))
        label = None
    return out


def innermost_header(lines):
    """label of the deepest loop header (the last one among equals: the pixel loop's inner loop)"""
    best, depth, label = None, -1, None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label = m.group(1)
        m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", l)
        if m and label and int(m.group(1)) > depth:
            best, depth = label, int(m.group(1))
    return best, depth


def innermost_headers(lines):
    """[(label, depth)] of every innermost loop, in program order"""
    out, label = [], None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            label = m.group(1)
        m = re.search(r"This Inner Loop Header: Depth=(\d+)", l)
        if m and label:
            out.append((label, int(m.group(1))))
    return out


def count(block):
    c = {"valu": 0, "salu": 0, "branch": 0, "mem": 0, "wait": 0}
    for _, op, _ in block:
        c[classify(op)] += 1
    return c


def analyse_loop(ins, header, depth, show):
    start = next(i for i, (lab, _, _) in enumerate(ins) if lab == header)
    back = next((i for i in range(start, len(ins)) if classify(ins[i][1]) == "branch" and ins[i][2].split()[-1] == header), None)
    if back is None:
        sys.exit("no branch back to " + header)
    likely = ins[start:back + 1]
    end = back + 1
    while end < len(ins):
        _, op, text = ins[end]
        end += 1
        if op == "s_branch" or (classify(op) == "branch" and text.split()[-1] == header):
            break
    exit_block = ins[back + 1:end]
    res = {}
    for name, block in (("likely path", likely), ("exit block", exit_block)):
        c = count(block)
        res[name] = c
        print("%-12s VALU %2d  SALU %2d  branch %d  (scalar + branch %2d)%s%s" % (
            name, c["valu"], c["salu"], c["branch"], c["salu"] + c["branch"],
            "  memory %d" % c["mem"] if c["mem"] else "", "  s_nop/s_waitcnt %d" % c["wait"] if c["wait"] else ""))
        if show:
            for _, _, text in block:
                print("    " + text)
    inner_branches = sum(1 for _, op, _ in likely[:-1] if classify(op) == "branch")
    if inner_branches:
        print("note: %d more branch(es) inside the likely path: it is not one basic block" % inner_branches)
    print("innermost loop: %s, depth %d" % (header, depth))
    res["fma"] = sum(1 for _, op, _ in likely if op.startswith("v_fma"))
    return res


def analyse(asm, show):
    lines = kernel_lines(asm, "mm_pixels")
    header, depth = innermost_header(lines)
    if header is None:
        sys.exit("mm_pixels has no loop")
    return analyse_loop(instructions(lines), header, depth, show)


def analyse_all(asm, show):
    """every innermost loop of mm_pixels, in program order: [counts as analyse gives them, with "fma": the v_fma_* of the likely path]"""
    lines = kernel_lines(asm, "mm_pixels")
    ins = instructions(lines)
    return [analyse_loop(ins, header, depth, show) for header, depth in innermost_headers(lines)]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("filter", help="name of a filter of tests/filters.py (mandelbrot, ...)")
    ap.add_argument("-D", dest="defs", action="append", default=[], metavar="name=value", help="user value to specialise on")
    ap.add_argument("--asm", action="store_true", help="print the instructions of both blocks")
    ap.add_argument("--all", action="store_true", help="every innermost loop of mm_pixels (a fused loop has two copies), not only the last")
    ap.add_argument("--source", metavar="FILE", help="analyse this kernel text instead of the generated one")
    args = ap.parse_args()
    ver = subprocess.run([hipcc(), "--version"], capture_output=True, text=True).stdout.strip().split("\n")
    print("compiler: " + "; ".join(l.strip() for l in ver[:2]))
    print("options : " + " ".join(JIT_OPTIONS))
    print("switches: " + (" ".join("%s=%s" % (k, v) for k, v in sorted(os.environ.items()) if k.startswith("MMHIP_PAIR")) or "(defaults)"))
    if args.source:
        with open(args.source) as f:
            source = f.read()
    else:
        from tests import filters as F
        uv = {}
        for d in args.defs:
            k, v = d.split("=", 1)
            uv[k] = float(v) if "." in v else int(v)
        source = F.load(args.filter).specialized(uv).kernel_source
    (analyse_all if args.all else analyse)(assembly(source), args.asm)


if __name__ == "__main__":
    main()
