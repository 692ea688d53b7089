#!/usr/bin/env python3
"""Instruction counts of a pair-mode kernel's innermost loop, offline (needs hipcc, no GPU).

    python tools/pair_loop_isa.py mandelbrot [-D name=value ...] [--asm] [--all] [--step]

Emits the specialised kernel text of the filter under the current environment (so MMHIP_PAIR_EXIT=0 and the
other generator switches apply), compiles it to gfx950 assembly with the option list of the JIT (runtime.cpp
jit_source; hiprtc includes the HIP runtime header by itself, here it is named), finds the innermost loop of
mm_pixels (with --all: every innermost loop, in program order) and prints VALU / SALU / branch counts of

  * its likely path: from the loop header to the first branch back to it, and
  * its exit block: what follows, up to the next branch back to the header or out (for the exit-driven loops:
    the block that writes the exit copies; for the per-iteration form there is none, the block shown is
    whatever follows the loop).

With --step it lists one step of the pixel loop instead -- what a pair step costs outside its inner loops (step_listing,
below).

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


# ---- one step of the pixel loop, outside its inner loops ----
MUL64 = ("v_mad_i64_i32", "v_mad_u64_u32", "v_mul_hi_u32", "v_mul_hi_i32")


def blocks_of(lines):
    """[{"name", "ins": [(opcode, text)], "header": depth or None, "in": (header label, depth) or None}] in layout order: a
    block starts at a label or at the compiler's `; %bb.N:` comment, the comments behind it say which loop it lies in"""
    out, cur = [], None
    for l in lines:
        m = re.match(r"^(\.LBB\d+_\d+):", l) or re.match(r"^; %bb\.(\d+):", l)
        if m:
            cur = {"name": m.group(1) if m.group(1).startswith(".") else "%bb." + m.group(1), "ins": [], "header": None, "in": None}
            out.append(cur)
        if cur is None:
            continue
        m = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", l)
        if m and not cur["ins"]:
            cur["header"] = int(m.group(1))
        m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", l)
        if m and not cur["ins"]:
            cur["in"] = (".L" + m.group(1), int(m.group(2)))
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") or re.match(r"^[\w.$]+:", t):
            continue
        cur["ins"].append((t.split()[0], t))
    return out


def step_listing(asm, show=False, quiet=False):
    """One step of mm_pixels' pixel loop (its outermost loop that has inner loops), the inner loops left out.

    The step's blocks -- those whose innermost loop is the pixel loop -- and the inner loops, each taken as one node, form a
    graph; every way from the loop header back to it is walked, and among those that pass through the last inner loop in
    program order and no other (the convention of the loop listing: for a fused loop, its fused copy) the one on which the fewest
    conditional branches are taken is listed as the likely path: the compiler lays the likely side of a branch out as the
    fall-through, and both the RGBA8 store and the fast step are marked likely in the text.  Counted: vector, scalar, branch and memory instructions of the step's blocks on
    that path; named: 64-bit multiplies (v_mad_i64_i32, v_mad_u64_u32, v_mul_hi_*) and vector compares among them."""
    blocks = blocks_of(kernel_lines(asm, "mm_pixels"))
    outer = next((b for b in blocks if b["header"] == 1 and any(c["in"] == (b["name"], 1) or (c["header"] or 0) > 1 for c in blocks)), None)
    if outer is None:
        sys.exit("mm_pixels has no pixel loop with inner loops")
    # node of every block: itself (a block of the step), the depth-2 loop it lies in, or None (outside the pixel loop)
    node, inner, cur2 = {}, [], None
    started = False
    for b in blocks:
        if b is outer:
            started = True
        if b is outer or b["in"] == (outer["name"], 1):
            node[b["name"]] = b["name"]
        elif started and (b["header"] or 0) == 2:
            cur2 = b["name"]
            inner.append(cur2)
            node[b["name"]] = cur2
        elif started and ((b["header"] or 0) > 2 or (b["in"] and b["in"][1] >= 2)):
            node[b["name"]] = cur2
        else:
            node[b["name"]] = None
    # edges, with what they cost: 1 for a conditional branch that is taken, 0 for falling through and for s_branch
    succ = {}
    for i, b in enumerate(blocks):
        n = node[b["name"]]
        if n is None:
            continue
        # (a wave that runs has lanes: s_cbranch_execnz is always taken, s_cbranch_execz never)
        targets = [(t.split()[-1], 0 if op in ("s_branch", "s_cbranch_execnz") or n in inner else 1) for op, t in b["ins"]
                   if classify(op) == "branch" and op != "s_cbranch_execz"]
        last = b["ins"][-1][0] if b["ins"] else None
        if last not in ("s_branch", "s_endpgm", "s_cbranch_execnz") and i + 1 < len(blocks):
            targets.append((blocks[i + 1]["name"], 0))
        for t, cost in targets:
            tn = node.get(t)
            if tn is not None and (tn != n or tn == outer["name"]):
                e = succ.setdefault(n, {})
                e[tn] = min(cost, e.get(tn, cost))
    by_name = dict((b["name"], b) for b in blocks)
    paths, stack = [], [(outer["name"], [outer["name"]], 0)]
    while stack and len(paths) < 200000:
        n, path, taken = stack.pop()
        for t, cost in succ.get(n, {}).items():
            if t == outer["name"]:
                paths.append((taken + cost, path))
            elif t not in path:
                stack.append((t, path + [t], taken + cost))
    last_inner = inner[-1] if inner else None
    through = [p for p in paths if [n for n in p[1] if n in inner] == [last_inner]] or paths
    if not through:
        sys.exit("no way through the pixel loop found")
    best = min(through, key=lambda p: (p[0], len(p[1])))[1]
    ins = [(n, op, t) for n in best if n not in inner for op, t in by_name[n]["ins"]]
    c = count([(None, op, t) for _, op, t in ins])
    res = dict(c)
    res["mul64"] = [t for _, op, t in ins if op in MUL64]
    res["vcmp"] = [t for _, op, t in ins if op.startswith("v_cmp")]
    res["vmem"] = [t for _, op, t in ins if classify(op) == "mem"]
    res["blocks"] = best
    res["ways"] = len(through)
    if not quiet:
        print("pair step     VALU %2d  SALU %2d  branch %d  memory %d  (outside the inner loops, likely path: %d blocks, %d ways through %s)" % (
            c["valu"], c["salu"], c["branch"], c["mem"], len([n for n in best if n not in inner]), len(through), last_inner))
        print("  64-bit multiplies: " + ("; ".join(res["mul64"]) or "none"))
        print("  vector compares  : " + ("; ".join(res["vcmp"]) or "none"))
        print("  memory           : " + ("; ".join(res["vmem"]) or "none"))
        if show:
            for n in best:
                print("  " + n + (":  (inner loop)" if n in inner else ":"))
                if n not in inner:
                    for op, t in by_name[n]["ins"]:
                        print("      " + t)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("filter", help="name of a filter of tests/filters.py (mandelbrot, ...)")
    ap.add_argument("-D", dest="defs", action="append", default=[], metavar="name=value", help="user value to specialise on")
    ap.add_argument("--asm", action="store_true", help="print the instructions of both blocks")
    ap.add_argument("--all", action="store_true", help="every innermost loop of mm_pixels (a fused loop has two copies), not only the last")
    ap.add_argument("--step", action="store_true", help="one step of the pixel loop outside its inner loops, likely path, instead of the loops")
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
    if args.step:
        step_listing(assembly(source), args.asm)
    else:
        (analyse_all if args.all else analyse)(assembly(source), args.asm)


if __name__ == "__main__":
    main()
