"""Compares the kernels of two device assembly files, one line per kernel: identical, reordered or differs.

    hipcc -std=c++17 -O2 -fPIC -I. -I../../include --offload-arch=gfx950 -ffp-contract=off --cuda-device-only -S clip_yuv.hip -o new.s
    python tools/clip_yuv_asm_compare.py parent.s new.s

Kernels are paired by demangled name and template arguments.  What is compared is a kernel's instruction text: labels,
comments, directives (.file, .ident, .p2align ...) and symbol names are left out.
  identical  the same instructions in the same order
  reordered  the same multiset of opcodes, and .amdhsa_next_free_vgpr, .amdhsa_next_free_sgpr, the LDS size and the
             private segment size are the parent's, the last one 0 (no scratch)
  differs    anything else, a kernel that only one file has included
The exit status is 0 when no kernel differs."""
import collections
import re
import subprocess
import sys

RESOURCES = (".amdhsa_next_free_vgpr", ".amdhsa_next_free_sgpr", ".amdhsa_group_segment_fixed_size", ".amdhsa_private_segment_fixed_size")


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return dict(zip(names, out))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def kernels(path):
    """{mangled name: (instructions, resources)} of one assembly file"""
    text, resources, body, block = {}, {}, None, None
    for raw in open(path):
        line = raw.split(";")[0].strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            block = resources.setdefault(m.group(1), {})
        elif line == ".end_amdhsa_kernel":
            block = None
        elif block is not None:
            word = line.split()
            if word and word[0] in RESOURCES:
                block[word[0]] = word[1]
        elif re.match(r"\.Lfunc_end\d+:", line):
            body = None
        elif re.match(r"[A-Za-z_][\w$.]*:$", line) and not line.startswith(".L"):
            body = text.setdefault(line[:-1], [])
        elif body is not None and line and not line.startswith(".") and not line.endswith(":"):
            body.append(re.sub(r"\.LBB\d+_\d+", ".LBB", " ".join(line.split())))
    return {name: (text[name], resources[name]) for name in resources if name in text}


def verdict(parent, new):
    if parent is None or new is None:
        return "differs"
    if parent[0] == new[0]:
        return "identical"
    opcodes = lambda body: collections.Counter(line.split()[0] for line in body)
    if opcodes(parent[0]) == opcodes(new[0]) and parent[1] == new[1] and new[1].get(".amdhsa_private_segment_fixed_size") == "0":
        return "reordered"
    return "differs"


def main(argv):
    if len(argv) != 3:
        sys.exit(__doc__)
    parent, new = kernels(argv[1]), kernels(argv[2])
    names = demangle(sorted(set(parent) | set(new)))
    worst = 0
    for mangled, name in sorted(names.items(), key=lambda kv: kv[1]):
        v = verdict(parent.get(mangled), new.get(mangled))
        worst |= v == "differs"
        print("%s  %s" % (v.ljust(9), re.sub(r"^void |\(.*\)$", "", name)))
    return worst


if __name__ == "__main__":
    sys.exit(main(sys.argv))
