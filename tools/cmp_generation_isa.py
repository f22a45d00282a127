#!/usr/bin/env python3
"""Are the generation kernels (k_main*, k_setup, k_indel_*, k_perfect, k_mt_*) of two device assembly files the same code?
A change that adds kernels of its own must leave them alone; --all compares every kernel of the first file instead (a change of
the host side alone must leave all of them as they are).  Compared per kernel: every instruction, directive and label, with
comments dropped and the function number taken out of the basic-block labels (.LBB<function>_<block>: hipcc numbers the
functions of a translation unit in order, so a kernel added in front of another renumbers labels and nothing else) and the
suffix out of a renumbered private symbol (.crctable.92: the compiler numbers function-local statics that share a name across
the translation unit, so a header whose statics move renumbers them and nothing else; two numbered statics of one name that a kernel swaps would
pass unseen).
For each kernel that differs, both files' instruction count and register use (amdhsa.kernels metadata) are printed.

Usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -w -I include -S --cuda-device-only -cuid=iss -o new.s insilicoseq_amd/csrc/iss_mi355x.hip
       (the library's own optimisation flags, __graft_entry__.build(); one -cuid for both files; the same on the parent commit ->
       parent.s);  python tools/cmp_generation_isa.py [--all] parent.s new.s"""
import re
import sys

GENERATION = re.compile(r"k_main|k_setup|k_indel_|k_perfect|k_mt_")
PRIVATE_NUMBER = re.compile(r"(?<![\w.])(\.[A-Za-z_]\w*)\.\d+(?=@|\b)")  # .crctable.92@rel32@lo -> .crctable.N@rel32@lo


def kernels(path):
    out, name = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name is not None:
            if line.startswith(".Lfunc_end"):
                name = None
                continue
            line = line.split(";", 1)[0].rstrip()
            if line:
                out[name].append(PRIVATE_NUMBER.sub(r"\1.N", re.sub(r"\.LBB\d+_", ".LBB_", line)))
    return out


RESOURCES = ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size")


def resources(path):
    """kernel -> {field: value} of RESOURCES, from the file's amdhsa.kernels metadata"""
    out, cur, inside = {}, {}, False
    for line in open(path):
        if line.startswith("amdhsa.kernels:"):
            inside = True
        elif inside and not line.startswith(" "):
            inside = False
        elif inside:
            if line.startswith("  - "):  # the next kernel's entry
                cur = {}
            m = re.match(r"^  [ -] \.(\w+):\s+(\S+)", line)
            if m:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == "name":
                    out[m.group(2)] = cur
    return out


def instructions(lines):
    return sum(1 for x in lines if not x.endswith(":") and not x.lstrip().startswith("."))


def main():
    every = "--all" in sys.argv[1:]
    paths = [x for x in sys.argv[1:] if x != "--all"]
    a, b = kernels(paths[0]), kernels(paths[1])
    names = [k for k in a if every or GENERATION.search(k)]
    bad = [k for k in names if a[k] != b.get(k)]
    res = [resources(p) for p in paths[:2]] if bad else None
    for k in bad:
        print("differs: %s" % k)
        for path, body, r in zip(paths, (a[k], b.get(k)), res):
            if body is None:
                print("    %s: missing" % path)
                continue
            print("    %s: %d instructions, %s" % (path, instructions(body), ", ".join(
                "%s %s" % (f, r.get(k, {}).get(f, "?")) for f in RESOURCES)))
    print("%d %skernels compared, %d differ (%d instructions and labels in all); kernels only in the second file: %d" % (
        len(names), "" if every else "generation ", len(bad), sum(len(a[k]) for k in names), len(set(b) - set(a))))
    return 1 if bad or not names else 0


if __name__ == "__main__":
    sys.exit(main())
