#!/usr/bin/env python3
"""Do two device assembly listings hold the same kernels, instruction for
instruction?

    hipcc <the flags of _build.py> --cuda-device-only -S csrc/hip/heat_fast.hip -o new.s
    python benchmarks/isa_equal.py old.s new.s

For a refactor that renames kernels (template arguments change the mangled
names) but must not change their machine code. Each listing is cut into its
kernels (.amdhsa_kernel); of each kernel it keeps the instructions, labels
and the .amdhsa_ resource directives plus the metadata note's register,
spill, scratch and LDS figures, drops comments, renumbers local labels by
first appearance and replaces the kernel's own symbol by a placeholder. The
two multisets of kernel texts must be equal: exit status 0, else 1 with the
demangled names left unmatched on either side.
"""
import collections
import re
import shutil
import subprocess
import sys

META = ["group_segment_fixed_size", "private_segment_fixed_size", "kernarg_segment_size", "max_flat_workgroup_size",
        "sgpr_count", "sgpr_spill_count", "vgpr_count", "vgpr_spill_count", "agpr_count", "wavefront_size"]


def kernels(text):
    """[(mangled name, normalised text)] of every kernel of a listing."""
    lines = text.splitlines()
    start = {}
    for i, line in enumerate(lines):
        m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
        if m:
            start.setdefault(m.group(1), i)
    meta = {}
    for entry in re.split(r"\n  - \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"^    \.(\w+):\s+(\S+)\s*$", "    .agpr_count:" + entry, re.M))
        if "name" in f:
            meta[f["name"]] = [f"{k}={f.get(k)}" for k in META]
    out = []
    for i, line in enumerate(lines):
        m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
        if not m:
            continue
        name = m.group(1)
        body, labels = [], {}
        for raw in lines[start[name] + 1:]:
            s = raw.split(";")[0].strip()
            if s:
                s = re.sub(r"\.L[\w$.]+", lambda l: labels.setdefault(l.group(0), f".L{len(labels)}"), s)
                body.append(re.sub(r"\s+", " ", s.replace(name, "<kernel>")))
            if s == ".end_amdhsa_kernel":
                break
        out.append((name, "\n".join(body + meta.get(name, ["no metadata"]))))
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if not tool or not names:
        return names
    return subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sides = [kernels(open(p).read()) for p in sys.argv[1:]]
    count = [collections.Counter(t for _, t in ks) for ks in sides]
    rc = 0
    for label, ks, mine, other in (("old", sides[0], count[0], count[1]), ("new", sides[1], count[1], count[0])):
        left = mine - other  # texts this side has more often than the other
        names = []
        for name, t in ks:
            if left[t] > 0:
                left[t] -= 1
                names.append(name)
        for n in demangle(names):
            print(f"unmatched in {label}: {n}")
            rc = 1
    print(f"{sys.argv[1]}: {len(sides[0])} kernels, {sys.argv[2]}: {len(sides[1])} kernels, "
          f"{'equal' if rc == 0 else 'DIFFERENT'}")
    return rc


if __name__ == "__main__":
    sys.exit(main())
