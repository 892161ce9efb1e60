#!/usr/bin/env python3
"""Instruction census of the wide-lane pipelined fast heat pass, per role and
per row update, from a device assembly listing of csrc/hip/heat_fast.hip:

    hipcc <the flags of _build.py> --cuda-device-only -S csrc/hip/heat_fast.hip -o heat_fast.s
    python benchmarks/heat_isa_census.py heat_fast.s [--kernel SUBSTR] [--md]

The kernel's steady state is one phase per workgroup barrier: RB = 2 row
updates of 8 points per lane. The listing of one kernel is cut at its
s_barrier lines; a piece with 2 x 32 v_pk_fma_f32 is one phase. Its role
follows from its memory instructions (role 0 loads rows from global memory,
the last role stores them, the roles between only touch the LDS ring) and the
masked (grid-edge) instantiation from its v_cndmask selects. Counts are
averaged over the phases of a class (the unroll period) and divided by the
rows per phase. It counts; it judges nothing.
"""
import argparse
import collections
import re
import sys

ROWS_PER_PHASE = 2
CLASSES = ["v_pk_add_f32", "v_pk_fma_f32", "v_pk_mul_f32", "v_mov_b32_dpp", "v_pk_mov_b32", "v_mov_b32",
           "v_mov_b64", "v_cndmask_b32", "other VALU", "VALU", "s_nop", "SALU", "LDS", "VMEM"]


def kernels(text):
    """{mangled name: [instruction lines]} and {name: metadata dict} of a listing."""
    body, meta = {}, {}
    name = None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m and "heat_pipe_kernel" in m.group(1):
            name = m.group(1)
            body[name] = []
            continue
        if name and re.match(r"^\s*\.(end_amdhsa_kernel|section|text)\b", line):
            name = None
        if name:
            s = line.split(";")[0].strip()
            if s and not s.startswith(".") and not s.endswith(":"):
                body[name].append(s)
    for entry in re.split(r"\n  - \.agpr_count:", text)[1:]:
        f = dict(re.findall(r"^    \.(\w+):\s+(\S+)\s*$", entry, re.M))
        if "name" in f:
            meta[f["name"]] = {"lds": int(f["group_segment_fixed_size"]), "scratch": int(f["private_segment_fixed_size"]),
                               "sgpr": int(f["sgpr_count"]), "vgpr": int(f["vgpr_count"]),
                               "spill": int(f["vgpr_spill_count"])}
    return body, meta


def census(lines):
    """Per-class counts of one piece of listing (instruction mnemonics, DPP
    moves told apart by their operands)."""
    c = collections.Counter()
    for s in lines:
        op = s.split()[0]
        dpp = op.endswith("_dpp")
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", op)
        if dpp and op == "v_mov_b32":
            op = "v_mov_b32_dpp"
        if op.startswith("v_"):
            c["VALU"] += 1
            c[op if op in CLASSES else "other VALU"] += 1
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith("s_") and op not in ("s_waitcnt", "s_barrier"):
            c["SALU"] += 1
        elif op.startswith("ds_"):
            c["LDS"] += 1
        elif op.startswith(("global_", "buffer_", "scratch_", "flat_")):
            c["VMEM"] += 1
            if not op.startswith("scratch_"):
                c["_load" if "load" in op else "_store"] += 1
    return c


def phases(lines):
    """Role / mask class -> list of per-phase Counters."""
    out = collections.defaultdict(list)
    piece = []
    for s in lines + ["s_barrier"]:
        if s.split()[0] != "s_barrier":
            piece.append(s)
            continue
        c = census(piece)
        piece = []
        if c["v_pk_fma_f32"] != 32 * ROWS_PER_PHASE:
            continue
        role = "0" if c["_load"] else ("last" if c["_store"] else "mid")
        masked = c["v_cndmask_b32"] >= 8 * ROWS_PER_PHASE
        out[(role, masked)].append(c)
    return out


def table(ph, md):
    rows = []
    for (role, masked), cs in sorted(ph.items(), key=lambda kv: (kv[0][1], {"0": 0, "mid": 1, "last": 2}[kv[0][0]])):
        n = len(cs) * ROWS_PER_PHASE
        avg = {k: sum(c[k] for c in cs) / n for k in CLASSES}
        rows.append((role, "masked" if masked else "unmasked", len(cs), avg))
    head = ["role", "instantiation", "phases"] + CLASSES
    sep = " | " if md else "  "
    lines = [sep.join(head)]
    if md:
        lines = ["| " + lines[0] + " |", "|" + "---|" * len(head)]
    for role, inst, n, avg in rows:
        cells = [role, inst, str(n)] + [f"{avg[k]:.1f}" for k in CLASSES]
        lines.append(("| " + sep.join(cells) + " |") if md else sep.join(cells))
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("listing")
    ap.add_argument("--kernel", default="", help="substring of the mangled kernel name (default: every pipe kernel)")
    ap.add_argument("--md", action="store_true", help="markdown tables")
    a = ap.parse_args()
    body, meta = kernels(open(a.listing).read())
    for name, lines in body.items():
        if a.kernel not in name:
            continue
        ph = phases(lines)
        if not ph:
            continue
        m = meta.get(name, {})
        print(f"\n{name}")
        print(f"vgpr {m.get('vgpr')}  sgpr {m.get('sgpr')}  scratch {m.get('scratch')} B  "
              f"spilled vgprs {m.get('spill')}  lds {m.get('lds')} B")
        print("per row update (counts per phase / %d), averaged over the unrolled phases:" % ROWS_PER_PHASE)
        print(table(ph, a.md))
    return 0


if __name__ == "__main__":
    sys.exit(main())
