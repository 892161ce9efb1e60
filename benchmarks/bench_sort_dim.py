"""sort(x, dim=) against torch.sort(x, dim, stable=True) on one GPU.

    python benchmarks/bench_sort_dim.py [--rounds 6] [--out table.md]

The project's convention (benchmarks/bench_primitives.py, scan_dim /
reduce_dim): three operand sets per shape (cache-defeated: every set is 256 MiB
or more), the arms alternated call by call in one process in an order
reshuffled every round, one event pair per call; median [min, max] ms. Arms:
this sort, torch.sort(stable=True), and a copy of the same operands, the
yardstick of the run: "pass share" is the time the copy's rate needs for the
bytes ONE pass over the data must move (esize read, esize + 8 written per
element) over the arm's time. Prints one JSON line per arm and, with --out,
writes the markdown table (the table of profiles/sort_dim.md)."""
import argparse
import json
import os
import random
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

SHAPES = [  # (shape, dim, what); the regime column of the table comes from sort_dim_launch_info
    ((65536, 2048), -1, "four lines per tile"),
    ((4096, 8192), -1, "one line per tile"),
    ((1 << 20, 64), -1, "short lines"),
    ((64, 1 << 21), 0, "short columns"),
    ((16, 1 << 22), -1, "long lines"),
    ((8192, 8192), 0, "columns of the tile's length"),
    ((16384, 4096), 0, "columns above the tile"),
]


def alternate(torch, arms, rounds, warm=1):
    order = list(arms)
    rnd = random.Random(0)
    ts = {a: [] for a in arms}
    turn = {a: 0 for a in arms}
    for r in range(rounds + warm):
        rnd.shuffle(order)  # no arm always runs behind the same predecessor
        for name in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            arms[name](turn[name] % 3)
            e1.record()
            e1.synchronize()
            turn[name] += 1
            if r >= warm:
                ts[name].append(e0.elapsed_time(e1))
    return {a: (sorted(t)[len(t) // 2], min(t), max(t)) for a, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of a shape's description")
    args = ap.parse_args()

    import torch

    import cme213x  # noqa: F401
    from cme213x.ops.sort import sort, sort_dim_launch_info

    dev = torch.device("cuda:0")
    rows = []
    for dt in (torch.float32, torch.int64):
        esize = 4 if dt == torch.float32 else 8
        for shape, dim, what in SHAPES:
            if args.only and args.only not in what:
                continue
            numel = shape[0] * shape[1]
            if dt == torch.float32:
                xs = [torch.rand(shape, device=dev, dtype=dt) for _ in range(3)]
            else:
                xs = [torch.randint(-2 ** 40, 2 ** 40, shape, device=dev, dtype=dt) for _ in range(3)]
            ys = [torch.empty_like(x) for x in xs]
            info = sort_dim_launch_info(shape, dim, dtype=dt, device=dev)
            regime = f"{info['regime']}, {info['form']}: {what}"
            ours = sort(xs[0], dim=dim)
            ref = torch.sort(xs[0], dim=dim, stable=True)
            ok = bool(torch.equal(ours.values, ref.values) and torch.equal(ours.indices, ref.indices))
            del ours, ref
            arms = {
                "copy": lambda i: ys[i].copy_(xs[i]),
                "sort_dim": lambda i: sort(xs[i], dim=dim),
                "torch.sort": lambda i: torch.sort(xs[i], dim=dim, stable=True),
            }
            res = alternate(torch, arms, args.rounds)
            copy_rate = 2 * esize * numel / res["copy"][0]  # bytes per ms
            pass_ms = (2 * esize + 8) * numel / copy_rate
            plan = f"{info['lines_per_tile']} / {info['passes']} / {info['workgroups']}"
            for arm in ("copy", "sort_dim", "torch.sort"):
                ms, lo, hi = res[arm]
                row = dict(bench="sort_dim", dtype=str(dt).split(".")[1], shape=list(shape), dim=dim, regime=regime,
                           plan=plan if arm == "sort_dim" else "", arm=arm, ms=round(ms, 4), ms_min=round(lo, 4),
                           ms_max=round(hi, 4), pass_share=round(pass_ms / ms, 3) if arm != "copy" else None,
                           copy_GBps=round(copy_rate / 1e6, 0) if arm == "copy" else None,
                           vs_torch=round(res["torch.sort"][0] / ms, 2) if arm == "sort_dim" else None,
                           equal_torch=ok if arm == "sort_dim" else None)
                rows.append(row)
                print(json.dumps(row), flush=True)
            del xs, ys
            torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("| dtype | shape | dim | regime | lines per tile / passes / workgroups | arm | "
                    "ms median [min, max] | copy GB/s | pass share | vs torch |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                cell = lambda v: "" if v is None else str(v)  # noqa: E731
                f.write(f"| {r['dtype']} | {r['shape']} | {r['dim']} | {r['regime']} | {r['plan']} | {r['arm']} | "
                        f"{r['ms']:.4f} [{r['ms_min']:.4f}, {r['ms_max']:.4f}] | {cell(r['copy_GBps'])} | "
                        f"{cell(r['pass_share'])} | {cell(r['vs_torch'])} |\n")


if __name__ == "__main__":
    main()
