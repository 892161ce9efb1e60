"""bincount(x, nbins=) against torch.bincount on one GPU, every regime forced.

    python benchmarks/bench_bincount.py [--rounds 5] [--out table.md] [--only SUBSTRING]
    python benchmarks/bench_bincount.py --block-columns

The project's convention (benchmarks/bench_sort_dim.py): three operand sets per
row (cache-defeated: every set is 256 MiB or more), the arms alternated call
by call in one process in an order reshuffled every round, one event pair per
call; median [min, max] ms. Arms: this bincount as the rule runs it ("auto")
and with each regime forced that can run the row (lds, window up to 64
windows, global, sorted), torch.bincount, histogram_dense(sort(x, key_bits=)),
text.histogram_u8 on the byte row, and the flattened scan.reduce(x, "max")
over the same bytes, the read-rate yardstick of profiles/reduce_dim.md: "read
share" is the yardstick's time over the arm's. The global rows also give the
rate of integer global atomics (adds per second; 8 bytes each). Every arm's
counts are compared with torch.bincount before timing.

--block-columns: graph.block_columns on the 2^21-node PageRank graph (4
blocks) with the edge counts from torch.bincount and from this bincount, the
two forms alternated, five timings of each."""
import argparse
import json
import os
import random
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

REGIMES = {"lds": 1, "window": 2, "global": 3, "sorted": 4}


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


def rows_of(torch, W):
    """(dtype, n, nbins, kind, what)"""
    out = []
    for dt in (torch.int32, torch.int64):
        for nbins in (256, 4096, W, 4 * W, 8 * W, 16 * W, 32 * W, 1 << 20, 1 << 23):
            out.append((dt, 1 << 26, nbins, "uniform", f"{nbins} bins"))
        out.append((dt, 1 << 26, 256, "sorted", "256 bins, sorted"))
        out.append((dt, 1 << 26, 256, "equal", "256 bins, all equal"))
    out.append((torch.uint8, 1 << 28, 256, "uniform", "bytes, 256 bins"))
    out.append((torch.int64, 0, 4 << 21, "block_columns", "block_columns keys (2^21 nodes, 4 blocks)"))
    return out


def operands(torch, dev, dt, n, nbins, kind):
    if kind == "block_columns":
        from cme213x.ops import graph as G

        g = G.make_graph(1 << 21, 8).to(dev)
        nn = g.n
        deg = (g.indices[1:] - g.indices[:-1]).to(torch.int64)
        row = torch.repeat_interleave(torch.arange(nn, device=dev), deg)
        key = (g.edges.to(torch.int64) // ((nn + 3) // 4)) * nn + row
        return [key, key.clone(), key.clone()]
    xs = []
    for s in range(3):
        g = torch.Generator(device=dev).manual_seed(s)
        if kind == "equal":
            x = torch.full((n,), nbins // 3, dtype=dt, device=dev)
        else:
            x = torch.randint(0, nbins, (n,), generator=g, device=dev, dtype=torch.int64 if dt != torch.uint8 else dt)
            x = x.to(dt)
            if kind == "sorted":
                x = torch.sort(x).values
        xs.append(x)
    return xs


def bench_rows(args) -> int:
    import torch

    import cme213x  # noqa: F401
    from cme213x.ops import text
    from cme213x.ops.algorithms import bincount, bincount_launch_info, histogram_dense
    from cme213x.ops.scan import reduce
    from cme213x.ops.sort import sort
    from cme213x.utils import tuning

    dev = torch.device("cuda:0")
    W = bincount_launch_info(1 << 26, 16, device=dev)["window"]
    rows = []
    for dt, n, nbins, kind, what in rows_of(torch, W):
        if args.only and args.only not in what:
            continue
        xs = operands(torch, dev, dt, n, nbins, kind)
        n = xs[0].numel()
        name = str(dt).split(".")[1]
        auto = bincount_launch_info(n, nbins, dtype=dt, device=dev)
        ref = torch.bincount(xs[0], minlength=nbins)

        def forced(code):
            def f(i):
                with tuning.override(bincount_regime=code):
                    return bincount(xs[i], nbins=nbins)
            return f

        arms = {"auto": lambda i: bincount(xs[i], nbins=nbins),
                "torch.bincount": lambda i: torch.bincount(xs[i], minlength=nbins)}
        if nbins <= W:
            arms["lds"] = forced(REGIMES["lds"])
        elif (nbins + W - 1) // W <= 64:
            arms["window"] = forced(REGIMES["window"])
        arms["global"] = forced(REGIMES["global"])
        if dt != torch.uint8:
            bits = max(1, (nbins - 1).bit_length())
            arms["sorted"] = forced(REGIMES["sorted"])
            arms["hist_dense(sort)"] = lambda i: histogram_dense(sort(xs[i], key_bits=bits), nbins)
            arms["reduce max"] = lambda i: reduce(xs[i], "max")
        else:
            arms["text.histogram_u8"] = lambda i: text.histogram_u8(xs[i], 0, 256)
            x32 = [x.view(torch.int32) for x in xs]
            arms["reduce max"] = lambda i: reduce(x32[i], "max")
        ok = {a: bool(torch.equal(f(0).to(torch.int64), ref)) for a, f in arms.items() if a != "reduce max"}
        res = alternate(torch, arms, args.rounds)
        yard = res["reduce max"][0]
        for arm, (ms, lo, hi) in res.items():
            row = dict(bench="bincount", dtype=name, n=n, nbins=nbins, data=kind, what=what,
                       rule=auto["regime"] if arm == "auto" else "", arm=arm, ms=round(ms, 4), ms_min=round(lo, 4),
                       ms_max=round(hi, 4), read_share=round(yard / ms, 3),
                       read_GBps=round(n * xs[0].element_size() / ms / 1e6, 0) if arm == "reduce max" else None,
                       vs_torch=round(res["torch.bincount"][0] / ms, 2),
                       Gadds_per_s=round(n / ms / 1e6, 2) if arm == "global" else None, equal_torch=ok.get(arm))
            rows.append(row)
            print(json.dumps(row), flush=True)
        del xs, ref
        torch.cuda.empty_cache()
    if args.out:
        with open(args.out, "w") as f:
            f.write("| dtype | n | row | arm | rule | ms median [min, max] | read share | vs torch.bincount | "
                    "Gadds/s | equal |\n|---|---|---|---|---|---|---|---|---|---|\n")
            for r in rows:
                cell = lambda v: "" if v is None else str(v)  # noqa: E731
                f.write(f"| {r['dtype']} | {r['n']} | {r['what']} | {r['arm']} | {r['rule']} | "
                        f"{r['ms']:.4f} [{r['ms_min']:.4f}, {r['ms_max']:.4f}] | {r['read_share']} | {r['vs_torch']} | "
                        f"{cell(r['Gadds_per_s'])} | {cell(r['equal_torch'])} |\n")
    return 0


def _time(torch, f, reps):
    f()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def bench_block_columns(args) -> int:
    import torch

    import cme213x  # noqa: F401
    from cme213x.ops import graph as G
    from cme213x.ops.algorithms import bincount

    g = G.make_graph(1 << 21, 8).to("cuda")
    forms = (("torch_bincount", lambda key, nbins: torch.bincount(key, minlength=nbins)),
             ("bincount", lambda key, nbins: bincount(key, nbins=nbins)))
    shipped = G._edge_counts
    runs = {name: [] for name, _ in forms}
    same = None
    for _ in range(5):
        for name, f in forms:
            G._edge_counts = f
            try:
                runs[name].append(_time(torch, lambda: G.block_columns(g, 4), args.reps))
                rp = G.block_columns(g, 4).rp
                same = rp if same is None else same
                assert torch.equal(rp, same)
            finally:
                G._edge_counts = shipped
    rec = {"bench": "block_columns_edge_counts", "nodes": 1 << 21, "edges": g.edges.numel(), "blocks": 4}
    for name, ts in runs.items():
        ts = sorted(ts)
        rec[f"ms_{name}"] = round(ts[len(ts) // 2], 4)
        rec[f"ms_{name}_min"] = round(ts[0], 4)
        rec[f"ms_{name}_max"] = round(ts[-1], 4)
    print(json.dumps(rec), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="substring of a row's description")
    ap.add_argument("--block-columns", action="store_true",
                    help="time graph.block_columns with torch.bincount and with this bincount")
    args = ap.parse_args()
    return bench_block_columns(args) if args.block_columns else bench_rows(args)


if __name__ == "__main__":
    sys.exit(main())
