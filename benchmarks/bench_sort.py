#!/usr/bin/env python3
"""GPU sort benchmark: radix (onesweep) and merge sort vs torch.sort.

    python benchmarks/bench_sort.py [--n 16777216] [--dtype uint32|int32|float32|int64|uint64|float64]
                                     [--algo radix merge] [--values | --value-bytes 0|4|8] [--descending]
                                     [--argsort] [--reps 20]

Times back-to-back calls with hipEvents (median over reps), one JSON line per
(algo, n): ms, Gkeys/s, and the "equivalent bandwidth" of a 4-pass LSD sort
(read + write of the keys per pass; BASELINE #15-16 compare against the
hw4 OpenMP sorts, hw/hw4/programming/radixsort.cpp / mergesort.cpp).

64-bit key dtypes (radix only) print, for every n, the 64-bit sort and two
comparisons taken in the same process on the same tensors with the same
timing protocol: ``torch.sort(stable=True)`` and this library's 32-bit radix
sort of the keys' low words, with 32-bit values where the 64-bit sort carries
values (the traffic model:
eight passes of 8-byte keys move four times the bytes of four passes of
4-byte keys). ``--argsort`` times ``argsort`` against
``torch.sort(stable=True).indices``; ``--kind index24`` draws keys below 2^24
(index-like keys: most passes are identity copies)."""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def _time(fn, reps: int) -> float:
    """Median hipEvent time of back-to-back calls, after three warm-up calls."""
    import torch

    for _ in range(3):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2]


def bench64(a, knobs) -> int:
    """64-bit keys: the radix sort (or argsort), torch.sort(stable=True) and
    the 32-bit radix sort at the same n, one JSON line each."""
    import torch

    from cme213x.ops.sort import argsort, sort

    dt = getattr(torch, a.dtype)
    vb = a.value_bytes if a.value_bytes is not None else (4 if a.values else 0)
    desc = a.descending
    for n in a.n:
        g = torch.Generator(device="cuda").manual_seed(1)
        if dt == torch.float64:
            x = torch.randn(n, device="cuda", generator=g, dtype=torch.float64)
        elif a.kind == "index24":
            x = torch.randint(0, 1 << 24, (n,), device="cuda", dtype=torch.int64, generator=g)
        else:
            x = torch.randint(-2**63, 2**63 - 1, (n,), device="cuda", dtype=torch.int64, generator=g)
        if a.kind == "sorted":
            x = torch.sort(x).values
        xt = x  # what torch.sort takes (no uint64 kernel: the int64 bits; its order differs, its time does not)
        if dt == torch.uint64:
            x = x.view(torch.uint64)
        v = None
        if vb:
            v = torch.arange(n, device="cuda", dtype=torch.int64 if vb == 8 else torch.int32)
        # the traffic model: the low words as 32-bit keys, 32-bit values where the 64-bit sort carries any
        x32 = xt.view(torch.int32)[::2].contiguous() if dt != torch.float64 else x.to(torch.float32)
        v32 = torch.arange(n, device="cuda", dtype=torch.int32) if (vb or a.argsort) else None
        # unsigned order = the int64 order of the keys with the top bit flipped
        flip = -2**63 if dt == torch.uint64 else 0
        ref = torch.sort(xt ^ flip if flip else xt, stable=True, descending=desc)
        if a.argsort:
            fn = lambda: argsort(x, descending=desc)  # noqa: E731
            ok = torch.equal(fn(), ref.indices)
            tfn = lambda: torch.sort(xt, stable=True, descending=desc).indices  # noqa: E731
        else:
            fn = (lambda: sort(x, v, descending=desc)) if v is not None else (lambda: sort(x, descending=desc))
            out = fn()
            keys = out[0] if isinstance(out, tuple) else out
            ok = torch.equal(keys.view(torch.int64) ^ flip if flip else keys, ref.values)
            if v is not None:
                ok = ok and torch.equal(out[1].to(torch.int64), ref.indices)
            tfn = lambda: torch.sort(xt, stable=True, descending=desc)  # noqa: E731
        del ref
        f32 = (lambda: sort(x32, v32)) if v32 is not None else (lambda: sort(x32))
        rows = [("argsort64" if a.argsort else "radix64", fn), ("torch_stable", tfn), ("radix32_model", f32)]
        res = {name: _time(f, a.reps) for name, f in rows}
        for name, _ in rows:
            ms = res[name]
            rec = {"bench": "sort", "algo": name, "n": n, "dtype": a.dtype, "value_bytes": vb, "kind": a.kind,
                   "descending": desc, "tune": knobs, "ms": round(ms, 4), "Gkeys_per_s": round(n / ms / 1e6, 2),
                   "vs_torch": round(res["torch_stable"] / ms, 2), "ok": bool(ok)}
            print(json.dumps(rec), flush=True)
    return 0


def bench_block_columns(a) -> int:
    """Preprocessing time of graph.block_columns on the hw1 PageRank graph
    (2^21 nodes, 8 edges per node) with this library's argsort and with the
    torch.sort(stable=True) it replaced, same process, same graph; then with
    the row-pointer scan as torch.cumsum and as this library's int64 scan."""
    import torch

    from cme213x.ops import graph as G
    from cme213x.ops.sort import argsort

    g = G.make_graph(1 << 21, 8).to("cuda")
    shipped = G._edge_order
    for blocks in (2, 4, 8):
        res = {}
        for name, f in (("argsort64", argsort), ("torch_stable", lambda k: torch.sort(k, stable=True).indices)):
            G._edge_order = f
            try:
                res[name] = _time(lambda: G.block_columns(g, blocks), a.reps)
            finally:
                G._edge_order = shipped
        print(json.dumps({"bench": "block_columns", "nodes": 1 << 21, "edges": g.edges.numel(), "blocks": blocks,
                          "ms_argsort64": round(res["argsort64"], 4), "ms_torch_sort": round(res["torch_stable"], 4)}),
              flush=True)
    # the row-pointer scan: the torch.cumsum it was against this library's int64
    # scan (shipped), the two forms alternated in this process, five timings of each
    # form (the spread of repeated runs of one form is what a difference
    # between the forms has to exceed)
    from cme213x.ops.scan import scan

    forms = (("torch_cumsum", lambda c, out: torch.cumsum(c, 0, out=out)),
             ("scan64", lambda c, out: scan(c, out=out)))
    shipped_rp = G._row_pointers
    runs = {name: [] for name, _ in forms}
    for _ in range(5):
        for name, f in forms:
            G._row_pointers = f
            try:
                runs[name].append(_time(lambda: G.block_columns(g, 4), a.reps))
            finally:
                G._row_pointers = shipped_rp
    rec = {"bench": "block_columns_row_pointers", "nodes": 1 << 21, "edges": g.edges.numel(), "blocks": 4}
    for name, ts in runs.items():
        ts = sorted(ts)
        rec[f"ms_{name}"] = round(ts[len(ts) // 2], 4)
        rec[f"ms_{name}_min"] = round(ts[0], 4)
        rec[f"ms_{name}_max"] = round(ts[-1], 4)
    print(json.dumps(rec), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[16 * 1024 * 1024])
    ap.add_argument("--dtype", default="uint32", choices=["uint32", "int32", "float32", "int64", "uint64", "float64"])
    ap.add_argument("--algo", nargs="+", default=["radix", "merge", "torch"])
    ap.add_argument("--values", action="store_true", help="sort (key, 32-bit value) pairs")
    ap.add_argument("--value-bytes", type=int, default=None, choices=[0, 4, 8],
                    help="bytes per value (8: 64-bit keys only); --values means 4")
    ap.add_argument("--descending", action="store_true")
    ap.add_argument("--argsort", action="store_true", help="time argsort (64-bit key dtypes)")
    ap.add_argument("--block-columns", action="store_true",
                    help="time graph.block_columns (2^21-node PageRank graph) with argsort and with torch.sort")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--kind", default="random", choices=["random", "small", "sorted", "index24"],
                    help="random: uniform 32-bit keys; small: keys < 2^16 (the high digits all zero); sorted; "
                         "index24: 64-bit keys < 2^24")
    ap.add_argument("--tune", nargs="*", default=[],
                    help="tuning knobs name=value (cme213x.utils.tuning), e.g. radix_ds=10")
    a = ap.parse_args()

    import torch

    import cme213x  # noqa: F401
    from cme213x.ops.sort import sort
    from cme213x.utils import tuning

    knobs = {kv.split("=")[0]: int(kv.split("=")[1]) for kv in a.tune}
    for k, val in knobs.items():
        tuning.set(k, val)

    if a.block_columns:
        return bench_block_columns(a)
    if a.dtype in ("int64", "uint64", "float64"):
        return bench64(a, knobs)
    if a.value_bytes == 8 or a.argsort or a.kind == "index24":
        ap.error("--value-bytes 8, --argsort and --kind index24 go with the 64-bit key dtypes")
    a.values = a.values or a.value_bytes == 4
    desc = a.descending
    dt = getattr(torch, a.dtype)
    for n in a.n:
        g = torch.Generator(device="cuda").manual_seed(1)
        if dt == torch.float32:
            x = torch.randn(n, device="cuda", generator=g)
        else:
            x = torch.randint(0, 2**31 - 1, (n,), device="cuda", dtype=torch.int64, generator=g)
            x = (x * 2 + (x & 1)).to(torch.int64) if dt == torch.uint32 else x - 2**30
            if a.kind == "small":
                x = x % 65536
            x = x.to(torch.int32).view(dt) if dt == torch.uint32 else x.to(dt)
        if a.kind == "sorted":
            x = torch.sort(x.to(torch.int64) if dt == torch.uint32 else x).values.to(x.dtype)
            x = x.view(dt) if dt == torch.uint32 else x
        v = torch.arange(n, device="cuda", dtype=torch.int32) if a.values else None
        ref = torch.sort(x.to(torch.int64) if dt == torch.uint32 else x, descending=desc).values
        for algo in a.algo:
            if algo == "torch":
                if dt == torch.uint32:
                    continue  # torch.sort has no uint32 kernel on ROCm
                fn = lambda: torch.sort(x, descending=desc)  # noqa: E731
            else:
                fn = ((lambda al=algo: sort(x, v, algo=al, descending=desc)) if v is not None else
                      (lambda al=algo: sort(x, algo=al, descending=desc)))
            out = fn()
            keys = out[0] if isinstance(out, tuple) else out
            ok = torch.equal(keys.to(torch.int64) if dt == torch.uint32 else keys, ref)
            ms = _time(fn, a.reps)
            rec = {"bench": "sort", "algo": algo, "n": n, "dtype": a.dtype, "values": a.values, "kind": a.kind,
                   "descending": desc, "tune": knobs, "ms": round(ms, 4),
                   "Gkeys_per_s": round(n / ms / 1e6, 2),
                   "eq_TBps_4pass": round(n * 4 * (2 if a.values else 1) * 2 * 4 / ms / 1e9, 2), "ok": ok}
            print(json.dumps(rec), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
