#!/usr/bin/env python3
"""Single-GPU benchmarks for the BASELINE.md headline primitives. One JSON line
per measurement with the reference number it is compared against.

  copy       1 GiB 16-B copy (achievable-HBM calibration)
  scan       2^26 elements: look-back / Blelloch / Hillis-Steele (BASELINE #11)
  reduce     2^26 elements
  scan64     int64 / float64 scans and sums at 2^25 and 2^27 against the copy
             rate of the same run (profiles/scan64_r8.md)
  scan_minmax  running max (cummax) by look-back and reduce-then-scan against the
             sum look-back, torch.cummax and the copy of the same run, float32 /
             int32 / int64 / float64 at 2^25 and 2^27 (profiles/scan_minmax.md)
  scan_dim   scans along one dimension, one shape per regime, float32 / int64,
             against torch.cumsum(x, dim) and the copy of the same run
             (profiles/scan_dim.md)
  scan_arg   cummax with indices along a dimension and flattened, float32 / int64,
             against the values-only scan, torch.cummax and the copy of the same
             run (profiles/scan_cumarg.md)
  reduce_dim sum / max / max with indices along one dimension, one shape per
             regime, float32 / int64, against torch.sum / amax / max(x, dim) and
             the flattened reduce of the same run (profiles/reduce_dim.md)
  spmvscan   the 15 final-project shapes (BASELINE #19-21, synthetic values)
  cipher     19.76 MB moby-dick x16 (BASELINE #1-3)
  pagerank   2^21 nodes, avg 8 edges, 20 iterations (BASELINE #5)
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


SINGLE = {}  # last measurement's one-call-per-event-pair median (ms)


def timeit(fn, iters=10, warmup=2):
    """Median ms per call. Each event pair brackets one call; when that call
    is short (< 0.2 ms) the pair brackets max(2, 0.2 ms / t) back-to-back calls
    instead and the time is divided by their count, so the host's per-call
    Python/launch latency (~5-10 us, box-dependent) and the idle-clock ramp
    between isolated calls do not masquerade as kernel time. The one-call
    median stays in SINGLE["ms"] (emitted as ms_single)."""
    import torch

    def med(reps):
        ts = []
        for _ in range(iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1) / reps)
        ts.sort()
        return ts[len(ts) // 2]

    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    single = med(1)
    SINGLE["ms"] = single
    if single >= 0.2:
        return single
    return min(single, med(max(2, min(100, int(0.2 / max(single, 1e-4))))))


def emit(**kw):
    single = SINGLE.pop("ms", None)
    if single is not None and "ms" in kw and single != kw["ms"]:
        kw["ms_single"] = single
    print(json.dumps(kw), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    args = ap.parse_args()
    import numpy as np
    import torch

    import cme213x
    from cme213x.ops import elementwise, scan as sc

    want = lambda k: args.only is None or k in args.only  # noqa: E731
    dev = torch.device("cuda")

    if want("copy"):
        a = torch.empty(1 << 28, dtype=torch.float32, device=dev).uniform_()
        b = torch.empty_like(a)
        ms = timeit(lambda: elementwise.copy_(b, a))
        emit(bench="copy", bytes=2 * a.numel() * 4, ms=ms, GBps=2 * a.numel() * 4 / ms / 1e6)
        ms = timeit(lambda: b.copy_(a))
        emit(bench="copy_torch", bytes=2 * a.numel() * 4, ms=ms, GBps=2 * a.numel() * 4 / ms / 1e6)
        del a, b

    if want("scan"):
        n = 1 << 26
        x = torch.rand(n, device=dev)
        y = torch.empty_like(x)
        for algo in ("lookback", "rts", "blelloch", "hillis", "blelloch_mlevel", "hillis_mlevel"):
            ms = timeit(lambda: sc.scan(x, True, y, algo))
            emit(bench="scan", algo=algo, n=n, ms=ms, GBps=8 * n / ms / 1e6, ref_ms=15.85,
                 speedup_vs_ref=15.85 / ms)
        ms = timeit(lambda: torch.cumsum(x, 0, out=y))
        emit(bench="scan", algo="torch.cumsum", n=n, ms=ms, GBps=8 * n / ms / 1e6)
        xi = torch.randint(0, 100, (n,), device=dev, dtype=torch.int32)
        yi = torch.empty_like(xi)
        for algo in ("lookback", "rts"):
            ms = timeit(lambda: sc.scan(xi, True, yi, algo))
            emit(bench="scan", algo=f"{algo}-int32", n=n, ms=ms, GBps=8 * n / ms / 1e6)
        for algo in ("vector", "tree"):
            ms = timeit(lambda: sc.reduce(x, "sum", algo))
            emit(bench="reduce", algo=algo, n=n, ms=ms, GBps=4 * n / ms / 1e6)
        ms = timeit(lambda: x.sum())
        emit(bench="reduce", algo="torch.sum", n=n, ms=ms, GBps=4 * n / ms / 1e6)
        del x, y, xi, yi

    # The arms of one (dtype, size) alternate call by call in this process (in
    # an order reshuffled every round); every call of an arm takes the next of
    # three operand sets. Returns {arm: (median, min, max) ms}.
    def alternate(arms, rounds=12, warm=2):
        import random

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

    if want("scan64"):
        # int64 / float64 at 2^25 and 2^27: the arms of one (dtype, size)
        # alternate call by call in this process (in an order reshuffled every
        # round), every call of an arm takes the next of three operand sets
        # (cache-defeated: 3 x 16 B x n is far past the 256 MB Infinity Cache at
        # both sizes) and the copy of the same operands is one of the arms, so
        # every share is against the copy rate of the same run.
        for dt in (torch.int64, torch.float64):
            for n in (1 << 25, 1 << 27):
                if dt == torch.int64:
                    xs = [torch.randint(-2 ** 40, 2 ** 40, (n,), device=dev, dtype=dt) for _ in range(3)]
                else:
                    xs = [torch.rand(n, device=dev, dtype=dt) for _ in range(3)]
                ys = [torch.empty_like(x) for x in xs]
                arms = {
                    "copy": lambda k: ys[k].copy_(xs[k]),
                    "rts": lambda k: sc.scan(xs[k], True, ys[k], "rts"),
                    "lookback": lambda k: sc.scan(xs[k], True, ys[k], "lookback"),
                    "torch.cumsum": lambda k: torch.cumsum(xs[k], 0, out=ys[k]),
                    "reduce": lambda k: sc.reduce(xs[k], "sum"),
                    "torch.sum": lambda k: xs[k].sum(),
                }
                res = alternate(arms)
                copy_bps = 16 * n / res["copy"][0] / 1e6
                for name, (ms, lo, hi) in res.items():
                    per = 8 if name in ("reduce", "torch.sum") else 16  # bytes per element of the model
                    emit(bench="scan64", dtype=str(dt).split(".")[1], n=n, arm=name, ms=round(ms, 4),
                         ms_min=round(lo, 4), ms_max=round(hi, 4), model_B_per_elem=per,
                         GBps=round(per * n / ms / 1e6, 1), share_of_copy=round(per * n / ms / 1e6 / copy_bps, 3))
                sc.check_lookback(dev)
                del xs, ys, arms

    if want("scan_minmax"):
        # Running max by both algorithms against the SUM look-back of the same
        # dtype (the same bytes through the same schedule), torch.cummax (which
        # also writes an int64 index per element) and the copy of the same
        # operands; measured like scan64: three cache-defeated operand sets (3 x
        # 8 B x 2^25 is past the 256 MB Infinity Cache), arms alternated. Noisy
        # ramps, so the running max changes all along. `ok`: the max look-back
        # is no slower than the sum look-back by more than the spread (max -
        # min) the sum arm itself shows in this run.
        for dt in (torch.float32, torch.int32, torch.int64, torch.float64):
            for n in (1 << 25, 1 << 27):
                ramp = torch.arange(n, device=dev, dtype=torch.int64)
                xs = [(ramp + torch.randint(-50, 51, (n,), device=dev)).to(dt) for _ in range(3)]
                del ramp
                ys = [torch.empty_like(x) for x in xs]
                arms = {
                    "copy": lambda k: ys[k].copy_(xs[k]),
                    "max-lookback": lambda k: sc.scan(xs[k], False, ys[k], "lookback", "max"),
                    "max-rts": lambda k: sc.scan(xs[k], False, ys[k], "rts", "max"),
                    "sum-lookback": lambda k: sc.scan(xs[k], False, ys[k], "lookback"),
                    "torch.cummax": lambda k: torch.cummax(xs[k], 0),
                }
                res = alternate(arms)
                size = xs[0].element_size()
                copy_bps = 2 * size * n / res["copy"][0] / 1e6
                sum_ms, sum_lo, sum_hi = res["sum-lookback"]
                for name, (ms, lo, hi) in res.items():
                    extra = {}
                    if name == "max-lookback":
                        extra = dict(sum_ms=round(sum_ms, 4), sum_spread_ms=round(sum_hi - sum_lo, 4),
                                     ok=bool(ms <= sum_ms + (sum_hi - sum_lo)))
                    emit(bench="scan_minmax", dtype=str(dt).split(".")[1], n=n, arm=name, ms=round(ms, 4),
                         ms_min=round(lo, 4), ms_max=round(hi, 4), model_B_per_elem=2 * size,
                         GBps=round(2 * size * n / ms / 1e6, 1),
                         share_of_copy=round(2 * size * n / ms / 1e6 / copy_bps, 3), **extra)
                sc.check_lookback(dev)
                del xs, ys, arms

    if want("scan_dim"):
        # Scans along one dimension, one shape per regime of csrc/hip/
        # scan_dim.hip, against torch.cumsum(x, dim) and the copy of the same
        # operands; measured like scan64 (three operand sets, arms alternated,
        # every share against the copy of the same run). One max arm against
        # torch.cummax. `ok`: our time does not exceed torch.cumsum's by more
        # than the larger spread (max - min) the two arms show in this run.
        shapes = [((65536, 2048), -1, "row, K == 1"), ((1 << 20, 64), -1, "row, short rows"),
                  ((16, 1 << 22), -1, "row, K > 1"), ((8192, 8192), 0, "column, wide"),
                  ((1 << 21, 64), 0, "column, tall and thin, K > 1"), ((64, 1 << 21), 0, "column, short and wide"),
                  ((256, 512, 512), 1, "column"), ((1 << 22, 3), 0, "column, narrow")]
        for dt in (torch.float32, torch.int64):
            for shape, dim, regime in shapes:
                if dt == torch.int64:
                    xs = [torch.randint(-2 ** 40, 2 ** 40, shape, device=dev, dtype=dt) for _ in range(3)]
                else:
                    xs = [torch.rand(shape, device=dev, dtype=dt) for _ in range(3)]
                ys = [torch.empty_like(x) for x in xs]
                arms = {
                    "copy": lambda k: ys[k].copy_(xs[k]),
                    "scan_dim": lambda k: sc.scan(xs[k], out=ys[k], dim=dim),
                    "torch.cumsum": lambda k: torch.cumsum(xs[k], dim, out=ys[k]),
                }
                if dt == torch.float32 and regime == "row, K == 1":
                    arms["scan_dim-max"] = lambda k: sc.scan(xs[k], out=ys[k], op="max", dim=dim)
                    arms["torch.cummax"] = lambda k: torch.cummax(xs[k], dim)
                res = alternate(arms, rounds=8)
                size, n = xs[0].element_size(), xs[0].numel()
                info = sc.scan_dim_launch_info(shape, dim, dtype=dt, device=dev)
                copy_bps = 2 * size * n / res["copy"][0] / 1e6
                t_ms, t_lo, t_hi = res["torch.cumsum"]
                for name, (ms, lo, hi) in res.items():
                    extra = {}
                    if name == "scan_dim":
                        spread = max(hi - lo, t_hi - t_lo)
                        extra = dict(form=info["form"], chunks=info["chunks"], vector=info["vector"],
                                     workgroups=info["workgroups"], torch_ms=round(t_ms, 4),
                                     spread_ms=round(spread, 4), ok=bool(ms <= t_ms + spread))
                    emit(bench="scan_dim", dtype=str(dt).split(".")[1], shape=list(shape), dim=dim, regime=regime,
                         arm=name, ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                         model_B_per_elem=2 * size, GBps=round(2 * size * n / ms / 1e6, 1),
                         share_of_copy=round(2 * size * n / ms / 1e6 / copy_bps, 3), **extra)
                del xs, ys, arms

    if want("scan_arg"):
        # cummax with indices (csrc/hip/scan_dim_arg.hip) against the values-only
        # scan along the same dimension, torch.cummax (values and indices, as
        # ours) and the copy of the same values; measured like scan_dim (three
        # operand sets, arms alternated and reshuffled, an event pair per call).
        # The byte bound: the indexed scan moves 2 * esize + 8 bytes per element
        # in a single pass and 3 * esize + 8 when chunked, the copy 2 * esize;
        # `pct_of_bound` is that bound at the copy rate of the same run over our
        # time. `ok`: our median does not exceed torch.cummax's by more than the
        # larger spread (max - min) the two arms show in this run. Plateau data
        # (values in 0..15): the index moves while the value stands still.
        shapes = [((1 << 25,), None, "1-D"), ((1 << 27,), None, "1-D"), ((65536, 2048), -1, "row, K == 1"),
                  ((1 << 20, 64), -1, "row, short rows"), ((16, 1 << 22), -1, "row, K > 1"),
                  ((8192, 8192), 0, "column, wide"), ((256, 512, 512), 1, "column"),
                  ((64, 1 << 21), 0, "column, short and wide")]
        for dt in (torch.float32, torch.int64):
            for shape, dim, regime in shapes:
                xs = [torch.randint(0, 16, shape, device=dev).to(dt) for _ in range(3)]
                ys = [torch.empty_like(x) for x in xs]
                idx = [torch.empty(shape, dtype=torch.int64, device=dev) for _ in range(3)]
                tdim = 0 if dim is None else dim
                arms = {
                    "copy": lambda k: ys[k].copy_(xs[k]),
                    "scan_dim-max": lambda k: sc.scan(xs[k], out=ys[k], op="max", dim=tdim),
                    "cummax+indices": lambda k: sc.cummax(xs[k], dim=dim, return_indices=True, out=(ys[k], idx[k])),
                }
                torch_arm = lambda k: torch.cummax(xs[k], tdim, out=(ys[k], idx[k]))  # noqa: E731
                if dim is None:
                    # torch.cummax takes about 0.4 s per call on the 1-D shapes: fewer rounds, with
                    # our arm alternating beside it (its reading of the main run is the one reported)
                    res = alternate(arms, rounds=8)
                    few = alternate({"torch.cummax": torch_arm, "ours": arms["cummax+indices"]}, rounds=3, warm=1)
                    res["torch.cummax"] = few["torch.cummax"]
                else:
                    arms["torch.cummax"] = torch_arm
                    res = alternate(arms, rounds=8)
                size, n = xs[0].element_size(), xs[0].numel()
                info = sc.scan_dim_launch_info(shape, tdim, dtype=dt, op="max", device=dev, indices=True)
                copy_bps = 2 * size * n / res["copy"][0] / 1e6
                per = (2 if info["chunks"] == 1 else 3) * size + 8
                t_ms, t_lo, t_hi = res["torch.cummax"]
                for name, (ms, lo, hi) in res.items():
                    extra = {}
                    if name == "cummax+indices":
                        spread = max(hi - lo, t_hi - t_lo)
                        extra = dict(form=info["form"], chunks=info["chunks"], tile=info["tile"], vector=info["vector"],
                                     waves=info["waves"], workgroups=info["workgroups"], ws_bytes=info["ws_bytes"],
                                     bound_B_per_elem=per, pct_of_bound=round(100 * per * n / copy_bps / 1e6 / ms, 1),
                                     torch_ms=round(t_ms, 4), spread_ms=round(spread, 4), ok=bool(ms <= t_ms + spread))
                    emit(bench="scan_arg", dtype=str(dt).split(".")[1], shape=list(shape), dim=dim, regime=regime,
                         arm=name, ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                         GBps=round((2 * size + (0 if name in ("copy", "scan_dim-max") else 8)) * n / ms / 1e6, 1),
                         **extra)
                del xs, ys, idx, arms

    if want("reduce_dim"):
        # Reductions along one dimension (csrc/hip/reduce_dim.hip), one shape per
        # regime of the scan_dim table: sum, max, and max with indices against
        # torch.sum / torch.amax / torch.max(x, dim), and against the flattened
        # reduce of this project over the same bytes -- the read-rate yardstick
        # of the same run. Measured like scan_dim: three operand sets, arms
        # alternated and reshuffled, an event pair per call. `read_share`: the
        # yardstick's time over the arm's; `vs_torch`: torch's time over ours.
        shapes = [((65536, 2048), -1, "row, K == 1"), ((1 << 20, 64), -1, "row, short rows"),
                  ((16, 1 << 22), -1, "row, K > 1"), ((1 << 27,), 0, "one line"), ((8192, 8192), 0, "column, wide"),
                  ((1 << 21, 64), 0, "column, tall and thin, K > 1"), ((64, 1 << 21), 0, "column, short and wide"),
                  ((256, 512, 512), 1, "column"), ((1 << 22, 3), 0, "column, narrow")]
        for dt in (torch.float32, torch.int64):
            for shape, dim, regime in shapes:
                if dt == torch.int64:
                    xs = [torch.randint(-2 ** 40, 2 ** 40, shape, device=dev, dtype=dt) for _ in range(3)]
                else:
                    xs = [torch.rand(shape, device=dev, dtype=dt) for _ in range(3)]
                pairs = {"reduce_dim-sum": "torch.sum", "reduce_dim-max": "torch.amax",
                         "reduce_dim-max+indices": "torch.max"}
                arms = {
                    "reduce-flat": lambda k: sc.reduce(xs[k].view(-1), "sum"),
                    "reduce_dim-sum": lambda k: sc.reduce(xs[k], "sum", dim=dim),
                    "torch.sum": lambda k: torch.sum(xs[k], dim),
                    "reduce_dim-max": lambda k: sc.reduce(xs[k], "max", dim=dim),
                    "torch.amax": lambda k: torch.amax(xs[k], dim),
                    "reduce_dim-max+indices": lambda k: sc.reduce(xs[k], "max", dim=dim, return_indices=True),
                    "torch.max": lambda k: torch.max(xs[k], dim),
                }
                res = alternate(arms, rounds=8)
                size, n = xs[0].element_size(), xs[0].numel()
                flat_ms = res["reduce-flat"][0]
                for name, (ms, lo, hi) in res.items():
                    extra = {}
                    if name in pairs:
                        info = sc.reduce_dim_launch_info(shape, dim, dtype=dt, op="max", device=dev,
                                                         indices=name.endswith("indices"))
                        t_ms, t_lo, t_hi = res[pairs[name]]
                        extra = dict(form=info["form"], chunks=info["chunks"], vector=info["vector"], waves=info["waves"],
                                     workgroups=info["workgroups"], ws_bytes=info["ws_bytes"], torch_ms=round(t_ms, 4),
                                     vs_torch=round(t_ms / ms, 2), spread_ms=round(max(hi - lo, t_hi - t_lo), 4))
                    emit(bench="reduce_dim", dtype=str(dt).split(".")[1], shape=list(shape), dim=dim, regime=regime,
                         arm=name, ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
                         GBps=round(size * n / ms / 1e6, 1), read_share=round(flat_ms / ms, 3), **extra)
                del xs, arms

    if want("spmvscan"):
        from cme213x.models.spmv_scan import BENCH_SHAPES, REF_MS, SpmvScanSolver, generate

        for name, (n, p, N) in BENCH_SHAPES.items():
            prob = generate(n, p, 100000, N, seed=1)
            sol = SpmvScanSolver(prob, dev)
            sol.run(2)
            ms = timeit(lambda: sol.run(), iters=5, warmup=1)
            emit(bench="spmvscan", matrix=name, n=n, p=p, N=N, ms=ms, GBps=12 * n * N / ms / 1e6,
                 ref_ms=REF_MS[name], speedup_vs_ref=REF_MS[name] / ms)
            # the same N-iteration loop replayed as one hipGraph
            from cme213x.utils.graphs import GraphRunner

            g = GraphRunner(lambda: sol.run())
            ms = timeit(g, iters=5, warmup=1)
            emit(bench="spmvscan_graph", matrix=name, n=n, p=p, N=N, ms=ms, GBps=12 * n * N / ms / 1e6,
                 ref_ms=REF_MS[name], speedup_vs_ref=REF_MS[name] / ms)

    if want("spmvscan_algos"):
        from cme213x.models.spmv_scan import BENCH_SHAPES, REF_MS, SpmvScanSolver, generate

        for name in ("dense2", "mac_econ_fwd500", "webbase-1M", "mc2depi"):
            n, p, N = BENCH_SHAPES[name]
            prob = generate(n, p, 100000, N, seed=1)
            for algo in ("lookback", "wave", "serial"):
                sol = SpmvScanSolver(prob, dev, algo)
                sol.run(1)
                ms = timeit(lambda: sol.run(), iters=3, warmup=1)
                emit(bench="spmvscan_algo", matrix=name, algo=algo, n=n, p=p, N=N, ms=ms,
                     GBps=12 * n * N / ms / 1e6, ref_ms=REF_MS[name], speedup_vs_ref=REF_MS[name] / ms)
                del sol

    if want("algorithms"):
        bench_algorithms(emit, timeit)

    if want("cipher"):
        path = "/root/reference/hw/hw1/programming/mobydick.txt"
        text = np.fromfile(path, dtype=np.uint8) if os.path.exists(path) else \
            np.random.default_rng(0).integers(0, 128, 1235150, dtype=np.uint8)
        for copies in (16, 208):
            d = torch.from_numpy(np.tile(text, copies)).to(dev)
            o = torch.empty_like(d)
            for w in ("char", "uint", "uint2", "uint4"):
                ms = timeit(lambda: elementwise.shift_cipher(d, 3, o, width=w))
                emit(bench="cipher", width=w, bytes=d.numel(), ms=ms, GBps_rw=2 * d.numel() / ms / 1e6)

    if want("transpose"):
        bench_transpose(emit, timeit)

    if want("spmv"):
        bench_spmv(emit, timeit)

    if want("sort"):
        bench_sort(emit, timeit)

    if want("vigenere"):
        bench_vigenere(emit, timeit)

    if want("gemm"):
        bench_gemm(emit, timeit)

    if want("misc"):
        bench_misc(emit, timeit)

    if want("pagerank"):
        from cme213x.ops.graph import bytes_model, iterate, make_graph

        g = make_graph(1 << 21, 8).to(dev)
        x0 = torch.full((1 << 21,), 1.0 / (1 << 21), device=dev)
        for grp in (1, 4, 8, 16):
            ms = timeit(lambda: iterate(g, x0, 20, grp))
            emit(bench="pagerank", group=grp, ms=ms, GBps_model=bytes_model(g, 20) / ms / 1e6, ref_ms=1188.11,
                 speedup_vs_ref=1188.11 / ms)
        from cme213x.ops.graph import block_columns

        for blocks in (2, 4, 8):
            bg = block_columns(g, blocks)
            for grp in (1, 2, 4):
                ms = timeit(lambda: iterate(bg, x0, 20, grp))
                emit(bench="pagerank", blocks=blocks, group=grp, ms=ms, GBps_model=bytes_model(g, 20) / ms / 1e6,
                     ref_ms=1188.11, speedup_vs_ref=1188.11 / ms)


def bench_transpose(emit, timeit):
    import torch

    from cme213x.ops.transpose import VARIANTS, transpose

    from cme213x.ops.transpose import DIAGNOSTICS, diagnostic, transpose_reps

    ref = {8192: None, 4096: 130.0, 2048: 128.0}  # BASELINE #7/#8 best (LDS+pad+unroll, Fermi)
    for n in (8192, 4096, 2048):
        x = torch.rand(n, n, device="cuda")
        out = torch.empty_like(x)
        for v in VARIANTS:
            ms = timeit(lambda: transpose(x, v, out))
            gbps = 2 * n * n * 4 / ms / 1e6
            emit(bench="transpose", n=n, variant=v, ms=ms, GBps=gbps, ref_GBps=ref[n],
                 vs_ref=(gbps / ref[n]) if ref[n] else None)
        for d in DIAGNOSTICS:
            ms = timeit(lambda: diagnostic(x, d, out))
            emit(bench="transpose_diag", n=n, kind=d, ms=ms, GBps=2 * n * n * 4 / ms / 1e6)
        # the paper's two timing modes for the same kernel (lds_pad)
        reps = 20
        ms = timeit(lambda: transpose_reps(x, reps, out)) / reps
        SINGLE.pop("ms", None)
        emit(bench="transpose_timing_mode", n=n, mode="loop inside kernel", ms=ms, GBps=2 * n * n * 4 / ms / 1e6)


def bench_spmv(emit, timeit):
    import torch

    from cme213x.ops.spmv import laplacian, random_csr, spmv, to_coo, to_csr_aligned, to_dia, to_ell, to_hyb

    mats = {"5pt-1M": laplacian("5pt", 1000), "27pt-1M": laplacian("27pt", 100),
            "random-1M": random_csr(1 << 20, 1 << 20, 16, seed=1), "skew-1M": random_csr(1 << 20, 1 << 20, 16,
                                                                                             seed=2, skew=True)}
    for name, a in mats.items():
        x = torch.rand(a.ncols, device="cuda")
        fmts = {"csr_scalar": a, "csr_vector": a, "csr_aligned": to_csr_aligned(a), "coo": to_coo(a),
                "hyb": to_hyb(a)}
        if int((a.rp[1:] - a.rp[:-1]).max()) <= 64:
            fmts["ell"] = to_ell(a)[0]
        if name.startswith(("5pt", "27pt")):
            fmts["dia"] = to_dia(a)
        for f, m in fmts.items():
            md = m.to("cuda")
            y = torch.empty(a.nrows, device="cuda")
            kern = "scalar" if f == "csr_scalar" else "auto"
            ms = timeit(lambda: spmv(md, x, y, kernel=kern), iters=20)
            # Bell & Garland GTX 285: 27-pt DIA 39.6 GFLOP/s; best unstructured HYB 24.2
            ref = 39.6 if (name.startswith("27pt") and f == "dia") else (24.2 if f == "hyb" and name == "random-1M" else None)
            emit(bench="spmv", matrix=name, fmt=f, nnz=a.nnz, ms=ms, GFLOPs=2 * a.nnz / ms / 1e6, ref_GFLOPs=ref,
                 vs_ref=(2 * a.nnz / ms / 1e6 / ref) if ref else None)


def bench_sort(emit, timeit):
    import torch

    from cme213x.ops.sort import sort

    for n, ref_s, ref_name in ((16_000_000, 0.084, "radix 16M keys, 32 OpenMP threads (BASELINE #16)"),
                               (48_000_000, 0.617, "merge sort 48M ints, 32 threads (BASELINE #15)")):
        x = torch.randint(0, 2**31 - 1, (n,), dtype=torch.int32, device="cuda")
        for algo in ("radix", "merge"):
            ms = timeit(lambda: sort(x, algo=algo), iters=5)
            emit(bench="sort", algo=algo, n=n, ms=ms, Mkeys_per_s=n / ms / 1e3, ref_ms=ref_s * 1e3, ref=ref_name,
                 speedup_vs_ref=ref_s * 1e3 / ms)
        ms = timeit(lambda: torch.sort(x), iters=5)
        emit(bench="sort", algo="torch.sort", n=n, ms=ms, Mkeys_per_s=n / ms / 1e3)


def bench_vigenere(emit, timeit):
    import os

    import numpy as np

    from cme213x.models.vigenere import create_cipher, solve_cipher

    path = "/root/reference/hw/hw3/programming/mobydick.txt"
    if os.path.exists(path):
        book = open(path, "rb").read()
    else:  # English-frequency synthetic corpus of the same size
        rng = np.random.default_rng(0)
        en = np.array([8.17, 1.49, 2.78, 4.25, 12.70, 2.23, 2.02, 6.09, 6.97, 0.15, 0.77, 4.03, 2.41, 6.75, 7.51,
                       1.93, 0.10, 5.99, 6.33, 9.06, 2.76, 0.98, 2.36, 0.15, 1.97, 0.07])
        book = rng.choice(np.arange(97, 123, dtype=np.uint8), 1_235_150, p=en / en.sum()).tobytes()
    c, key = create_cipher(book, 500, device="cuda", out_path=None)
    import time

    import torch

    solve_cipher(c, device="cuda", out_path=None, verbose=False)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        r = solve_cipher(c, device="cuda", out_path=None, verbose=False)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    emit(bench="vigenere_solve_x10", key_length=r["key_length"], seconds=secs, ref_seconds=17.0,
         speedup_vs_ref=17.0 / secs)


def bench_gemm(emit, timeit):
    import torch

    from cme213x.ops.gemm import sgemm

    ref = {"naive": 80.0, "lds": 235.9, "mfma": 784.6}  # GTX 480 GFLOP/s (Lecture09; mfma vs CUBLAS)
    for n in (1024, 4096, 8192):
        A = torch.randn(n, n, device="cuda")
        B = torch.randn_like(A)
        C = torch.empty_like(A)
        for v in (("naive",) if n <= 4096 else ()) + ("lds", "mfma"):
            ms = timeit(lambda: sgemm(A, B, C, variant=v), iters=3, warmup=1)
            gf = 2 * n ** 3 / ms / 1e6
            emit(bench="sgemm", n=n, variant=v, ms=ms, GFLOPs=gf, ref_GFLOPs=ref[v], vs_ref=gf / ref[v])
        torch.backends.cuda.matmul.allow_tf32 = False
        ms = timeit(lambda: torch.mm(A, B, out=C), iters=3, warmup=1)
        emit(bench="sgemm", n=n, variant="torch.mm(hipBLASLt)", ms=ms, GFLOPs=2 * n ** 3 / ms / 1e6)


def bench_algorithms(emit, timeit):
    import torch

    from cme213x.ops import algorithms as A

    n = 1 << 26
    x = torch.rand(n, device="cuda")
    m = x < 0.5
    ms = timeit(lambda: A.copy_if(x, m))
    emit(bench="copy_if", n=n, ms=ms, GBps=(4 * n + 2 * n + 4 * n / 2) / ms / 1e6)
    ms = timeit(lambda: x[m])
    emit(bench="copy_if", impl="torch x[mask]", n=n, ms=ms, GBps=(4 * n + 2 * n + 4 * n / 2) / ms / 1e6)
    ms = timeit(lambda: A.stable_partition(x, m))
    emit(bench="stable_partition", n=n, ms=ms, GBps=(8 * n + 2 * n) / ms / 1e6)
    k = torch.sort(torch.randint(0, 1 << 20, (n,), device="cuda", dtype=torch.int32)).values
    ms = timeit(lambda: A.unique(k))
    emit(bench="unique", n=n, ms=ms, GBps=(4 * n + 4 * (1 << 20)) / ms / 1e6)
    ms = timeit(lambda: torch.unique_consecutive(k))
    emit(bench="unique", impl="torch.unique_consecutive", n=n, ms=ms, GBps=(4 * n + 4 * (1 << 20)) / ms / 1e6)
    v = torch.rand(n, device="cuda")
    ms = timeit(lambda: A.reduce_by_key(k, v))
    emit(bench="reduce_by_key", n=n, segments=1 << 20, ms=ms)
    q = torch.randint(0, 1 << 20, (1 << 24,), device="cuda", dtype=torch.int32)
    ms = timeit(lambda: A.lower_bound(k, q))
    emit(bench="lower_bound", n=n, queries=q.numel(), ms=ms, Gqueries_per_s=q.numel() / ms / 1e6)
    ms = timeit(lambda: torch.searchsorted(k, q))
    emit(bench="lower_bound", impl="torch.searchsorted", n=n, queries=q.numel(), ms=ms,
         Gqueries_per_s=q.numel() / ms / 1e6)
    ms = timeit(lambda: A.max_element(x))
    emit(bench="max_element", n=n, ms=ms, GBps=4 * n / ms / 1e6)
    ms = timeit(lambda: torch.argmax(x).item())
    emit(bench="max_element", impl="torch.argmax", n=n, ms=ms, GBps=4 * n / ms / 1e6)
    keys = torch.randint(0, 256, (n,), device="cuda", dtype=torch.int32)
    ms = timeit(lambda: A.counting_sort(keys, 256))
    emit(bench="counting_sort", n=n, num_keys=256, ms=ms, Gkeys_per_s=n / ms / 1e6)


def bench_misc(emit, timeit):
    import math

    import torch

    from cme213x.ops.atomics import global_max, monte_carlo_pi

    n = 1 << 30
    import time

    monte_carlo_pi(1 << 20, 1, "cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    pi, _ = monte_carlo_pi(n, 3, "cuda")
    dt = time.perf_counter() - t0
    emit(bench="monte_carlo_pi", samples=n, seconds=dt, Gsamples_per_s=n / dt / 1e9, err=abs(pi - math.pi))
    x = torch.randn(1 << 26, device="cuda")
    ms = timeit(lambda: global_max(x))
    emit(bench="global_max", n=x.numel(), ms=ms, GBps=4 * x.numel() / ms / 1e6)


if __name__ == "__main__":
    main()
