#!/usr/bin/env python3
"""64-bit segmented scan and the float64 SpMV-scan run on one GPU
(profiles/segscan64_r9.md). One JSON line per measurement.

  segscan  segmented_scan int64 / float64 at 2^25 and 2^27 elements, mean
           segment lengths 8, 1000 and "no heads", against (a) the unsegmented
           scan(algo="lookback") of the same dtype and size, (b) the float32
           segmented_scan at the same BYTE count, (c) what a torch user does
           today, c = torch.cumsum(v); c - base[seg_id] (seg_id and the segment
           starts are precomputed outside the timed region), and (d) the
           16-B-lane byte copy of the same byte count, the in-run HBM rate.
           Every arm cycles through 3 operand sets (>= 1.5 GB in total)
           round-robin, so no call reads what the 256 MB Infinity Cache kept;
           the arms alternate inside one process, batch by batch, and the
           median batch of each is reported.
  run      spmv_scan_run float64 on the 15 final-project shapes against the
           float32 run of the same shapes (alternating), with the warm byte
           copy of one step's traffic (read a, xx, write a) beside it. The
           run iterates in place on one array, so it is cache-warm by nature.
  --arms   additionally the tuning arms of libcme213_tune.so (CME_TUNE=1):
           rows x prefetch for the scan, rows x prefetch x fused launch for the
           run.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

NSETS = 3


def emit(out, **kw):
    line = json.dumps(kw)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def alternate(dev, arms, sets_of, reps=5, rounds=2):
    """{arm: median ms per call}: in every repetition each arm runs one timed
    batch of ``rounds`` passes over its operand sets, arm after arm."""
    import torch

    for name, fn in arms.items():
        for s in sets_of[name]:
            fn(s)
    torch.cuda.synchronize(dev)
    ts = {name: [] for name in arms}
    for _ in range(reps):
        for name, fn in arms.items():
            sets = sets_of[name]
            calls = rounds * len(sets)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for i in range(calls):
                fn(sets[i % len(sets)])
            e1.record()
            e1.synchronize()
            ts[name].append(e0.elapsed_time(e1) / calls)
    return {name: sorted(v)[len(v) // 2] for name, v in ts.items()}


def _heads(n, seglen, gen, dev):
    import torch

    if seglen is None:
        return torch.zeros(n, dtype=torch.uint8, device=dev)
    return (torch.rand(n, device=dev, generator=gen) < 1.0 / seglen).to(torch.uint8)


def _bitmask(f):
    """int32 bitmask words of uint8 flags (bit i % 32 of word i // 32)."""
    import torch

    n = f.numel()
    pad = torch.zeros((n + 31) // 32 * 32, dtype=torch.int64, device=f.device)
    pad[:n] = f
    w = (pad.view(-1, 32) << torch.arange(32, device=f.device)).sum(1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


def bench_segscan(dev, out, arms_on, sizes):
    import torch

    from cme213x import _ext
    from cme213x.ops import elementwise, scan as sc

    if arms_on:
        _ext.proto(_ext.TUNE_PROTOS, "cme_segscan64_tune", "pppqiiipp")
    gen = torch.Generator(device=dev).manual_seed(1)
    for n in sizes:
        for dtype in (torch.int64, torch.float64):
            for seglen in (8, 1000, None):
                sets64, sets32 = [], []
                for _ in range(NSETS):
                    if dtype == torch.int64:
                        x = torch.randint(-2 ** 40, 2 ** 40, (n,), device=dev, generator=gen, dtype=torch.int64)
                    else:
                        x = torch.rand(n, device=dev, generator=gen, dtype=torch.float64) * 2 - 1
                    f = _heads(n, seglen, gen, dev)
                    h = f.clone()
                    h[0] = 1
                    starts = torch.nonzero(h).flatten()
                    sets64.append(dict(x=x, out=torch.empty_like(x), u8=f, bits=_bitmask(f),
                                       seg=torch.cumsum(h, 0, dtype=torch.int64) - 1, prev=(starts - 1).clamp_(min=0)))
                    del h, starts
                    x32 = torch.rand(2 * n, device=dev, generator=gen, dtype=torch.float32) * 2 - 1
                    sets32.append(dict(x=x32, out=torch.empty_like(x32), bits=_bitmask(_heads(2 * n, seglen, gen, dev))))

                def torch_way(s):
                    c = torch.cumsum(s["x"], 0)
                    base = c[s["prev"]]
                    base[0] = 0
                    return torch.sub(c, base[s["seg"]], out=s["out"])

                arms = {
                    "segscan64_bits": lambda s: sc.segmented_scan(s["x"], s["bits"], out=s["out"]),
                    "segscan64_u8": lambda s: sc.segmented_scan(s["x"], s["u8"], out=s["out"]),
                    "scan64_lookback": lambda s: sc.scan(s["x"], out=s["out"], algo="lookback"),
                    "segscan32_same_bytes": lambda s: sc.segmented_scan(s["x"], s["bits"], out=s["out"]),
                    "torch_cumsum_minus_base": torch_way,
                    "copy_same_bytes": lambda s: elementwise.copy_(s["out"], s["x"]),
                }
                sets_of = {k: sets64 for k in arms}
                sets_of["segscan32_same_bytes"] = sets32
                if arms_on:
                    ws = sc._run64_ws(sets64[0]["x"])
                    for rows in (4, 8, 16):
                        for pf in (0, 1):
                            arms[f"arm_rows{rows}_pf{pf}"] = (
                                lambda s, rows=rows, pf=pf: _ext.call_hip(
                                    "cme_segscan64_tune", s["x"].data_ptr(), s["out"].data_ptr(), s["bits"].data_ptr(), n,
                                    3 if dtype == torch.int64 else 4, rows, pf, ws.data_ptr(), _ext.stream_ptr(dev)))
                            sets_of[f"arm_rows{rows}_pf{pf}"] = sets64
                ms = alternate(dev, arms, sets_of)
                assert not sc.lookback_timed_out(dev)
                ref = torch_way(sets64[0]).clone()
                got = sc.segmented_scan(sets64[0]["x"], sets64[0]["bits"])
                ok = bool(torch.equal(got, ref)) if dtype == torch.int64 else bool(
                    ((got - ref).abs() <= 1e-9 * (1 + ref.abs())).all())
                for name, t in ms.items():
                    emit(out, bench="segscan", dtype=str(dtype).split(".")[1], n=n, seglen=seglen, arm=name,
                         ms=round(t, 4), GBps_16B_per_elem=round(16.0 * n / t / 1e6, 1), matches_torch=ok)
                del sets64, sets32, ref, got
                torch.cuda.empty_cache()


def bench_run(dev, out, arms_on, names):
    import numpy as np
    import torch

    from cme213x import _ext
    from cme213x.models.spmv_scan import BENCH_SHAPES, SpmvScanSolver, generate
    from cme213x.ops import elementwise, scan as sc

    if arms_on:
        _ext.proto(_ext.TUNE_PROTOS, "cme_spmv_scan_run64_tune", "pppqipiip")
    for name in names or BENCH_SHAPES:
        n, p, N = BENCH_SHAPES[name]
        prob = generate(n, p, 100000, N, seed=0, dtype=np.float64)
        s64 = SpmvScanSolver(prob, dev, dtype=torch.float64)
        s32 = SpmvScanSolver(prob, dev, dtype=torch.float32)
        runs = {"f64": (s64, lambda: s64.run()), "f32": (s32, lambda: s32.run())}
        if arms_on:
            ws = sc._run64_ws(s64.a)
            for rows in (2, 4, 8):
                for mode in (0, 1, 2, 3):
                    runs[f"f64_rows{rows}_pf{mode & 1}_fused{mode >> 1}"] = (
                        s64, lambda rows=rows, mode=mode: _ext.call_hip(
                            "cme_spmv_scan_run64_tune", s64.a.data_ptr(), s64.xx.data_ptr(), s64.flags.data_ptr(), n, N,
                            ws.data_ptr(), rows, mode, _ext.stream_ptr(dev)))
        # one step's traffic as a warm byte copy: read a and xx, write a = 1.5 copies of n elements
        buf = torch.empty(3 * n, dtype=torch.float64, device=dev)
        half = 3 * n // 2

        def copy_steps():
            for _ in range(N):
                elementwise.copy_(buf[half:2 * half], buf[:half])

        ts = {k: [] for k in list(runs) + ["copy_24B_per_elem"]}
        finals = {}
        for rep in range(6):  # the first repetition is the warm-up
            for k, (sol, fn) in runs.items():
                sol.reset()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                if rep:
                    ts[k].append(e0.elapsed_time(e1))
                elif k != "f32":
                    finals[k] = sol.a.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            copy_steps()
            e1.record()
            e1.synchronize()
            if rep:
                ts["copy_24B_per_elem"].append(e0.elapsed_time(e1))
        assert not sc.lookback_timed_out(dev)
        base = finals["f64"]
        for k, v in ts.items():
            t = sorted(v)[len(v) // 2]
            same = None
            if k in finals:  # arms differ in summation order only
                same = bool(((finals[k] - base).abs() <= 1e-9 * (1e-300 + base.abs().max())).all())
            bytes_per = 12.0 if k == "f32" else 24.0
            emit(out, bench="run", shape=name, n=n, p=p, N=N, arm=k, ms=round(t, 4),
                 GBps_model=round(bytes_per * n * N / t / 1e6, 1), agrees_with_f64=same)
        del s64, s32, buf, finals


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None, help="segscan, run")
    ap.add_argument("--arms", action="store_true", help="also time the tuning arms (needs libcme213_tune.so)")
    ap.add_argument("--sizes", nargs="*", type=int, default=[1 << 25, 1 << 27])
    ap.add_argument("--shapes", nargs="*", default=None)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    args = ap.parse_args()
    import torch

    import cme213x  # noqa: F401

    if not torch.cuda.is_available():
        raise SystemExit("bench_segscan64: needs a GPU (a CPU timing says nothing about it)")
    dev = torch.device("cuda")
    out = open(args.out, "a") if args.out else None
    want = lambda k: args.only is None or k in args.only  # noqa: E731
    if want("segscan"):
        bench_segscan(dev, out, args.arms, args.sizes)
    if want("run"):
        bench_run(dev, out, args.arms, args.shapes)


if __name__ == "__main__":
    main()
