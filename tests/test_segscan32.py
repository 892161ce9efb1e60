"""float32 ``segmented_scan`` and ``spmv_scan_run`` on the HIP and the CPU
backend: head layouts at the lane-vector, wave, tile and 64-tile-group edges of
the kernel, uint8 head bytes other than 1, bitmask tails, a size that sends
every workgroup of the persistent grid round its tile loop three times (taken
from ``scan_launch_info``), ``mul``, in-place output, views that are not 16-byte
(flags: 4-byte) aligned, inf / NaN kept inside their segment, the operand
checks, and the four tilings and the 64-step launches of ``spmv_scan_run``.

Oracles and tolerances: see ``scan_util.py``.
"""
import numpy as np
import pytest
import torch

from cme213x.ops.scan import TILE, lookback_timed_out, scan, scan_launch_info, segmented_scan, spmv_scan_run
from scan_util import (CPU, U32, assert_bits, assert_bound, cached, pack_bits, seg_exact_oracle, seg_rounding_oracle,
                       to_numpy, view_of)

T = TILE  # 4096: elements per tile of the float32 segmented scan (asserted against the launch query)
WAVE = 1024  # elements one wave of a tile covers
SIZES = [1, 2, 3, 5, T - 1, T, T + 1, 2 * T + 1, 3 * T + 31, 64 * T - 1, 64 * T, 64 * T + 1, 64 * T + T + 1]
assert {n % 32 for n in SIZES} >= {1, 31}
MODES = ["u8", "u8any", "bits"]  # uint8 1, uint8 drawn from {1, 2, 0x80, 0xff}, int32 bitmask words
# single heads: at a tile's start, one past it, its last element (tile 1, so a
# predecessor tile exists), a wave boundary inside tile 1 and the element before
# it, the first element of tile 64 and the last of tile 63 (the group boundary
# of the two-level look-back)
SINGLE = {"tile_start": T, "tile_start+1": T + 1, "tile_end-1": 2 * T - 1, "wave_start": T + 2 * WAVE,
          "wave_start-1": T + 2 * WAVE - 1, "tile64_first": 64 * T, "tile63_last": 64 * T - 1}
LAYOUTS = ["none", "all", *SINGLE, "last_tile", "rand5", "rand5000", "bit0_bit31"]


def _valid(layout: str, n: int) -> bool:
    if layout in SINGLE:
        return SINGLE[layout] < n
    if layout == "last_tile":
        return n > T
    return True


def _heads(layout: str, n: int) -> np.ndarray:
    """uint8 head flags (0 / 1); element 0 is left clear where the layout does
    not put a head there (it starts a segment anyway)."""
    f = np.zeros(n, dtype=np.uint8)
    if layout == "all":
        f[:] = 1
    elif layout in SINGLE:
        f[SINGLE[layout]] = 1
    elif layout == "last_tile":
        lo = (n - 1) // T * T
        f[lo + (n - lo) // 2] = 1
    elif layout in ("rand5", "rand5000"):
        mean = 5 if layout == "rand5" else 5000
        f[:] = np.random.default_rng(n % 1000 + mean).random(n) < 1.0 / mean
    elif layout == "bit0_bit31":  # heads at bit 0 and bit 31 of every third bitmask word
        f[0::96] = 1
        f[31::96] = 1
        f[0] = 0
    return f


def _flags(f: np.ndarray, mode: str, dev) -> torch.Tensor:
    if mode == "bits":
        return torch.from_numpy(pack_bits(f)).to(dev)
    if mode == "u8any":  # any non-zero byte is a head: 2 and 0x80 have bit 0 clear
        pick = np.random.default_rng(f.size).integers(0, 4, f.size)
        f = f * np.array([1, 2, 0x80, 0xFF], dtype=np.uint8)[pick]
    return torch.from_numpy(f).to(dev)


def _data(kind: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n % 1000 + 7 * len(kind))
    if kind == "int":  # sum |v| < 2^24 over the whole array: exact whatever the layout
        a = max(1, min(1000, (2 ** 24 - 1) // n))
        return rng.integers(-a, a + 1, n).astype(np.float32)
    if kind == "int_for_mul":  # sum |v * m| < 2^24 with |m| <= 2
        a = max(1, min(500, (2 ** 23 - 1) // n))
        return rng.integers(-a, a + 1, n).astype(np.float32)
    if kind == "mul_int":
        return rng.integers(-2, 3, n).astype(np.float32)
    if kind == "pm1":
        return rng.integers(-1, 2, n).astype(np.float32)
    assert kind in ("uniform", "mul_uniform")
    return rng.uniform(-1, 1, n).astype(np.float32)


def _x(kind: str, n: int) -> np.ndarray:
    return cached(("seg32x", kind, n), lambda: _data(kind, n))


def _dev(kind: str, n: int, dev) -> torch.Tensor:
    return cached(("seg32dev", kind, n, str(dev)), lambda: torch.from_numpy(_x(kind, n)).to(dev))


def _f(layout: str, n: int) -> np.ndarray:
    return cached(("seg32f", layout, n), lambda: _heads(layout, n))


def _exact(kind: str, layout: str, n: int, mul: bool = False) -> np.ndarray:
    def make():
        v = _x(kind, n).astype(np.float64)
        if mul:
            v = v * _x("mul_int", n)
        return seg_exact_oracle(v, _f(layout, n), 2.0 ** 24).astype(np.float32)
    return cached(("seg32ref", kind, layout, n, mul), make)


def _done(gpu):
    assert not lookback_timed_out(gpu)


# ------------------------------------------------------------------ the cases
def _case_exact(dev, layout, sizes=SIZES, kind="int"):
    for n in sizes:
        if not _valid(layout, n):
            continue
        f, want = _f(layout, n), _exact(kind, layout, n)
        for mode in MODES:
            y = segmented_scan(_dev(kind, n, dev), _flags(f, mode, dev))
            assert y.dtype == torch.float32 and y.shape == (n,)
            assert_bits(y, want, f"{layout} n={n} {mode}")
        if layout == "all":
            assert_bits(want, _x(kind, n))
        if layout == "none":  # the plain scan
            assert_bits(want, np.cumsum(_x(kind, n).astype(np.float64)).astype(np.float32))
            assert_bits(scan(_dev(kind, n, dev), algo="lookback"), want, f"plain scan n={n}")


def _case_mul(dev, layout, sizes):
    for n in sizes:
        if not _valid(layout, n):
            continue
        f, want = _f(layout, n), _exact("int_for_mul", layout, n, mul=True)
        for mode in MODES:
            y = segmented_scan(_dev("int_for_mul", n, dev), _flags(f, mode, dev), mul=_dev("mul_int", n, dev))
            assert_bits(y, want, f"mul {layout} n={n} {mode}")
            x = _dev("int_for_mul", n, dev).clone()
            assert segmented_scan(x, _flags(f, mode, dev), out=x, mul=_dev("mul_int", n, dev)) is x
            assert_bits(x, want, f"mul in place {layout} n={n} {mode}")
            x.copy_(_dev("int", n, dev))
            assert segmented_scan(x, _flags(f, mode, dev), out=x) is x
            assert_bits(x, _exact("int", layout, n), f"in place {layout} n={n} {mode}")


def _case_rounding(dev, layout, sizes):
    for n in sizes:
        if not _valid(layout, n):
            continue
        f = _f(layout, n)
        x, m = _x("uniform", n), _x("mul_uniform", n)
        ref, bound = seg_rounding_oracle(x.astype(np.float64), f, U32)
        mref, mbound = seg_rounding_oracle(x.astype(np.float64) * m.astype(np.float64), f, U32, extra=1)
        for mode in MODES:
            fl = _flags(f, mode, dev)
            assert_bound(segmented_scan(_dev("uniform", n, dev), fl), ref, bound, f"{layout} n={n} {mode}")
            assert_bound(segmented_scan(_dev("uniform", n, dev), fl, mul=_dev("mul_uniform", n, dev)), mref, mbound,
                         f"mul {layout} n={n} {mode}")


MUL_SIZES = [1, 3, T + 1, 3 * T + 31, 64 * T + 1, 64 * T + T + 1]
ROUNDING_LAYOUTS = [lay for lay in LAYOUTS if lay != "all"]  # one cumsum per segment: "all" is covered by the exact tier
ROUNDING_SIZES = [5, T + 1, 3 * T + 31, 64 * T + T + 1]


def _case_poison(dev, dtype, tile):
    """An inf at the head and a NaN at the end of ONE segment, which ends at a
    lane-vector, wave-row, wave, tile or group boundary: every other segment,
    before and after, keeps its exact bits."""
    n = 64 * tile + tile + 1
    limit = 2.0 ** 24 if dtype == np.float32 else 2.0 ** 44
    x = _x("int", n).astype(dtype)
    for end in (tile + 8, tile + 256, tile + WAVE, 2 * tile, 64 * tile):
        f = _heads("rand5000", n).copy()
        f[end - 5:end + 1] = [1, 0, 0, 0, 0, 1]  # the poisoned segment [end - 5, end); the next starts at the boundary
        want = seg_exact_oracle(x, f, limit).astype(dtype)
        xp = x.copy()
        xp[end - 5] = np.inf
        xp[end - 1] = np.nan
        for mode in MODES:
            y = to_numpy(segmented_scan(torch.from_numpy(xp).to(dev), _flags(f, mode, dev)))
            what = f"segment [{end - 5}, {end}) {mode}"
            assert np.all(np.isinf(y[end - 5:end - 1])) and np.isnan(y[end - 1]), what
            assert_bits(y[:end - 5], want[:end - 5], what + " before")
            assert_bits(y[end:], want[end:], what + " after")


def _case_views(dev):
    """x[k:], mul[k:], out[k:] (4-byte aligned only) and uint8 flags[k:] (1-byte
    aligned only), one operand at a time and all together."""
    for n in (7, T + 1, 3 * T + 31):
        layout = "rand5"
        f = _f(layout, n)
        x, m = _x("int_for_mul", n), _x("mul_int", n)
        want, mwant = _exact("int_for_mul", layout, n), _exact("int_for_mul", layout, n, mul=True)
        for mode in MODES:
            fl = _flags(f, mode, dev)
            fa = to_numpy(fl)
            for off in (1, 2, 3):
                what = f"n={n} {mode} view [{off}:]"
                xv, mv, fv = view_of(x, off, dev), view_of(m, 4 - off, dev), view_of(fa, off, dev)
                if dev.type == "cuda":
                    assert xv.data_ptr() % 16 == 4 * off and (mode == "bits" or fv.data_ptr() % 4 == off)
                assert_bits(segmented_scan(xv, fl), want, what + " x")
                assert_bits(segmented_scan(_dev("int_for_mul", n, dev), fv), want, what + " flags")
                assert_bits(segmented_scan(_dev("int_for_mul", n, dev), fl, mul=mv), mwant, what + " mul")
                ov = view_of(np.zeros_like(x), off, dev)
                assert segmented_scan(_dev("int_for_mul", n, dev), fl, out=ov) is ov
                assert_bits(ov, want, what + " out")
                assert segmented_scan(xv, fv, out=ov, mul=mv) is ov
                assert_bits(ov, mwant, what + " all")
                assert_bits(xv, x, what + " input changed")
                assert segmented_scan(xv, fv, out=xv, mul=mv) is xv
                assert_bits(xv, mwant, what + " in place")


def _rejections(dev):
    x = torch.ones(100, dtype=torch.float32, device=dev)
    f = torch.zeros(100, dtype=torch.uint8, device=dev)
    for bad in (f.bool(), f.long(), f.to(torch.int16), f.float()):
        with pytest.raises(TypeError, match="uint8.*int32"):
            segmented_scan(x, bad)
    with pytest.raises(ValueError, match="shorter"):
        segmented_scan(x, f[:99])
    with pytest.raises(ValueError, match="shorter"):
        segmented_scan(x, torch.zeros(3, dtype=torch.int32, device=dev))  # 96 bits
    segmented_scan(x, torch.zeros(4, dtype=torch.int32, device=dev))
    with pytest.raises(ValueError, match="flags.*contiguous"):
        segmented_scan(x, torch.zeros(200, dtype=torch.uint8, device=dev)[::2])
    for name in ("mul", "out"):
        for bad in (x.double(), x.int(), x[:99], torch.ones(200, device=dev)[::2]):
            with pytest.raises(ValueError, match=name):
                segmented_scan(x, f, **{name: bad})
    if dev.type == "cuda":
        with pytest.raises(ValueError, match="flags.*device"):
            segmented_scan(x, f.cpu())
        for name in ("mul", "out"):
            with pytest.raises(ValueError, match=name):
                segmented_scan(x, f, **{name: x.cpu()})
        with pytest.raises(ValueError, match="contiguous"):
            spmv_scan_run(torch.ones(200, device=dev)[::2], x, torch.zeros(4, dtype=torch.int32, device=dev), 1)
        with pytest.raises(ValueError, match="contiguous"):
            spmv_scan_run(x.clone(), torch.ones(200, device=dev)[::2], torch.zeros(4, dtype=torch.int32, device=dev), 1)


def _case_non_contiguous_x(dev):
    n, layout = T + 1, "rand5"
    base = torch.zeros(2 * n, dtype=torch.float32, device=dev)
    base[::2] = _dev("int", n, dev)
    xs = base[::2]
    assert not xs.is_contiguous()
    for mode in MODES:
        assert_bits(segmented_scan(xs, _flags(_f(layout, n), mode, dev)), _exact("int", layout, n), mode)


# ------------------------------------------------------------------------ GPU
@pytest.mark.gpu
@pytest.mark.parametrize("layout", LAYOUTS)
def test_segscan_exact_gpu(gpu, layout):
    _case_exact(gpu, layout)
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["none", "rand5000", "tile63_last"])
def test_segscan_three_rounds_gpu(gpu, layout):
    """Every workgroup of the persistent grid walks at least three tiles."""
    cap = scan_launch_info(1 << 40, "segscan", device=gpu)["workgroups"]
    n = 3 * cap * T + 12345
    info = scan_launch_info(n, "segscan", device=gpu)
    assert info["tile"] == T and info["workgroups"] == cap and info["tiles"] >= 3 * info["workgroups"], info
    assert n < 2 ** 24  # data in {-1, 0, 1}: sum |v| < 2^24 whatever the layout
    _case_exact(gpu, layout, [n], kind="pm1")
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["none", "all", "tile_end-1", "tile63_last", "rand5", "rand5000"])
def test_segscan_mul_and_in_place_gpu(gpu, layout):
    _case_mul(gpu, layout, MUL_SIZES)
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ROUNDING_LAYOUTS)
def test_segscan_rounding_gpu(gpu, layout):
    _case_rounding(gpu, layout, ROUNDING_SIZES)
    _done(gpu)


@pytest.mark.gpu
def test_segscan_poison_stays_in_its_segment_gpu(gpu):
    _case_poison(gpu, np.float32, T)
    _done(gpu)


@pytest.mark.gpu
def test_segscan_views_gpu(gpu):
    _case_views(gpu)
    _done(gpu)


@pytest.mark.gpu
def test_segscan_rejected_inputs_gpu(gpu):
    _rejections(gpu)
    _done(gpu)


@pytest.mark.gpu
def test_segscan_non_contiguous_x_gpu(gpu):
    _case_non_contiguous_x(gpu)
    _done(gpu)


@pytest.mark.gpu
def test_segscan_two_streams_gpu(gpu):
    n = 300 * T + 1
    f = _f("rand5000", n)
    fd = [_flags(f, mode, gpu) for mode in ("u8any", "bits")]
    xd = _dev("int", n, gpu)
    torch.cuda.synchronize(gpu)
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    outs = []
    for fl, s in zip(fd, streams):
        with torch.cuda.stream(s):
            outs.append(segmented_scan(xd, fl))
    _done(gpu)  # synchronises the device
    for y in outs:
        assert_bits(y, _exact("int", "rand5000", n))


# ------------------------------------------------------- spmv_scan_run, float32
# (n, steps, kind). Every value of every step is an integer the float32 kernels
# hold exactly, whatever the summation order:
#  * "general": a in [-3, 3], xx in {-1, 0, 1}, segments of at most 64 elements:
#    one step multiplies the largest magnitude by at most 64, so 3 * 64^3 < 2^24
#    bounds every partial sum of 3 steps;
#  * "one_xx": xx is +-1 at ONE position of each segment and 0 elsewhere, so a
#    step leaves +-a[l] (or 0) in every element: |a| <= 3 after any number of
#    steps -- what the long runs (two and three launches of 64 steps) need.
# Both are asserted on the float64 reference, step by step.
RUN_SHAPES = [(50_001, 3, "general"), (50_001, 70, "one_xx"), (50_001, 130, "one_xx"),  # <= 64 tiles
              (300 * T + 77, 3, "general"), (300 * T + 77, 70, "one_xx"),  # < 400 tiles
              (600 * T + 5, 3, "general"),  # < 900 tiles
              (1000 * T + 123, 3, "general")]  # >= 900 tiles
RUN_CLASSES = [lambda t: t <= 64, lambda t: 64 < t < 400, lambda t: 400 <= t < 900, lambda t: t >= 900]


def test_run_shapes_take_each_tiling():
    tiles = [(n + T - 1) // T for n, _, _ in RUN_SHAPES]
    for cls in RUN_CLASSES:
        assert any(cls(t) for t in tiles), tiles
    assert {s for _, s, _ in RUN_SHAPES} == {3, 70, 130}  # one, two and three launches of at most 64 steps


def _run_case(n, steps, kind):
    def make():
        rng = np.random.default_rng(n % 89 + steps)
        lens = rng.integers(1, 65, n // 16 + 64)
        starts = np.concatenate([[0], np.cumsum(lens)])
        starts = starts[starts < n]
        f = np.zeros(n, dtype=np.uint8)
        f[starts] = 1
        a = rng.integers(-3, 4, n).astype(np.float64)
        if kind == "general":
            xx = rng.integers(-1, 2, n).astype(np.float64)
        else:
            xx = np.zeros(n)
            seg_len = np.diff(np.append(starts, n))
            xx[starts + rng.integers(0, seg_len)] = rng.integers(0, 2, starts.size) * 2.0 - 1.0
        ref = a.copy()
        for _ in range(steps):  # asserts: integers, sum |a * xx| over every segment < 2^24
            ref = seg_exact_oracle(ref * xx, f, 2.0 ** 24)
        return a.astype(np.float32), xx.astype(np.float32), pack_bits(f), ref.astype(np.float32)
    return cached(("run32", n, steps), make)


def _case_run(dev, n, steps, kind, view: int = 0):
    a, xx, words, ref = _run_case(n, steps, kind)
    flags = torch.from_numpy(words).to(dev)
    # copies: on the CPU a tensor made from a cached array shares its memory
    ad, xd = (view_of(a, view, dev), view_of(xx, view, dev)) if view else (torch.from_numpy(a.copy()).to(dev),
                                                                             torch.from_numpy(xx.copy()).to(dev))
    y = spmv_scan_run(ad, xd, flags, steps)
    assert y is ad and y.dtype == torch.float32
    assert_bits(y, ref, f"run n={n} steps={steps}")
    assert_bits(xd, xx, "xx changed")
    b = torch.from_numpy(a.copy()).to(dev)
    for _ in range(steps):
        segmented_scan(b, flags, out=b, mul=xd)
    assert_bits(b, ref, f"{steps} segmented_scan calls n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("n,steps,kind", RUN_SHAPES)
def test_spmv_scan_run_float32_gpu(gpu, n, steps, kind):
    _case_run(gpu, n, steps, kind)
    _done(gpu)


@pytest.mark.gpu
def test_spmv_scan_run_float32_one_launch_per_step_gpu(gpu):
    from cme213x.utils import tuning

    with tuning.override(spmvscan_multi=0):
        assert tuning.get("spmvscan_multi") == 0
        _case_run(gpu, 300 * T + 77, 70, "one_xx")
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("off", [1, 2, 3])
def test_spmv_scan_run_float32_views_gpu(gpu, off):
    _case_run(gpu, 50_001, 3, "general", view=off)
    _case_run(gpu, 300 * T + 77, 70, "one_xx", view=off)
    _done(gpu)


# ------------------------------------------------------------------ CPU backend
CPU_SIZES = [1, 2, 3, 5, T + 1, 3 * T + 31, 64 * T + 1]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_segscan_exact_cpu(layout):
    _case_exact(CPU, layout, CPU_SIZES)


@pytest.mark.parametrize("layout", ["none", "all", "tile_end-1", "tile63_last", "rand5", "rand5000"])
def test_segscan_mul_and_in_place_cpu(layout):
    _case_mul(CPU, layout, MUL_SIZES)


@pytest.mark.parametrize("layout", ["none", "tile_start", "rand5", "rand5000", "bit0_bit31"])
def test_segscan_rounding_cpu(layout):
    _case_rounding(CPU, layout, [5, T + 1, 3 * T + 31])


def test_segscan_poison_stays_in_its_segment_cpu():
    _case_poison(CPU, np.float32, T)


def test_segscan_views_cpu():
    _case_views(CPU)


def test_segscan_rejected_inputs_cpu():
    _rejections(CPU)


def test_segscan_non_contiguous_x_cpu():
    _case_non_contiguous_x(CPU)


@pytest.mark.parametrize("n,steps,kind", [s for s in RUN_SHAPES if s[0] == 50_001] + [(300 * T + 77, 3, "general")])
def test_spmv_scan_run_float32_cpu(n, steps, kind):
    _case_run(CPU, n, steps, kind)
