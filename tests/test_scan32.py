"""32-bit ``scan`` (int32, uint32, float32) and ``reduce`` on the HIP and the CPU
backend: every algorithm at the lane-vector, wave-row, tile and group edges of
its kernels, a size that sends every workgroup of the persistent look-back grid
round its tile loop three times (taken from ``scan_launch_info``), wrapping
integer sums, inf / NaN, 4-byte-aligned views, in-place output, and the
look-back's epochs across launches, streams and the 24-bit epoch wrap.

Oracles and tolerances: see ``scan_util.py``.
"""
import numpy as np
import pytest
import torch

from cme213x.ops import scan as scan_mod
from cme213x.ops.scan import lookback_timed_out, reduce, scan, scan_launch_info, segmented_scan
from scan_util import (CPU, assert_bits, assert_bound, assert_exact_tier, cached, excl, int_oracle, pack_bits,
                       rounding_oracle, seg_info, to_numpy, to_torch, view_of)

LB_TILE = 16384  # elements per tile of the 32-bit look-back scan (asserted against the launch query)
GROUP = 64 * LB_TILE  # tiles per group of the two-level look-back
SIZES = [1, 2, 3, 4, 5, 7, 255, 256, 257, 4095, 4096, 4097, 16383, 16384, 16385, 32769]
LB_SIZES = [GROUP - 1, GROUP, GROUP + 1, GROUP + LB_TILE + 1]
ML_SIZES = [1, 5, 511, 512, 513, 512 * 512 - 1, 512 * 512, 512 * 512 + 1]  # one, two and three levels of 512-element blocks
VECTOR_ALGOS = ["lookback", "rts", "blelloch", "hillis"]
ML_ALGOS = ["blelloch_mlevel", "hillis_mlevel"]
INT_PATTERNS = ["small", "pm2_20", "minus1", "intmax", "u32max", "u32wide"]
PATTERNS = INT_PATTERNS + ["f32_int"]
# smallest unit a kernel of each algorithm could lose or count twice
ROUNDING = {"lookback": (LB_TILE, 100_003), "rts": (4096, 100_003), "blelloch": (4096, 100_003),
            "hillis": (4096, 100_003), "blelloch_mlevel": (512, 79 * 512 - 1), "hillis_mlevel": (512, 79 * 512 - 1)}


def _data(pattern: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n % 1000 + 31 * PATTERNS.index(pattern))
    if pattern == "small":
        return rng.integers(-3, 4, n, dtype=np.int32)
    if pattern == "pm2_20":
        return (rng.integers(0, 2, n, dtype=np.int32) * 2 - 1) * np.int32(2 ** 20)
    if pattern == "minus1":
        return np.full(n, -1, dtype=np.int32)
    if pattern == "intmax":  # wraps from the second element on
        return np.full(n, 2 ** 31 - 1, dtype=np.int32)
    if pattern == "u32max":
        return np.full(n, 2 ** 32 - 1, dtype=np.uint32)
    if pattern == "u32wide":
        return rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    assert pattern == "f32_int"  # as wide as the exact tier allows at this size
    a = max(3, min(1000, (2 ** 24 - 1) // n))
    return rng.integers(-a, a + 1, n).astype(np.float32)


def _case(pattern: str, n: int):
    """(input, inclusive oracle) of one (pattern, size), computed once."""
    def make():
        x = _data(pattern, n)
        if x.dtype == np.float32:
            return x, assert_exact_tier(x).astype(np.float32)
        return x, int_oracle(x)
    return cached(("scan32", pattern, n), make)


def _dev(pattern: str, n: int, dev) -> torch.Tensor:
    return cached(("scan32dev", pattern, n, str(dev)), lambda: to_torch(_case(pattern, n)[0], dev))


def _check_scan(dev, pattern, n, algo):
    x, inc = _case(pattern, n)
    for exclusive in (False, True):
        y = scan(_dev(pattern, n, dev), exclusive, algo=algo)
        assert y.shape == (n,)
        assert_bits(y, excl(inc) if exclusive else inc, f"{pattern} n={n} {algo} exclusive={exclusive}")


def _done(gpu):
    assert not lookback_timed_out(gpu)


# --------------------------------------------------------------------- GPU scans
@pytest.mark.gpu
def test_launch_query_gpu(gpu):
    for exclusive in (False, True):
        for dt in (torch.float32, torch.int32, torch.uint32):
            cap = scan_launch_info(1 << 40, "lookback", exclusive, gpu, dt)
            assert cap["tile"] == LB_TILE and cap["tiles"] == (1 << 40) // LB_TILE
            assert 1 <= cap["blocks_per_cu"] <= 4 and cap["workgroups"] % cap["blocks_per_cu"] == 0
            one = scan_launch_info(LB_TILE + 1, "lookback", exclusive, gpu, dt)
            assert one["tiles"] == one["workgroups"] == 2
    seg = scan_launch_info(1 << 40, "segscan", device=gpu)
    assert seg["tile"] == 4096 and 1 <= seg["blocks_per_cu"] <= 4 and seg["workgroups"] % seg["blocks_per_cu"] == 0
    assert scan_launch_info(0, "segscan", device=gpu)["tiles"] == 0
    with pytest.raises(ValueError, match="kind"):
        scan_launch_info(5, "rts", device=gpu)
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", VECTOR_ALGOS)
@pytest.mark.parametrize("pattern", PATTERNS)
def test_scan_edges_gpu(gpu, pattern, algo):
    for n in SIZES + (LB_SIZES if algo == "lookback" else []):
        _check_scan(gpu, pattern, n, algo)
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ML_ALGOS)
@pytest.mark.parametrize("pattern", ["small", "intmax", "f32_int"])
def test_scan_mlevel_edges_gpu(gpu, pattern, algo):
    for n in ML_SIZES:
        _check_scan(gpu, pattern, n, algo)
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int32, np.float32])
def test_scan_lookback_three_rounds_gpu(gpu, dtype):
    """Every workgroup of the persistent grid walks at least three tiles: the
    second and third round, the prefetch rotation and both LDS parities."""
    tdt = torch.int32 if dtype == np.int32 else torch.float32
    for exclusive in (False, True):
        cap = scan_launch_info(1 << 40, "lookback", exclusive, gpu, tdt)["workgroups"]
        n = 3 * cap * LB_TILE + 12345
        info = scan_launch_info(n, "lookback", exclusive, gpu, tdt)
        assert info["tile"] == LB_TILE and info["workgroups"] == cap and info["tiles"] >= 3 * info["workgroups"], info

        def make():
            x = np.random.default_rng(5).integers(-3, 4, n, dtype=np.int32)
            c = np.cumsum(x, dtype=np.int64)
            assert max(c.max(), 0) - min(c.min(), 0) < 2 ** 24  # exact in float32 too, in any association
            return x, c.astype(np.int32)
        x, inc = cached(("rounds", n), make)
        y = scan(torch.from_numpy(x).to(gpu).to(tdt), exclusive, algo="lookback")
        assert_bits(y, (excl(inc) if exclusive else inc).astype(dtype), f"n={n} exclusive={exclusive}")
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", VECTOR_ALGOS + ML_ALGOS)
def test_scan_float32_rounding_gpu(gpu, algo):
    tile, n = ROUNDING[algo]
    x = cached(("round_x", n), lambda: np.random.default_rng(n).uniform(0.5, 1.0, n).astype(np.float32))
    ref, bound = cached(("round_ref", n, tile), lambda: rounding_oracle(x, tile))
    for exclusive in (False, True):
        y = scan(torch.from_numpy(x).to(gpu), exclusive, algo=algo)
        # exclusive: element i holds the prefix of i terms, the bound of the preceding element
        assert_bound(y, excl(ref) if exclusive else ref, excl(bound) if exclusive else bound, f"{algo} {exclusive}")
    _done(gpu)


def _poison_case(dev, algo, n, boundaries):
    """One inf or NaN just before and just after each boundary: everything
    before it is exact, everything from it on is not finite."""
    x, inc = _case("f32_int", n)
    for b in boundaries:
        for p in (b - 1, b):
            for poison in (np.inf, np.nan):
                xp = x.copy()
                xp[p] = poison
                xd = torch.from_numpy(xp).to(dev)
                for exclusive in (False, True):
                    y = to_numpy(scan(xd, exclusive, algo=algo))
                    first = p + 1 if exclusive else p  # the first output that includes element p
                    what = f"{algo} n={n} poison {poison} at {p} exclusive={exclusive}"
                    assert_bits(y[:first], (excl(inc) if exclusive else inc)[:first], what)
                    assert not np.isfinite(y[first:]).any(), what
                    if np.isnan(poison):
                        assert np.isnan(y[first:]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("algo", VECTOR_ALGOS)
def test_scan_inf_nan_gpu(gpu, algo):
    if algo == "lookback":  # lane vector, wave row, a wave's 16 rows, tile, group of 64 tiles
        _poison_case(gpu, algo, GROUP + LB_TILE + 1, [4, 256, 4096, LB_TILE, GROUP])
    else:  # lane vector, wave row, wave, tile, the look-back's tile size
        _poison_case(gpu, algo, 32769, [4, 256, 1024, 4096, 16384])
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ["rts", "lookback"])
@pytest.mark.parametrize("pattern", ["intmax", "f32_int"])
def test_scan_in_place_gpu(gpu, pattern, algo):
    for n in (5, 32769, GROUP + LB_TILE + 1):
        x, inc = _case(pattern, n)
        for exclusive in (False, True):
            xd = to_torch(x, gpu)
            assert scan(xd, exclusive, out=xd, algo=algo) is xd
            assert_bits(xd, excl(inc) if exclusive else inc, f"n={n} exclusive={exclusive}")
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", ML_ALGOS)
def test_scan_mlevel_in_place_inclusive_still_raises_gpu(gpu, algo):
    xd = to_torch(_case("small", 513)[0], gpu)
    with pytest.raises(ValueError, match="in-place"):
        scan(xd, False, out=xd, algo=algo)
    _done(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("algo", VECTOR_ALGOS + ML_ALGOS)
@pytest.mark.parametrize("pattern", ["small", "f32_int"])
def test_scan_4_byte_aligned_views_gpu(gpu, pattern, algo):
    """buf[1:], buf[2:] and buf[3:] are contiguous but not 16-byte aligned, as
    the input, as ``out`` and as both (also in place)."""
    for n in (7, 4097, 32769):
        x, inc = _case(pattern, n)
        for off in (1, 2, 3):
            for exclusive in (False, True):
                want = excl(inc) if exclusive else inc
                what = f"{algo} n={n} view [{off}:] exclusive={exclusive}"
                xv = view_of(x, off, gpu)
                assert xv.data_ptr() % 16 == 4 * off
                assert_bits(scan(xv, exclusive, algo=algo), want, what + " in")
                assert_bits(xv, x, what + " input changed")
                ov = view_of(np.zeros_like(x), off, gpu)
                assert scan(_dev(pattern, n, gpu), exclusive, out=ov, algo=algo) is ov
                assert_bits(ov, want, what + " out")
                ov = view_of(np.zeros_like(x), 4 - off, gpu)
                assert scan(xv, exclusive, out=ov, algo=algo) is ov
                assert_bits(ov, want, what + " in and out")
                if algo in ("rts", "lookback"):
                    assert scan(xv, exclusive, out=xv, algo=algo) is xv
                    assert_bits(xv, want, what + " in place")
    _done(gpu)


@pytest.mark.gpu
def test_scan_float32_rts_bitwise_reproducible_gpu(gpu):
    n = 3_000_001
    x = torch.from_numpy(np.random.default_rng(3).standard_normal(n).astype(np.float32)).to(gpu)
    a = scan(x, algo="rts")
    scan(x[: n // 3].clone(), True, algo="lookback")  # other work on the device in between
    reduce(x)
    b = scan(x, algo="rts")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    _done(gpu)


# ------------------------------------------------------------- look-back state
def _pool(n: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).integers(-50, 51, n, dtype=np.int32)


def _epoch_case(i: int, pool: np.ndarray):
    """Launch i of a run: size, dtype and exclusive all change."""
    n = [777, LB_TILE + 1, 3 * LB_TILE + 5, 65 * LB_TILE + 3][i % 4]
    lo = (i * 7919) % (pool.size - n)
    x = pool[lo:lo + n]
    dt = [np.int32, np.float32, np.uint32][i % 3]
    exclusive = i % 5 in (1, 3)
    inc = np.cumsum(x, dtype=np.int64)  # exact in float32 too: test_epoch_pools_are_exact_in_float32
    want = (excl(inc) if exclusive else inc)
    want = (want & 0xFFFFFFFF).astype(np.uint32) if dt == np.uint32 else want.astype(dt)
    return x.astype(dt), exclusive, want


@pytest.mark.gpu
def test_lookback_200_epochs_gpu(gpu):
    """200 back-to-back look-back launches on one stream share one descriptor
    array, with a new epoch per launch and no memset."""
    pool = _pool(66 * LB_TILE, 11)
    runs = []
    for i in range(200):
        x, exclusive, want = _epoch_case(i, pool)
        runs.append((scan(to_torch(x, gpu), exclusive, algo="lookback"), want))
    _done(gpu)
    for i, (y, want) in enumerate(runs):
        assert_bits(y, want, f"launch {i}")


@pytest.mark.gpu
def test_lookback_families_interleave_gpu(gpu, monkeypatch):
    """float32 segmented scans, an int64 scan, a look-back ``copy_if`` and the
    32-bit look-back scan issued back to back never read each other's words."""
    from cme213x.ops import algorithms

    monkeypatch.setattr(algorithms, "SELECT_ALGO", "lookback")
    n = 65 * LB_TILE + 9
    g = np.random.default_rng(12)
    runs = []
    for r in range(4):
        a = g.integers(-50, 51, n, dtype=np.int32)
        f = (g.random(n) < 0.001).astype(np.uint8)
        wide = g.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
        keep = (g.random(n) < 0.5).astype(np.uint8)
        starts, seg = seg_info(f)
        c = np.cumsum(a, dtype=np.int64)
        assert np.abs(c).max() < 2 ** 23  # every contiguous partial sum is exact in float32
        seg_want = (c - np.concatenate([[0], c])[starts][seg]).astype(np.float32)
        ad, af = torch.from_numpy(a).to(gpu), torch.from_numpy(a.astype(np.float32)).to(gpu)
        runs.append((scan(ad, bool(r % 2), algo="lookback"), (c - a if r % 2 else c).astype(np.int32)))
        runs.append((segmented_scan(af, torch.from_numpy(f).to(gpu)), seg_want))
        runs.append((scan(torch.from_numpy(wide).to(gpu), algo="lookback"), np.cumsum(wide)))
        runs.append((algorithms.copy_if(ad, torch.from_numpy(keep).to(gpu)), a[keep != 0]))
        runs.append((segmented_scan(af, torch.from_numpy(pack_bits(f)).to(gpu)), seg_want))
    _done(gpu)
    for i, (y, want) in enumerate(runs):
        assert_bits(y, want, f"launch {i}")


@pytest.mark.gpu
def test_lookback_two_streams_gpu(gpu):
    n = 300 * LB_TILE + 1
    xs = [_pool(n, 13 + i) for i in range(2)]
    xd = [torch.from_numpy(x).to(gpu) for x in xs]
    torch.cuda.synchronize(gpu)
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    outs = []
    for i, (x, s) in enumerate(zip(xd, streams)):
        with torch.cuda.stream(s):
            outs.append(scan(x, bool(i), algo="lookback"))
    _done(gpu)  # synchronises the device
    for i, (x, y) in enumerate(zip(xs, outs)):
        c = np.cumsum(x, dtype=np.int64)
        assert_bits(y, (c - x if i else c).astype(np.int32), f"stream {i}")


@pytest.mark.gpu
def test_lookback_epoch_wrap_gpu(gpu):
    """Six scans across the 24-bit epoch limit: the descriptor array is zeroed
    and the count restarts at 1."""
    from cme213x import _ext

    pool = _pool(66 * LB_TILE, 14)
    scan(to_torch(pool, gpu), algo="lookback")  # the stream's descriptor array exists
    key = (f"lookback:{_ext.stream_ptr(gpu)}", gpu.index)
    assert key in scan_mod._epochs
    scan_mod._epochs[key] = scan_mod._EPOCH_LIMIT - 3
    runs, epochs = [], []
    for i in range(6):
        x, exclusive, want = _epoch_case(i + 3, pool)
        runs.append((scan(to_torch(x, gpu), exclusive, algo="lookback"), want))
        epochs.append(scan_mod._epochs[key])
    assert epochs == [scan_mod._EPOCH_LIMIT - 2, scan_mod._EPOCH_LIMIT - 1, 1, 2, 3, 4]
    _done(gpu)
    for i, (y, want) in enumerate(runs):
        assert_bits(y, want, f"launch {i} (epoch {epochs[i]})")


# ---------------------------------------------------------------------- reduce
R_SIZES = [1, 2, 3, 5, 1023, 1024, 1025, (1 << 20) - 1, (1 << 20) + 1, (1 << 22) - 1, (1 << 22) + 1, 3_000_017]
R_BLOCK = 1024  # elements one workgroup takes per sweep: the smallest unit a reduction could lose
R_ROUNDING_SIZES = [1, 2, 3, 5, 1023, 1024, 1025, 50_001]  # where the rounding bound meets its condition


def _reduce_data(n: int):
    def make():
        rng = np.random.default_rng(n % 1000 + 3)
        return {"neg_i": rng.integers(-1000, 0, n, dtype=np.int32), "pos_i": rng.integers(1, 1001, n, dtype=np.int32),
                "wide_i": rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32),
                "neg_f": -rng.uniform(0.5, 1000.0, n).astype(np.float32),
                "pos_f": rng.uniform(0.5, 1000.0, n).astype(np.float32),
                "int_f": rng.integers(0, 4, n).astype(np.float32)}  # sum <= 3 n < 2^24: exact in any order
    return cached(("reduce", n), make)


def _item(t: torch.Tensor):
    assert t.dim() == 0
    return to_numpy(t)[()]


def _reduce_cases(dev):
    algos_sum = ["vector", "tree"] if dev.type == "cuda" else ["vector"]
    for n in R_SIZES:
        d = _reduce_data(n)
        t = {k: torch.from_numpy(v).to(dev) for k, v in d.items()}
        # all-negative data for max, all-positive for min: an identity of 0 would win
        for kind in ("i", "f"):
            assert _item(reduce(t["neg_" + kind], "max")) == d["neg_" + kind].max() < 0, n
            assert _item(reduce(t["pos_" + kind], "min")) == d["pos_" + kind].min() > 0, n
            assert _item(reduce(t["neg_" + kind], "min")) == d["neg_" + kind].min(), n
            assert _item(reduce(t["pos_" + kind], "max")) == d["pos_" + kind].max(), n
        for algo in algos_sum:
            want = np.int64(d["wide_i"].astype(np.int64).sum() & 0xFFFFFFFF).astype(np.uint32).view(np.int32)
            assert _item(reduce(t["wide_i"], "sum", algo)) == want, (n, algo)  # wraps modulo 2^32
            s = float(d["int_f"].astype(np.float64).sum())
            assert s < 2.0 ** 24 and _item(reduce(t["int_f"], "sum", algo)) == np.float32(s), (n, algo)


def _reduce_rounding(dev):
    algos_sum = ["vector", "tree"] if dev.type == "cuda" else ["vector"]
    for n in R_ROUNDING_SIZES:
        x = np.random.default_rng(n).uniform(0.5, 1.0, n).astype(np.float32)
        ref, bound = rounding_oracle(x, R_BLOCK)  # asserts bound < half of the smallest block sum
        for algo in algos_sum:
            got = float(_item(reduce(torch.from_numpy(x).to(dev), "sum", algo)))
            assert abs(got - ref[-1]) <= bound[-1], (n, algo, got, ref[-1], bound[-1])


def _reduce_extremes(dev):
    """INT_MIN / INT_MAX / -inf / +inf, one at a time, at the first element and
    in the scalar tail (n % 4 = 1, 2, 3) of otherwise one-signed data."""
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    for n in (1025, 1026, 1027, 5 * 1024 * 1024 // 4 + 3):
        assert n % 4 in (1, 2, 3)
        d = _reduce_data(n)
        for p in (0, n - 1, n - 2, n - 3):
            for key, op, extreme in (("pos_i", "min", lo), ("neg_i", "max", hi), ("pos_f", "min", -np.inf),
                                     ("neg_f", "max", np.inf), ("neg_i", "min", lo), ("pos_f", "max", np.inf)):
                x = d[key].copy()
                x[p] = extreme
                assert _item(reduce(torch.from_numpy(x).to(dev), op)) == extreme, (n, p, key, op)


@pytest.mark.gpu
def test_reduce_sizes_gpu(gpu):
    _reduce_cases(gpu)
    _done(gpu)


@pytest.mark.gpu
def test_reduce_float32_rounding_gpu(gpu):
    _reduce_rounding(gpu)
    _done(gpu)


@pytest.mark.gpu
def test_reduce_extremes_gpu(gpu):
    _reduce_extremes(gpu)
    _done(gpu)


@pytest.mark.gpu
def test_reduce_4_byte_aligned_views_gpu(gpu):
    for n in (5, 1027, (1 << 20) + 1):
        d = _reduce_data(n)
        for off in (1, 2, 3):
            assert _item(reduce(view_of(d["neg_i"], off, gpu), "max")) == d["neg_i"].max()
            assert _item(reduce(view_of(d["pos_f"], off, gpu), "min")) == d["pos_f"].min()
            for algo in ("vector", "tree"):
                assert _item(reduce(view_of(d["int_f"], off, gpu), "sum", algo)) == d["int_f"].astype(np.float64).sum()
    _done(gpu)


# ------------------------------------------------------------------ CPU backend
@pytest.mark.parametrize("pattern", PATTERNS)
def test_scan_edges_cpu(pattern):
    for n in SIZES + LB_SIZES + ML_SIZES:
        _check_scan(CPU, pattern, n, "auto")


def test_scan_float32_rounding_cpu():
    n = 100_003
    x = np.random.default_rng(n).uniform(0.5, 1.0, n).astype(np.float32)
    ref, bound = rounding_oracle(x, 4096)
    for exclusive in (False, True):
        y = scan(torch.from_numpy(x), exclusive)
        assert_bound(y, excl(ref) if exclusive else ref, excl(bound) if exclusive else bound)


def test_scan_inf_nan_cpu():
    _poison_case(CPU, "auto", 32769, [4, 256, 4096, 16384])


def test_scan_in_place_and_views_cpu():
    for pattern in ("intmax", "f32_int"):
        x, inc = _case(pattern, 4097)
        for exclusive in (False, True):
            want = excl(inc) if exclusive else inc
            xv = view_of(x, 1, CPU)
            ov = view_of(np.zeros_like(x), 3, CPU)
            assert scan(xv, exclusive, out=ov) is ov
            assert_bits(ov, want)
            assert scan(xv, exclusive, out=xv) is xv
            assert_bits(xv, want)


def test_epoch_pools_are_exact_in_float32():
    """The epoch tests scan slices of a pool: every prefix of the pool stays
    below 2^23, so every contiguous partial sum stays below 2^24."""
    for seed in (11, 14):
        assert np.abs(np.cumsum(_pool(66 * LB_TILE, seed), dtype=np.int64)).max() < 2 ** 23


def test_reduce_sizes_cpu():
    _reduce_cases(CPU)


def test_reduce_float32_rounding_cpu():
    _reduce_rounding(CPU)


def test_reduce_extremes_cpu():
    _reduce_extremes(CPU)
