"""64-bit segmented scan (int64, float64) on the HIP and the CPU backend, the
float64 ``spmv_scan_run`` and the ``fp --double`` driver.

int64 results are compared exactly against the vectorised oracle ``cumsum(v) -
base[seg_id]`` in int64, which is itself exact modulo 2^64. float64 is compared
bitwise where every summation order is exact (integer-valued data whose
per-segment prefixes stay below 2^44) and otherwise against one
``numpy.longdouble`` ``cumsum`` per segment under the worst-case bound of any
summation order, |y_i - ref_i| <= 1.01 * m * 2^-53 * sum |v_j| (m: the 1-based
position in the segment, the sum over the segment's elements up to i; m + 1
with ``mul``, for the product's own rounding).

"Bitwise" leaves out the sign of a zero: IEEE 754 gives (-0) + (+0) = +0, the
kernels shift zeros in as the identity of their lane scans, so a sum of
negative zeros comes back as +0. Both sides are normalised with ``+ 0.0``
before their bits are compared; every other value keeps all 64 bits.
"""
import os

import numpy as np
import pytest
import torch

from cme213x.ops.scan import (SEGTILE64, head_flags_from_offsets, lookback_timed_out, scan, segmented_scan,
                              spmv_scan_run)

T = SEGTILE64
EDGE_SIZES = [1, 2, 3, T - 1, T, T + 1, 64 * T - 1, 64 * T + 1]
LARGE = 9_000_011
SIZES = EDGE_SIZES + [LARGE]
INT_PATTERNS = ["small", "wide", "minus1", "lowmax", "wrap"]
MODES = ["u8", "bits"]
U = 2.0 ** -53
CPU = torch.device("cpu")

# single heads: at a tile's start, one past it, its last element (tile 1, so a
# predecessor tile exists), the first element of tile 64 and the last of tile
# 63 (the group boundary of the two-level look-back)
SINGLE = {"tile_start": T, "tile_start+1": T + 1, "tile_end-1": 2 * T - 1, "tile64_first": 64 * T,
          "tile63_last": 64 * T - 1}
LAYOUTS = ["none", "all", *SINGLE, "last_tile", "rand5", "rand5000", "bit0_bit31"]


def _valid(layout: str, n: int) -> bool:
    if layout in SINGLE:
        return SINGLE[layout] < n
    if layout == "last_tile":
        return n > T  # otherwise the last tile is the first
    return True


def _heads(layout: str, n: int) -> np.ndarray:
    """uint8 head flags of one layout; element 0 is deliberately left clear
    where the layout does not put a head there (it starts a segment anyway)."""
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


def _int_data(pattern: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n % 1000 + 17 * INT_PATTERNS.index(pattern))
    if pattern == "small":
        return rng.integers(-3, 4, n, dtype=np.int64)
    if pattern == "wide":  # prefixes cross 32-bit boundaries in both directions
        return rng.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    if pattern == "minus1":  # the two halves of a slot differ from the first element on
        return np.full(n, -1, dtype=np.int64)
    if pattern == "lowmax":  # the low half carries into the high half all the time
        return np.full(n, 2 ** 32 - 1, dtype=np.int64)
    sign = rng.integers(0, 2, n, dtype=np.int64) * 2 - 1  # near +-2^62: sums wrap modulo 2^64
    return sign * (2 ** 62) + rng.integers(-1000, 1000, n, dtype=np.int64)


def _data(kind: str, n: int) -> np.ndarray:
    if kind in INT_PATTERNS:
        return _int_data(kind, n)
    if kind == "f64_exact":
        return np.floor(np.random.default_rng(n % 1000).uniform(0, 2 ** 20, n))  # every prefix < 2^44
    if kind == "f64_uniform":
        return np.random.default_rng(n % 1000 + 5).uniform(-1, 1, n)
    if kind == "mul_int":
        return np.random.default_rng(n % 1000 + 9).integers(-3, 4, n, dtype=np.int64)
    assert kind == "mul_f64"
    return np.random.default_rng(n % 1000 + 10).uniform(-1, 1, n)


_cache: dict = {}


def _cached(key, make):
    """A few entries are kept: the parametrisations visit a (data, size) and a
    (layout, size) consecutively, so inputs, device copies and oracles are
    computed once and shared by the cases that follow."""
    if key not in _cache:
        if len(_cache) > 12:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


def _x(kind: str, n: int) -> np.ndarray:
    return _cached(("x", kind, n), lambda: _data(kind, n))


def _seg(layout: str, n: int):
    """(uint8 flags, segment starts, segment id of every element)."""
    def make():
        f = _heads(layout, n)
        h = f.copy()
        h[0] = 1
        return f, np.flatnonzero(h), np.cumsum(h, dtype=np.int64) - 1
    return _cached(("seg", layout, n), make)


def _vector_oracle(v: np.ndarray, layout: str, n: int) -> np.ndarray:
    """cumsum(v) - base[seg_id]: exact for int64 (modulo 2^64) and for float64
    data whose sums are all exactly representable."""
    _, starts, seg = _seg(layout, n)
    with np.errstate(over="ignore"):
        c = np.cumsum(v)
        base = np.concatenate([np.zeros(1, dtype=v.dtype), c])[starts]
        return c - base[seg]


def _ref(kind: str, layout: str, n: int) -> np.ndarray:
    return _cached(("ref", kind, layout, n), lambda: _vector_oracle(_x(kind, n), layout, n))


def _longdouble_oracle(v: np.ndarray, layout: str, n: int, extra: int = 0):
    """(per-segment longdouble running sums, bound): one cumsum per segment."""
    _, starts, seg = _seg(layout, n)
    assert starts.size <= 200_000
    ref = np.empty(n, dtype=np.longdouble)
    asum = np.empty(n, dtype=np.float64)
    av = np.abs(v).astype(np.float64)
    for lo, hi in zip(starts, np.append(starts[1:], n)):
        ref[lo:hi] = np.cumsum(v[lo:hi])
        asum[lo:hi] = np.cumsum(av[lo:hi])
    m = np.arange(n) - starts[seg] + 1 + extra
    return ref, 1.01 * m * U * asum


def _flags(layout: str, n: int, mode: str, dev) -> torch.Tensor:
    def make():
        f = _seg(layout, n)[0]
        if mode == "u8":
            return torch.from_numpy(f).to(dev)
        words = np.packbits(np.pad(f, (0, -n % 32)), bitorder="little").view(np.int32)
        return torch.from_numpy(words.copy()).to(dev)
    return _cached(("flags", layout, n, mode, str(dev)), make)


def _dev(kind: str, n: int, dev) -> torch.Tensor:
    return _cached(("dev", kind, n, str(dev)), lambda: torch.from_numpy(_x(kind, n)).to(dev))


def _bits(a: np.ndarray) -> np.ndarray:
    """The 64 bits of every element; a float zero loses its sign (see above)."""
    return (a + 0.0).view(np.int64) if a.dtype == np.float64 else a.view(np.int64)


def _assert_bits(got: torch.Tensor, want: np.ndarray) -> None:
    g = got.cpu().numpy()
    assert g.dtype == want.dtype
    bad = np.flatnonzero(_bits(g) != _bits(want))
    assert bad.size == 0, f"{bad.size} elements differ, first at {bad[0]}: {g[bad[0]]!r} != {want[bad[0]]!r}"


def _assert_bound(got: torch.Tensor, ref, bound) -> None:
    err = np.abs(got.cpu().numpy().astype(np.longdouble) - ref)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"element {worst}: error {float(err[worst]):.3e} > bound {float(bound[worst]):.3e}"


LAYOUT_CASES = [(n, lay) for n in SIZES for lay in LAYOUTS if _valid(lay, n)]
PATTERN_LAYOUTS = ["none", "rand5", "rand5000"]
# one longdouble cumsum per segment: at most 200 000 segments a case
UNIFORM_CASES = ([(n, lay) for n in EDGE_SIZES for lay in ("none", "rand5", "rand5000", "bit0_bit31")]
                 + [(n, lay) for n in (64 * T + 1, LARGE) for lay in SINGLE]
                 + [(LARGE, "none"), (LARGE, "rand5000"), (LARGE, "last_tile")])


# ------------------------------------------------------------------ the cases
def _case_int64(dev, pattern, n, layout, mode):
    y = segmented_scan(_dev(pattern, n, dev), _flags(layout, n, mode, dev))
    assert y.dtype == torch.int64
    _assert_bits(y, _ref(pattern, layout, n))
    if layout == "all":
        assert torch.equal(y, _dev(pattern, n, dev))
    if layout == "none" and dev.type == "cuda":
        assert torch.equal(y, scan(_dev(pattern, n, dev), algo="lookback"))


def _case_float64_exact(dev, n, layout, mode):
    y = segmented_scan(_dev("f64_exact", n, dev), _flags(layout, n, mode, dev))
    assert y.dtype == torch.float64
    _assert_bits(y, _ref("f64_exact", layout, n))
    if layout == "none":  # the plain-scan oracle
        _assert_bits(y, np.cumsum(_x("f64_exact", n)))


def _case_float64_uniform(dev, n, layout, mode):
    ref, bound = _cached(("ld", layout, n), lambda: _longdouble_oracle(_x("f64_uniform", n), layout, n))
    _assert_bound(segmented_scan(_dev("f64_uniform", n, dev), _flags(layout, n, mode, dev)), ref, bound)


def _case_mul(dev, n, layout, mode):
    xi, mi = _x("wide", n), _x("mul_int", n)
    y = segmented_scan(_dev("wide", n, dev), _flags(layout, n, mode, dev), mul=_dev("mul_int", n, dev))
    _assert_bits(y, _cached(("refmul", layout, n), lambda: _vector_oracle(xi * mi, layout, n)))
    xf, mf = _x("f64_uniform", n), _x("mul_f64", n)
    if layout == "all":  # every element a head: out == x * mul, one correctly rounded product each
        y = segmented_scan(_dev("f64_uniform", n, dev), _flags(layout, n, mode, dev), mul=_dev("mul_f64", n, dev))
        _assert_bits(y, xf * mf)
        return
    ref, bound = _cached(("ldmul", layout, n), lambda: _longdouble_oracle(
        xf.astype(np.longdouble) * mf.astype(np.longdouble), layout, n, extra=1))
    _assert_bound(segmented_scan(_dev("f64_uniform", n, dev), _flags(layout, n, mode, dev),
                                 mul=_dev("mul_f64", n, dev)), ref, bound)


MUL_CASES = [(1, "none"), (3, "all"), (T + 1, "rand5"), (64 * T + 1, "rand5"), (64 * T + 1, "tile63_last"),
             (LARGE, "rand5000"), (LARGE, "all")]


# ------------------------------------------------------------------------ GPU
@pytest.mark.gpu
def test_large_size_walks_several_tiles_and_groups(gpu):
    """The large size gives more tiles than workgroups, so blocks walk several
    tiles, and more than 64 tiles, so the group level of the look-back runs."""
    from cme213x.ops.scan import segscan64_launch_info

    info = segscan64_launch_info(LARGE, gpu)
    assert info["tile"] == T
    assert info["tiles"] == (LARGE + T - 1) // T > 64
    assert info["tiles"] > info["workgroups"] >= 1, info
    assert info["workgroups"] % info["blocks_per_cu"] == 0 and info["ws_bytes"] >= 32 * info["tiles"]
    small = segscan64_launch_info(3, gpu)
    assert small["tiles"] == small["workgroups"] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", LAYOUT_CASES)
def test_segscan_int64_layouts_gpu(gpu, n, layout, mode):
    _case_int64(gpu, "wide", n, layout, mode)
    assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", PATTERN_LAYOUTS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("pattern", INT_PATTERNS)
def test_segscan_int64_patterns_gpu(gpu, pattern, n, layout, mode):
    _case_int64(gpu, pattern, n, layout, mode)
    assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", LAYOUT_CASES)
def test_segscan_float64_exact_gpu(gpu, n, layout, mode):
    _case_float64_exact(gpu, n, layout, mode)
    assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", UNIFORM_CASES)
def test_segscan_float64_uniform_gpu(gpu, n, layout, mode):
    _case_float64_uniform(gpu, n, layout, mode)
    assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", MUL_CASES)
def test_segscan_mul_gpu(gpu, n, layout, mode):
    _case_mul(gpu, n, layout, mode)
    assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", ["wide", "f64_exact"])
def test_segscan_in_place_gpu(gpu, kind, mode):
    n, layout = 64 * T + 1, "rand5000"
    x = _dev(kind, n, gpu).clone()
    m = _dev("mul_int", n, gpu).to(x.dtype)
    assert segmented_scan(x, _flags(layout, n, mode, gpu), out=x) is x
    _assert_bits(x, _ref(kind, layout, n))
    x.copy_(_dev(kind, n, gpu))
    segmented_scan(x, _flags(layout, n, mode, gpu), out=x, mul=m)
    _assert_bits(x, _vector_oracle(_x(kind, n) * _x("mul_int", n).astype(_x(kind, n).dtype), layout, n))
    assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", [T + 1, LARGE])
@pytest.mark.parametrize("kind", ["wide", "f64_exact"])
def test_segscan_8_byte_aligned_views_gpu(gpu, kind, n, mode):
    """x[1:], mul[1:] and out[1:] of 64-bit tensors are contiguous and 8-byte
    but not 16-byte aligned."""
    layout = "rand5000"
    xs = _x(kind, n)
    ms = _x("mul_int", n).astype(xs.dtype)
    base = torch.empty(n + 1, dtype=torch.from_numpy(xs).dtype, device=gpu)
    x, mul, out = base[1:], torch.empty_like(base)[1:], torch.empty_like(base)[1:]
    x.copy_(torch.from_numpy(xs))
    mul.copy_(torch.from_numpy(ms))
    assert all(t.is_contiguous() and t.data_ptr() % 16 == 8 for t in (x, mul, out))
    y = segmented_scan(x, _flags(layout, n, mode, gpu), out=out)
    assert y.data_ptr() == out.data_ptr()
    _assert_bits(out, _ref(kind, layout, n))
    segmented_scan(x, _flags(layout, n, mode, gpu), out=out, mul=mul)
    _assert_bits(out, _vector_oracle(xs * ms, layout, n))
    assert not lookback_timed_out(gpu)


def _case_poison_float64(dev):
    """An inf at the head and a NaN at the end of ONE segment, which ends at a
    lane-vector, wave-row, wave, tile or group boundary: every other segment,
    before and after, keeps its exact bits (the float32 twin is in
    test_segscan32.py)."""
    from scan_util import seg_exact_oracle

    n = 64 * T + T + 1
    x = _x("f64_exact", n)
    for end in (T + 8, T + 256, T + 1024, 2 * T, 64 * T):
        f = _heads("rand5000", n)
        f[end - 5:end + 1] = [1, 0, 0, 0, 0, 1]  # the poisoned segment [end - 5, end); the next starts at the boundary
        want = seg_exact_oracle(x, f, 2.0 ** 44)
        xp = x.copy()
        xp[end - 5] = np.inf
        xp[end - 1] = np.nan
        for mode in MODES:
            fl = torch.from_numpy(f if mode == "u8" else np.packbits(np.pad(f, (0, -n % 32)), bitorder="little")
                                  .view(np.int32).copy()).to(dev)
            y = segmented_scan(torch.from_numpy(xp).to(dev), fl).cpu().numpy()
            assert np.all(np.isinf(y[end - 5:end - 1])) and np.isnan(y[end - 1]), (end, mode)
            assert np.array_equal(_bits(y[:end - 5]), _bits(want[:end - 5])), (end, mode)
            assert np.array_equal(_bits(y[end:]), _bits(want[end:])), (end, mode)


@pytest.mark.gpu
def test_segscan_float64_poison_stays_in_its_segment_gpu(gpu):
    _case_poison_float64(gpu)
    assert not lookback_timed_out(gpu)


def test_segscan_float64_poison_stays_in_its_segment_cpu():
    _case_poison_float64(CPU)


# ------------------------------------------------------------- look-back state
def _rand_heads(gen, shape) -> torch.Tensor:
    return (torch.rand(shape, generator=gen) < 0.001).to(torch.uint8)


def _torch_oracle(x: torch.Tensor, f: torch.Tensor) -> torch.Tensor:
    """cumsum(v) - base[seg_id] along the last dimension (int64: exact)."""
    h = f.clone().long()
    h[..., 0] = 1
    c = torch.cumsum(x, -1)
    before = c - x  # the cumsum just before each element
    idx = torch.cummax(torch.where(h.bool(), torch.arange(x.shape[-1]).expand_as(h), 0), -1).values
    return c - torch.gather(before, -1, idx)


@pytest.mark.gpu
def test_segscan64_epochs_reuse_workspace(gpu):
    """200 back-to-back int64 segmented scans on one stream share one
    descriptor array, a new epoch per launch and no memset."""
    n = 3 * T + 5
    g = torch.Generator().manual_seed(21)
    xs = torch.randint(-2 ** 40, 2 ** 40, (200, n), generator=g, dtype=torch.int64)
    fs = _rand_heads(g, (200, n))
    xd, fd = xs.to(gpu), fs.to(gpu)
    outs = [segmented_scan(xd[i], fd[i]) for i in range(200)]
    assert not lookback_timed_out(gpu)
    assert torch.equal(torch.stack(outs).cpu(), _torch_oracle(xs, fs))


@pytest.mark.gpu
def test_scan_families_alternate_on_one_stream(gpu):
    """float32, int64 and float64 segmented scans and an int64 plain look-back
    scan issued back to back never read each other's descriptor words; every
    size spans more than 64 tiles (several groups of the two-level look-back)."""
    n32, n64, np64 = 65 * 4096 + 7, 65 * T + 3, 65 * 8192 + 3
    g = torch.Generator().manual_seed(22)
    rounds = []
    for _ in range(5):
        a = torch.randint(-50, 50, (n32,), generator=g, dtype=torch.int64)
        b = torch.randint(-2 ** 40, 2 ** 40, (n64,), generator=g, dtype=torch.int64)
        c = torch.randint(0, 2 ** 20, (n64,), generator=g, dtype=torch.int64)
        d = torch.randint(-2 ** 40, 2 ** 40, (np64,), generator=g, dtype=torch.int64)
        fa, fb = _rand_heads(g, (n32,)), _rand_heads(g, (n64,))
        fad, fbd = fa.to(gpu), fb.to(gpu)
        ya = segmented_scan(a.float().to(gpu), fad)  # |sums| < 2^24: exact in float32
        yb = segmented_scan(b.to(gpu), fbd)
        yc = segmented_scan(c.double().to(gpu), fbd)
        yd = scan(d.to(gpu), algo="lookback")
        rounds.append((ya, _torch_oracle(a, fa), yb, _torch_oracle(b, fb), yc, _torch_oracle(c, fb), yd,
                       torch.cumsum(d, 0)))
    assert not lookback_timed_out(gpu)
    for ya, ra, yb, rb, yc, rc, yd, rd in rounds:
        assert torch.equal(ya.cpu().long(), ra)
        assert torch.equal(yb.cpu(), rb)
        assert torch.equal(yc.cpu().long(), rc) and yc.dtype == torch.float64
        assert torch.equal(yd.cpu(), rd)


@pytest.mark.gpu
def test_segscan64_two_streams(gpu):
    n = 300 * T + 1
    g = torch.Generator().manual_seed(23)
    xs = [torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64) for _ in range(2)]
    fs = [_rand_heads(g, (n,)) for _ in range(2)]
    xd, fd = [x.to(gpu) for x in xs], [f.to(gpu) for f in fs]
    torch.cuda.synchronize(gpu)
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    outs = []
    for x, f, s in zip(xd, fd, streams):
        with torch.cuda.stream(s):
            outs.append(segmented_scan(x, f))
    assert not lookback_timed_out(gpu)  # synchronises the device
    for x, f, y in zip(xs, fs, outs):
        assert torch.equal(y.cpu(), _torch_oracle(x, f))


@pytest.mark.gpu
def test_graph_capture_segscan64(gpu):
    """An int64 and a float64 segmented scan (epoch 0: the descriptors are
    zeroed inside the graph) captured on a single stream; two replays on
    changed inputs and heads are exact, and so is an eager call in between."""
    n = 70 * T + 9
    g = torch.Generator().manual_seed(24)
    xi = torch.zeros(n, dtype=torch.int64, device=gpu)
    xf = torch.zeros(n, dtype=torch.float64, device=gpu)
    fl = torch.zeros(n, dtype=torch.uint8, device=gpu)
    oi, of = torch.empty_like(xi), torch.empty_like(xf)
    segmented_scan(xi, fl, out=oi)  # warm-up outside the capture
    segmented_scan(xf, fl, out=of)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        segmented_scan(xi, fl, out=oi)
        segmented_scan(xf, fl, out=of)
    for _ in range(2):
        a = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64)
        b = torch.randint(0, 2 ** 20, (n,), generator=g, dtype=torch.int64)
        f = _rand_heads(g, (n,))
        xi.copy_(a.to(gpu))
        xf.copy_(b.double().to(gpu))
        fl.copy_(f.to(gpu))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(oi.cpu(), _torch_oracle(a, f))
        assert torch.equal(of.cpu().long(), _torch_oracle(b, f))  # integer-valued, < 2^44: exact
        assert torch.equal(segmented_scan(xi, fl).cpu(), _torch_oracle(a, f))  # eager, between replays
    assert not lookback_timed_out(gpu)


# ------------------------------------------------------------------ rejections
def _rejections(dev):
    f = torch.zeros(100, dtype=torch.uint8, device=dev)
    for dt in (torch.int32, torch.float16):
        with pytest.raises(TypeError, match="float32.*int64.*float64"):
            segmented_scan(torch.ones(100, dtype=dt, device=dev), f)
    x = torch.ones(100, dtype=torch.float64, device=dev)
    with pytest.raises(ValueError, match="mul"):
        segmented_scan(x, f, mul=torch.ones(100, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError, match="mul"):
        segmented_scan(x.long(), f, mul=x)
    with pytest.raises(ValueError, match="mul"):
        segmented_scan(x, f, mul=x[:99])
    with pytest.raises(ValueError, match="out"):
        segmented_scan(x, f, out=torch.empty(100, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError, match="shorter"):
        segmented_scan(x, f[:50])


@pytest.mark.gpu
def test_rejected_inputs_gpu(gpu):
    _rejections(gpu)


def test_rejected_inputs_cpu():
    _rejections(CPU)


# ------------------------------------------------------- spmv_scan_run, float64
# (n, p, N) with heads from the final project's generator. Every value stays
# an integer below 2^53 in magnitude, so every summation order is exact:
#  * "general": a in [-3, 3], xx in {-1, 0, 1} at random. One step multiplies
#    the largest magnitude by at most the longest segment L, so 3 * L^N bounds
#    every partial sum; asserted below for the generated heads.
#  * "one_xx": xx is +-1 at ONE random position of each segment and 0 elsewhere,
#    so a step leaves a[l] * xx[l] (or 0) in every element: |a| <= 3 after any
#    number of steps -- the condition L^N cannot give for 70 or 130 steps.
# The oracle's values are asserted to be integers within that range.
RUN_SHAPES = [(37035, 3128, 6, "general"), (1_200_000, 200_000, 70, "one_xx"), (300_000, 20_000, 130, "one_xx")]


def _run_case(n, p, N, kind):
    def make():
        from cme213x.models.spmv_scan import generate

        s = generate(n, p, 1000, N, seed=n % 97).s.astype(np.int64)
        rng = np.random.default_rng(n % 89)
        a = rng.integers(-3, 4, n).astype(np.float64)
        lens = np.diff(s)
        seg = np.repeat(np.arange(lens.size), lens)
        if kind == "general":
            xx = rng.integers(-1, 2, n).astype(np.float64)
            limit = 3.0 * float(lens.max()) ** N
            assert limit < 2.0 ** 53, (lens.max(), N)
        else:
            xx = np.zeros(n)
            xx[s[:-1] + rng.integers(0, lens)] = rng.integers(0, 2, lens.size) * 2.0 - 1.0
            limit = 3.0
        ref = a.copy()
        for _ in range(N):
            # the running sum over the WHOLE array is taken in longdouble (64
            # mantissa bits), which holds n * limit exactly
            c = np.cumsum((ref * xx).astype(np.longdouble))
            assert np.abs(c).max() < 2.0 ** 63
            ref = (c - np.concatenate([np.zeros(1, np.longdouble), c])[s[:-1]][seg]).astype(np.float64)
            assert np.abs(ref).max() <= limit
        assert np.all(ref == np.rint(ref))
        return a, xx, torch.from_numpy(s), ref
    return _cached(("run", n, p, N), make)


def _case_run(dev, n, p, N, kind):
    a, xx, s, ref = _run_case(n, p, N, kind)
    flags = head_flags_from_offsets(s, n, dev)
    ad = torch.from_numpy(a).to(dev)
    y = spmv_scan_run(ad, torch.from_numpy(xx).to(dev), flags, N)
    assert y is ad and y.dtype == torch.float64
    _assert_bits(y, ref)


@pytest.mark.gpu
@pytest.mark.parametrize("n,p,N,kind", RUN_SHAPES)
def test_spmv_scan_run_float64_gpu(gpu, n, p, N, kind):
    _case_run(gpu, n, p, N, kind)
    assert not lookback_timed_out(gpu)


@pytest.mark.parametrize("n,p,N,kind", RUN_SHAPES)
def test_spmv_scan_run_float64_cpu(n, p, N, kind):
    _case_run(CPU, n, p, N, kind)


def test_spmv_scan_run_rejects_mixed_dtypes_cpu():
    a = torch.ones(10, dtype=torch.float64)
    f = torch.zeros(1, dtype=torch.int32)
    with pytest.raises(ValueError, match="dtype"):
        spmv_scan_run(a, a.float(), f, 1)
    with pytest.raises(TypeError, match="float32.*float64"):
        spmv_scan_run(a.long(), a.long(), f, 1)


# ------------------------------------------------------------------ CPU backend
CPU_SIZES = [1, 2, 3, T + 1, 64 * T + 1, 1_000_003]
CPU_LAYOUTS = [(n, lay) for n in CPU_SIZES for lay in LAYOUTS if _valid(lay, n)]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", CPU_LAYOUTS)
def test_segscan_int64_layouts_cpu(n, layout, mode):
    _case_int64(CPU, "wide", n, layout, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", PATTERN_LAYOUTS)
@pytest.mark.parametrize("n", CPU_SIZES)
@pytest.mark.parametrize("pattern", INT_PATTERNS)
def test_segscan_int64_patterns_cpu(pattern, n, layout, mode):
    _case_int64(CPU, pattern, n, layout, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", CPU_LAYOUTS)
def test_segscan_float64_exact_cpu(n, layout, mode):
    _case_float64_exact(CPU, n, layout, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", [c for c in UNIFORM_CASES if c[0] <= 64 * T + 1] + [(1_000_003, "rand5000")])
def test_segscan_float64_uniform_cpu(n, layout, mode):
    _case_float64_uniform(CPU, n, layout, mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n,layout", [c for c in MUL_CASES if c[0] < LARGE] + [(1_000_003, "rand5000")])
def test_segscan_mul_cpu(n, layout, mode):
    _case_mul(CPU, n, layout, mode)


def test_segscan_in_place_and_views_cpu():
    n, layout = T + 1, "rand5"
    for kind in ("wide", "f64_exact"):
        xs = _x(kind, n)
        f = _flags(layout, n, "u8", CPU)
        x = torch.from_numpy(xs.copy())
        assert segmented_scan(x, f, out=x) is x
        _assert_bits(x, _ref(kind, layout, n))
        base = torch.from_numpy(np.concatenate([xs[:1], xs]))
        out = torch.empty_like(base)[1:]
        assert segmented_scan(base[1:], f, out=out).data_ptr() == out.data_ptr()
        _assert_bits(out, _ref(kind, layout, n))


# ----------------------------------------------------------------- the drivers
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
SMALL_A, SMALL_X = os.path.join(DATA, "small_a.txt"), os.path.join(DATA, "small_x.txt")
# b.txt of `fp small_a.txt small_x.txt` on the CPU before --double existed
SMALL_B_F32 = b"5.4 3.36204 3.44204 -1.63036 "


@pytest.fixture
def in_tmp(tmp_path):
    old = os.getcwd()
    os.chdir(tmp_path)
    yield tmp_path
    os.chdir(old)


def _significant_digits(token: str) -> int:
    return len(token.lower().split("e")[0].replace("-", "").replace(".", "").lstrip("0"))


def test_fp_double_cli(in_tmp, capsys):
    """`fp a.txt x.txt check --double`: b.txt and b_cpu.txt carry 17
    significant digits, and the relative L2 error is at most 1e-12 -- a
    condition that tells float64 from float32 (3.2e-8 on this fixture), not a
    measurement -- both as fp reports it and as checker recomputes it from
    b.txt."""
    from cme213x.__main__ import main
    from cme213x.models.spmv_scan import errors, load, reference_solution

    assert main(["fp", SMALL_A, SMALL_X, "check", "--double"]) == 0
    out = capsys.readouterr().out
    rel = float(out.split("relative L2 error")[1].split(",")[0])
    assert rel <= 1e-12, out
    for name in ("b.txt", "b_cpu.txt"):
        toks = open(name).read().split()
        assert len(toks) == 4 and max(_significant_digits(t) for t in toks) == 17, toks
    prob = load(SMALL_A, SMALL_X, dtype=np.float64)
    b = np.fromfile("b.txt", sep=" ")
    assert errors(reference_solution(prob), b)["relL2"] <= 1e-12
    assert main(["checker", SMALL_A, SMALL_X, "b.txt", "--double"]) == 0  # reads a.txt / x.txt unrounded, as fp did
    out = capsys.readouterr().out
    assert float(out.split("Relative L2 error:")[1].split()[0]) <= 1e-12, out


def test_fp_default_output_is_unchanged_cpu(in_tmp):
    from cme213x.models.spmv_scan import run_fp

    res = run_fp(SMALL_A, SMALL_X, cpu_check=True, device="cpu")
    assert open("b.txt", "rb").read() == SMALL_B_F32
    assert open("b_cpu.txt", "rb").read() == SMALL_B_F32
    assert 1e-9 < res["relL2"] < 1e-6  # float32


def _fp_double_generated(device):
    from cme213x.models.spmv_scan import generate, run_fp, save

    prob = generate(37035, 3128, 1000, 6, seed=3, dtype=np.float64)
    assert prob.a.dtype == np.float64 and prob.x.dtype == np.float64
    save(prob, "a.txt", "x.txt")
    res = run_fp("a.txt", "x.txt", cpu_check=True, device=device, double=True)
    assert res["relL2"] <= 1e-12, res
    b = np.fromfile("b.txt", sep=" ")
    assert b.size == prob.n
    toks = open("b.txt").read().split()
    assert max(_significant_digits(t) for t in toks[:2000]) == 17
    return res


def test_fp_double_generated_cpu(in_tmp):
    _fp_double_generated("cpu")


@pytest.mark.gpu
def test_fp_double_generated_gpu(gpu, in_tmp):
    _fp_double_generated("cuda")
    assert not lookback_timed_out(gpu)
