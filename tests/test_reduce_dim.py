"""Reductions along one dimension (``reduce(x, op, dim=d, keepdim=,
return_indices=)``, ``argmax`` / ``argmin``) on the HIP and the CPU backend.

Oracles, none of them the code under test:

* integer sums: ``numpy.sum(axis=)`` in int64, reduced modulo 2^32 for the
  32-bit types; exact comparison, operands over the full range so sums wrap;
* float sums, exact tier: integers in [-8, 8] on lines of at most 2^20
  elements, so every association is exact (``|sum| < 2^23`` asserted on the
  float64 oracle); bitwise comparison, the sign of a zero left out as in
  ``scan_util.bits``;
* float sums, rounding tier: uniform(1, 2) on lines of at most 1024 elements
  against a longdouble sum under ``1.01 * n * u * sum|v|``. The bound is at most
  0.127 while every element, hence every chunk partial, is at least 1: a lost or
  doubled partial cannot hide under it. Asserted on the oracle;
* max / min, values only: NaN if the line holds one, else the element with the
  largest (smallest) order-preserving integer key of its bits, so that
  ``-0.0 < +0.0``; ``numpy.max`` / ``numpy.min`` for integers. Every bit is
  compared; the data holds only the default NaN;
* max / min with indices: ``torch.max`` / ``torch.min(x_cpu, dim)``, and
  ``numpy.argmax`` / ``numpy.argmin`` for uint32 and as the independent
  statement of "first NaN, else first equal" (the two are asserted equal).
  ``values`` is compared bitwise with ``x`` gathered at the oracle's index,
  ``indices`` exactly. The lines cycle through five kinds: a noisy ramp
  (rising, falling or flat) cut off so that a tenth of the line repeats the
  extreme exactly; the same with NaN on about 2 % of the elements; all
  ``-inf`` / type-minimum; one-signed values with zeros of both signs as the
  extreme; all ``+inf`` / type-maximum.

The GPU shapes are the smallest at which each mechanism can go wrong; their
edges come from ``reduce_dim_launch_info``: the tile of the row form (a
workgroup per line, a wave per line where there are many short lines), the
width of a workgroup and the unroll depth of the column form, and -- through
the ``scan_dim_chunks`` / ``scan_dim_maxblocks`` knobs -- the chunked regime
with both finish kernels and the grid-stride loops. The CPU backend chunks by
its thread count; it runs the same shapes. Nothing above 2^22 elements is
tested: the 64-bit index arithmetic is checked by reading the code.
"""
import contextlib

import numpy as np
import pytest
import torch

from cme213x.ops.scan import argmax, argmin, reduce, reduce_dim_launch_info
from scan_util import bits, to_numpy, to_torch

NP = {"f32": np.float32, "i32": np.int32, "u32": np.uint32, "i64": np.int64, "f64": np.float64}
TORCH = {"f32": torch.float32, "i32": torch.int32, "u32": torch.uint32, "i64": torch.int64, "f64": torch.float64}
ALL = list(NP)
MAIN = ["f32", "i64"]
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
WIDE_K = 40  # more chunks than a thread of the finish kernel folds alone: a workgroup per line


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def knobs(dev, **kw):
    """The launch-shape knobs of the HIP backend (the CPU backend has none)."""
    if dev.type != "cuda" or not kw:
        return contextlib.nullcontext()
    from cme213x.utils import tuning

    return tuning.override(**kw)


# ------------------------------------------------------------------ edges
def edges(dev, dt: str) -> dict:
    """Structural sizes of the launch, from the launch-info query on the GPU;
    the CPU backend gets fixed stand-ins of the same magnitude."""
    if dev.type != "cuda":
        return {"tile": 1024, "wave_tile": 256, "wave_rows": 1024, "vector": 4, "width": 512, "unroll": 8}
    d = TORCH[dt]
    block = reduce_dim_launch_info((3, 1 << 20), -1, dtype=d, device=dev)
    assert block["form"] == "row" and block["waves"] == 4
    rows = next(o for o in (1 << k for k in range(4, 14))
                if reduce_dim_launch_info((o, 65), -1, dtype=d, device=dev)["waves"] == 1)
    wave = reduce_dim_launch_info((rows, 65), -1, dtype=d, device=dev)
    col = reduce_dim_launch_info((3, 50, 64), 1, dtype=d, device=dev)
    assert col["form"] == "col" and col["vector"] == 16 // np.dtype(NP[dt]).itemsize
    return {"tile": block["tile"], "wave_tile": wave["tile"], "wave_rows": rows, "vector": col["vector"],
            "width": 256 * col["vector"], "unroll": col["tile"]}


# ------------------------------------------------------------------- data
def lowest(dtype):
    dtype = np.dtype(dtype)
    return dtype.type(-np.inf) if dtype.kind == "f" else np.iinfo(dtype).min


def highest(dtype):
    dtype = np.dtype(dtype)
    return dtype.type(np.inf) if dtype.kind == "f" else np.iinfo(dtype).max


def from_lines(a: np.ndarray, shape, axis: int) -> np.ndarray:
    """(lines, n) -> ``shape`` with the lines along ``axis``."""
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    return np.ascontiguousarray(a.reshape(outer, inner, shape[axis]).transpose(0, 2, 1)).reshape(shape)


def make_sum(shape, dt: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed + 17 * len(shape) + sum(shape))
    if dt in ("f32", "f64"):
        return rng.integers(-8, 9, shape).astype(NP[dt])  # exact tier
    if dt == "i64":
        return rng.integers(-2 ** 63, 2 ** 63 - 1, shape, dtype=np.int64)  # sums wrap modulo 2^64
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(NP[dt])  # wrap modulo 2^32


def make_ext(shape, axis: int, dt: str, op: str, seed: int = 0) -> np.ndarray:
    """Data of the max / min tests: see the module docstring."""
    rng = np.random.default_rng(seed + 31 * len(shape) + sum(shape))
    dtype = np.dtype(NP[dt])
    n = shape[axis]
    lines = int(np.prod(shape, dtype=np.int64)) // max(n, 1)
    line = np.arange(lines).reshape(-1, 1)
    slope = np.array([3, -3, 0])[(line // 5) % 3]  # the extreme late, early, anywhere
    v = slope * np.arange(n).reshape(1, -1) + rng.integers(-1000, 1001, (lines, n))
    cap = np.sort(v, axis=1)[:, [(9 * n) // 10]]
    v = np.minimum(v, cap)  # a tenth of the line repeats the extreme
    if dtype.kind == "f":
        v = np.minimum(v + 0.25 * rng.integers(0, 4, (lines, n)), cap)
        zeros = np.where((line % 5 == 3), -np.abs(v), v)
        r = rng.random((lines, n))
        zeros[(line % 5 == 3) & (r < 0.05)] = 0.0
        zeros[(line % 5 == 3) & (r > 0.95)] = -0.0
        v = zeros
    elif dtype == np.uint32:
        v = v - v.min() + 5
    v = v if op == "max" else (0xFFFFFFFF - v if dtype == np.uint32 else -v)
    v = v.astype(dtype)
    if dtype.kind == "f":
        v[(line % 5 == 1) & (rng.random((lines, n)) < 0.02)] = np.nan
    v[(line % 5 == 2)[:, 0]] = lowest(dtype)
    v[(line % 5 == 4)[:, 0]] = highest(dtype)
    return from_lines(v, shape, axis)


def view_at(x: np.ndarray, offset: int, dev) -> torch.Tensor:
    """``x`` on ``dev``; with ``offset``, starting that many elements into its
    buffer (a contiguous view aligned to the element only)."""
    if not offset:
        return to_torch(x, dev)
    base = torch.zeros(x.size + offset, dtype=to_torch(x.reshape(-1)[:1], "cpu").dtype, device=dev)
    xt = base[offset:].view(x.shape)
    xt.copy_(to_torch(x, dev))
    assert xt.is_contiguous() and xt.data_ptr() == base.data_ptr() + offset * x.itemsize
    return xt


# ---------------------------------------------------------------- oracles
def raw(a: np.ndarray) -> np.ndarray:
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "f" else a


def sum_oracle(x: np.ndarray, axis: int) -> np.ndarray:
    if x.dtype.kind == "f":
        s = np.sum(x.astype(np.float64), axis=axis)
        assert x.shape[axis] <= 2 ** 20 and np.all(s == np.rint(s)) and np.abs(s).max(initial=0) < 2.0 ** 23
        return s.astype(x.dtype)
    s = np.sum(x.astype(np.int64), axis=axis, dtype=np.int64)
    if x.itemsize == 4:
        return (s & 0xFFFFFFFF).astype(np.uint32).view(x.dtype)
    return s


def value_oracle(x: np.ndarray, axis: int, op: str) -> np.ndarray:
    """IEEE maximum / minimum of every line, from the ordered keys of the bits."""
    if x.dtype.kind != "f":
        return (np.max if op == "max" else np.min)(x, axis=axis)
    b = raw(x)
    info = np.iinfo(b.dtype)
    key = b ^ ((b >> (8 * x.itemsize - 1)) & info.max)  # -0.0 just below +0.0, monotone otherwise
    nan = np.isnan(x)
    key = np.where(nan, info.min if op == "max" else info.max, key)
    at = (np.argmax if op == "max" else np.argmin)(key, axis=axis)
    r = np.take_along_axis(x, np.expand_dims(at, axis), axis).squeeze(axis)
    r[nan.any(axis=axis)] = np.nan
    return r


def index_oracle(x: np.ndarray, axis: int, op: str):
    """(x at the index, index) of torch.max / torch.min(x, dim) on CPU tensors;
    numpy states the same rule and is all there is for uint32."""
    at = (np.argmax if op == "max" else np.argmin)(x, axis=axis).astype(np.int64)
    if x.dtype != np.uint32:
        t = (torch.max if op == "max" else torch.min)(torch.from_numpy(x.copy()), axis).indices.numpy()
        assert np.array_equal(t, at), "torch and numpy disagree on the index rule"
    return np.take_along_axis(x, np.expand_dims(at, axis), axis).squeeze(axis), at


def assert_same(got, want: np.ndarray, key, what) -> None:
    g = to_numpy(got) if isinstance(got, torch.Tensor) else got
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    bad = np.flatnonzero(key(g).reshape(-1) != key(want).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at flat index {bad[0]}: "
                           f"{g.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}")


def check_ext(dev, x: np.ndarray, xt: torch.Tensor, dim, what, ops=("max", "min")) -> None:
    """Values-only and indexed max / min of ``xt`` (``x`` on the device)."""
    axis = None if dim is None else dim % x.ndim
    flat, fax = (x.reshape(-1), 0) if dim is None else (x, axis)
    for op in ops:
        assert_same(reduce(xt, op, dim=dim, keepdim=False, return_indices=False) if dim is not None
                    else reduce(xt.reshape(-1), op, dim=0), value_oracle(flat, fax, op), raw, (what, op, "values"))
        want_v, want_i = index_oracle(flat, fax, op)
        v, i = reduce(xt, op, dim=dim, return_indices=True)
        assert i.dtype == torch.int64 and i.device == xt.device
        assert_same(i, want_i, raw, (what, op, "indices"))
        assert_same(v, want_v, raw, (what, op, "values at the indices"))
        only = (argmax if op == "max" else argmin)(xt, dim)
        assert torch.equal(only, i), (what, op, "argmax / argmin against the pair")


def check(dev, shape, dim: int, dt: str, seed: int = 0, offset: int = 0, ops=("sum", "max", "min")) -> None:
    """reduce(dim=) of fresh data against the oracles: the sum, the values-only
    and the indexed max / min, argmax / argmin. ``offset``: the operand starts
    that many elements into its buffer."""
    axis = dim % len(shape)
    what = (shape, dim, dt, offset)
    if "sum" in ops:
        x = make_sum(shape, dt, seed)
        got = reduce(view_at(x, offset, dev), "sum", dim=dim)
        assert_same(got, sum_oracle(x, axis), bits, (what, "sum"))
    for op in ops:
        if op != "sum":
            x = make_ext(shape, axis, dt, op, seed)
            check_ext(dev, x, view_at(x, offset, dev), dim, what, ops=(op,))


# --------------------------------------------------------------- row form
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_workgroup_per_line(dev, dt):
    """n around the tile (-1, 0, +1, two tiles + 1) and small odd n (rows start
    off 16-byte alignment), for 1 (a single line), 3 and 7 rows."""
    tile = edges(dev, dt)["tile"]
    for outer in (1, 3, 7):
        for n in (1, 2, 3, 65, 257, tile - 1, tile, tile + 1, 2 * tile + 1):
            check(dev, (outer, n), -1, dt)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_wave_per_line(dev, dt):
    """Many short rows: a wave per row on the GPU."""
    e = edges(dev, dt)
    rows, tile = e["wave_rows"], e["wave_tile"]
    if dev.type == "cuda":
        for ind in (False, True):
            info = reduce_dim_launch_info((rows + 3, 2 * tile + 3), -1, dtype=TORCH[dt], device=dev, indices=ind)
            assert info["waves"] == 1 and info["chunks"] == 1 and info["ws_bytes"] == 0
    for n in (1, 65, tile - 1, tile, tile + 1, 2 * tile + 3):
        check(dev, (rows + 3, n), -1, dt)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_grid_stride(dev, dt):
    """Two workgroups for all the rows: each goes round its row loop many
    times, in both row kernels."""
    e = edges(dev, dt)
    with knobs(dev, scan_dim_maxblocks=2):
        if dev.type == "cuda":
            assert reduce_dim_launch_info((67, 257), -1, dtype=TORCH[dt], device=dev)["workgroups"] == 2
        check(dev, (67, 257), -1, dt)
        check(dev, (67, e["tile"] + 1), -1, dt)
        check(dev, (e["wave_rows"] + 3, 65), -1, dt)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [3, WIDE_K])
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_chunked(dev, dt, chunks):
    """Partials and the finish kernel (a thread per line for 3 chunks, a
    workgroup per line for 40): n not divisible by K, a short last chunk, n < K
    (empty chunks), chunks of several tiles, a single line."""
    tile = edges(dev, dt)["tile"]
    size = np.dtype(NP[dt]).itemsize
    with knobs(dev, scan_dim_chunks=chunks):
        if dev.type == "cuda":
            info = reduce_dim_launch_info((3, 100), -1, dtype=TORCH[dt], device=dev)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * size
            info = reduce_dim_launch_info((3, 100), -1, dtype=TORCH[dt], op="min", device=dev, indices=True)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * (size + 8)
        for n in (2, 5, 100, tile + 1, 3 * tile + 5):
            check(dev, (3, n), -1, dt)
        check(dev, (1, 3 * tile + 5), -1, dt)
        check(dev, (3 * tile + 4,), 0, dt)


# ------------------------------------------------------------ column form
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form(dev, dt):
    """inner around the width of a workgroup of lane vectors (256 * vector
    - 1, 0, + 1) and not a multiple of the vector (scalar lanes); n around the
    unroll depth and n == 1."""
    e = edges(dev, dt)
    w, u = e["width"], e["unroll"]
    for outer in (1, 3):
        for inner in (2, 3, 5, 64, w - 1, w, w + 1):
            for n in (1, u - 1, u, u + 1, 129):
                if outer == 3 and n in (u - 1, u):
                    continue
                check(dev, (outer, n, inner), 1, dt)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_forced_scalar(dev, dt):
    """inner divisible by the lane vector, but the operand starts one element
    off 16-byte alignment: the scalar mapping."""
    if dev.type == "cuda":
        assert reduce_dim_launch_info((3, 9, 64), 1, dtype=TORCH[dt], device=dev)["vector"] > 1
    for shape in ((3, 9, 64), (1, 129, 4), (2, 10, 256)):
        check(dev, shape, 1, dt, offset=1)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [3, WIDE_K])
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_chunked(dev, dt, chunks):
    size = np.dtype(NP[dt]).itemsize
    with knobs(dev, scan_dim_chunks=chunks):
        if dev.type == "cuda":
            info = reduce_dim_launch_info((3, 100, 64), 1, dtype=TORCH[dt], device=dev)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * 64 * size
            info = reduce_dim_launch_info((3, 100, 64), 1, dtype=TORCH[dt], device=dev, indices=True)
            assert info["ws_bytes"] == 3 * chunks * 64 * (size + 8)
        for outer in (1, 3):
            for inner in (3, 64, 65):
                for n in (2, 5, 100, 129):
                    check(dev, (outer, n, inner), 1, dt)
        check(dev, (2, 100, 64), 1, dt, offset=1)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_grid_stride(dev, dt):
    with knobs(dev, scan_dim_maxblocks=2):
        check(dev, (3, 17, 1025), 1, dt)
        check(dev, (3, 17, 1024), 1, dt)
        with knobs(dev, scan_dim_chunks=3):  # the finish kernel's loop over the lines as well
            check(dev, (3, 17, 1025), 1, dt)


# ------------------------------------------------------- shapes and dtypes
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_rank_one_to_four_every_dim_and_keepdim(dev, dt):
    for shape in ((37,), (5, 37), (5, 37, 9), (2, 3, 19, 8)):
        for d in range(-len(shape), len(shape)):
            check(dev, shape, d, dt)
            x = make_ext(shape, d % len(shape), dt, "max")
            xt = to_torch(x, dev)
            kept = tuple(1 if a == d % len(shape) else s for a, s in enumerate(shape))
            s = reduce(xt, "sum", dim=d, keepdim=True)
            v, i = reduce(xt, "max", dim=d, keepdim=True, return_indices=True)
            assert s.shape == v.shape == i.shape == argmin(xt, d, keepdim=True).shape == torch.Size(kept)
            v0, i0 = reduce(xt, "max", dim=d, return_indices=True)
            assert torch.equal(i.squeeze(d), i0) and np.array_equal(raw(to_numpy(v.squeeze(d))), raw(to_numpy(v0)))
            assert np.array_equal(raw(to_numpy(s.squeeze(d))), raw(to_numpy(reduce(xt, "sum", dim=d))))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", ALL)
def test_every_dtype_in_every_regime(dev, dt):
    e = edges(dev, dt)
    tile = e["tile"]
    check(dev, (5, 301), -1, dt)  # row, single pass
    check(dev, (e["wave_rows"] + 1, 67), -1, dt)  # row, a wave per line
    check(dev, (3, 50, 64), 1, dt)  # column, lane vectors
    check(dev, (3, 50, 65), 1, dt)  # column, scalar lanes
    with knobs(dev, scan_dim_chunks=3):
        check(dev, (3, 2 * tile + 3), -1, dt)  # row, chunked
        check(dev, (3, 129, 64), 1, dt)  # column, chunked
        check(dev, (3, 129, 65), 1, dt)
    with knobs(dev, scan_dim_chunks=WIDE_K):
        check(dev, (2, 2 * tile + 3), -1, dt)  # a workgroup of the finish kernel per line


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", ALL)
def test_views_aligned_to_the_element_only(dev, dt):
    """x[1:], x[2:], x[3:]: 4- and 8-byte phases of the 16-byte lane vectors."""
    for off in (1, 2, 3):
        check(dev, (5, 301), 1, dt, offset=off)
        check(dev, (3, 50, 64), 1, dt, offset=off)
        check(dev, (3, 21, 5), 1, dt, offset=off)
    with knobs(dev, scan_dim_chunks=3):
        check(dev, (3, 1001), 1, dt, offset=1)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("dt", MAIN)
def test_where_the_extreme_sits(dev, dt, chunks):
    """One extreme, then the same value twice, at: the first and last element
    (the masked head / tail vectors of a view at x[1:]), the vectors next to
    them, the first and the last chunk. The pair names the first of the two."""
    tile = edges(dev, dt)["tile"]
    n = 3 * tile + 5
    rng = np.random.default_rng(3)
    spots = (0, 1, 2, 3, 4, 5, n // 3 - 1, n // 3, n // 3 + 1, n - 6, n - 5, n - 4, n - 3, n - 2, n - 1)
    for shape, dim in (((len(spots), n), 1), ((n, len(spots)), 0)):
        base = rng.integers(-100, 101, shape).astype(NP[dt])
        for op, peak in (("max", 1000), ("min", -1000)):
            one, two = base.copy(), base.copy()
            for line, p in enumerate(spots):
                at = (line, p) if dim == 1 else (p, line)
                one[at] = two[at] = peak
                later = spots[(line + 4) % len(spots)]
                if later > p:
                    two[(line, later) if dim == 1 else (later, line)] = peak
            for x in (one, two):
                with knobs(dev, scan_dim_chunks=chunks):
                    v, i = reduce(view_at(x, 1, dev), op, dim=dim, return_indices=True)
                    flat = reduce(view_at(x, 1, dev), op, dim=dim)
                assert np.array_equal(to_numpy(i), np.array(spots)), (shape, op, to_numpy(i))
                assert (to_numpy(v) == peak).all() and (to_numpy(flat) == peak).all()


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_flattened_with_indices_and_non_contiguous(dev):
    """dim=None with indices against torch.argmax / argmin of the flattened
    tensor: 0-d results; a single line of all -inf still has index 0; a
    transposed operand is copied."""
    for dt in MAIN:
        for shape in ((7, 300), (40_001,), (3, 5, 7)):
            for op, targ in (("max", torch.argmax), ("min", torch.argmin)):
                x = make_ext((int(np.prod(shape)),), 0, dt, op, seed=len(shape)).reshape(shape)
                xt = to_torch(x, dev)
                v, i = reduce(xt, op, return_indices=True)
                assert v.shape == i.shape == torch.Size(()) and i.dtype == torch.int64
                want = int(targ(torch.from_numpy(x.copy())))
                assert int(i) == want and int((argmax if op == "max" else argmin)(xt)) == want
                assert raw(to_numpy(v)) == raw(x.reshape(-1)[want])
                k = reduce(xt, op, keepdim=True, return_indices=True)
                assert k.values.shape == k.indices.shape == torch.Size((1,) * len(shape)) and int(k.indices) == want
        check_ext(dev, x.reshape(-1), to_torch(x.reshape(-1), dev), None, "flat")
    for fill, op in ((-np.inf, "max"), (np.inf, "min"), (np.nan, "max")):
        v, i = reduce(torch.full((5000,), fill, device=dev), op, return_indices=True)
        assert int(i) == 0 and raw(to_numpy(v)) == raw(np.float32(fill))
    a = make_ext((37, 53), 0, "f32", "max")
    t = to_torch(a, dev).t()
    assert not t.is_contiguous()
    check_ext(dev, np.ascontiguousarray(a.T), t, 1, "transposed")
    s = make_sum((37, 53), "i64")
    assert np.array_equal(to_numpy(reduce(to_torch(s, dev).t(), "sum", dim=0)), sum_oracle(s.T, 0))


# ---------------------------------------------------------- rounding tier
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_float_sums_round_within_the_bound(dev, dt, chunks):
    u = 2.0 ** -24 if dt == "f32" else 2.0 ** -53
    rng = np.random.default_rng(5)
    for shape, dim in (((5, 1024), 1), ((3, 1021), 1), ((1024, 67), 0), ((2, 1000, 4), 1), ((1023,), 0)):
        v = rng.uniform(1.0, 2.0, shape).astype(NP[dt])
        wide = v.astype(np.longdouble)
        ref = np.sum(wide, axis=dim)
        bound = (1.01 * u * shape[dim] * np.sum(np.abs(wide), axis=dim)).astype(np.float64)
        # on the oracle alone: a whole element (hence a whole chunk partial) does not fit under the bound
        assert shape[dim] <= 1024 and bound.max() <= 0.127 and v.min() >= 1.0
        with knobs(dev, scan_dim_chunks=chunks):
            got = to_numpy(reduce(to_torch(v, dev), "sum", dim=dim)).astype(np.longdouble)
        err = np.abs(got - ref).astype(np.float64)
        assert np.all(err <= bound), (shape, dim, float((err - bound).max()))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_float_sums_repeat_bit_for_bit(dev, dt):
    """Two consecutive runs of one call, in every regime."""
    e = edges(dev, dt)
    rng = np.random.default_rng(21)
    cases = [((5, 3 * e["tile"] + 7), 1, {}), ((e["wave_rows"] + 3, 67), 1, {}), ((3, 129, 64), 1, {}),
             ((3, 129, 65), 1, {}), ((3, 20_011), 1, {"scan_dim_chunks": 7}), ((3, 1001, 64), 1, {"scan_dim_chunks": 7}),
             ((3, 20_011), 1, {"scan_dim_chunks": WIDE_K}), ((1 << 20,), 0, {}), ((1 << 18, 4), 0, {})]
    for shape, dim, kn in cases:
        x = to_torch(rng.uniform(-1, 1, shape).astype(NP[dt]), dev)
        with knobs(dev, **kn):
            first, second = reduce(x, "sum", dim=dim), reduce(x, "sum", dim=dim)
        assert np.array_equal(raw(to_numpy(first)), raw(to_numpy(second))), (shape, kn)
        wide = to_numpy(x).astype(np.longdouble)  # and the runs are sums: the worst-case bound of any order
        bound = 1.01 * shape[dim] * (2.0 ** -24 if dt == "f32" else 2.0 ** -53) * np.sum(np.abs(wide), axis=dim)
        assert np.all(np.abs(to_numpy(first).astype(np.longdouble) - np.sum(wide, axis=dim)) <= bound), (shape, kn)


# ------------------------------------------------------ rules at the edges
@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_empty_shapes(dev):
    for shape, dim in (((3, 0), 1), ((2, 0, 3), 1), ((0,), 0), ((0,), None), ((0, 0), 1)):
        x = torch.zeros(shape, dtype=torch.int64, device=dev)
        want = torch.zeros(shape, dtype=torch.int64).sum() if dim is None else torch.zeros(shape, dtype=torch.int64).sum(dim)
        got = reduce(x, "sum", dim=dim, keepdim=dim is None)
        assert got.dtype == torch.int64 and (got == 0).all()
        assert got.shape == (want.shape if dim is not None else torch.Size((1,) * len(shape)))
        for op in ("max", "min"):
            with pytest.raises(ValueError):
                reduce(x, op, dim=dim, keepdim=True)
            with pytest.raises(ValueError):
                reduce(x, op, dim=dim, return_indices=True)
        with pytest.raises(ValueError):
            argmax(x, dim)
    for shape, dim, left in (((0, 4), 1, (0,)), ((2, 3, 0), 1, (2, 0)), ((0, 4, 3), 1, (0, 3))):
        x = torch.zeros(shape, device=dev)
        for op in ("sum", "max", "min"):
            assert reduce(x, op, dim=dim).shape == torch.Size(left)
        v, i = reduce(x, "min", dim=dim, return_indices=True)
        assert v.shape == i.shape == torch.Size(left) and i.dtype == torch.int64
        assert argmin(x, dim, keepdim=True).shape == torch.Size(left[:1] + (1,) + left[1:])


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_rejected_arguments(dev):
    x = torch.arange(12, dtype=torch.float32, device=dev).view(3, 4)
    with pytest.raises(ValueError, match="sum"):
        reduce(x, "sum", dim=1, return_indices=True)
    with pytest.raises(ValueError, match="sum"):
        reduce(x, "sum", return_indices=True)
    with pytest.raises(TypeError, match="algo"):
        reduce(x, "sum", algo="tree", dim=1)
    with pytest.raises(TypeError, match="algo"):
        reduce(x, "max", algo="tree", return_indices=True)
    with pytest.raises(TypeError):
        reduce(x.half(), "sum", dim=0)
    with pytest.raises(TypeError):
        argmax(x.to(torch.int16), 0)
    with pytest.raises(ValueError, match="op"):
        reduce(x, "prod", dim=0)
    for d in (2, -3):
        with pytest.raises(IndexError):
            reduce(x, "sum", dim=d)
        with pytest.raises(IndexError):
            argmin(x, d)
    with pytest.raises(ValueError):
        reduce(torch.tensor(1.0, device=dev), "sum", dim=0)
    assert torch.equal(reduce(x, "sum", dim=-1), reduce(x, "sum", dim=1))
    assert torch.equal(reduce(x, "sum", dim=0).cpu(), x.cpu().sum(0))
    # a 0-d tensor is a line of one element
    v, i = reduce(torch.tensor(2.5, device=dev), "min", return_indices=True)
    assert float(v) == 2.5 and int(i) == 0 and v.shape == torch.Size(())


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_the_flattened_reduce_is_what_it_was(dev):
    """reduce(x, op) without the new arguments: the untouched path against
    torch.sum / amax / amin of exact-tier data, a 0-d tensor, "tree" included."""
    for dt in ("f32", "i64"):
        x = make_sum((7, 3001), "f32", seed=2).astype(NP[dt])
        xt, xc = to_torch(x, dev), torch.from_numpy(x)
        for op, f in (("sum", torch.sum), ("max", torch.amax), ("min", torch.amin)):
            got = reduce(xt, op)
            assert isinstance(got, torch.Tensor) and got.shape == torch.Size(()) and got.dtype == xt.dtype
            assert got.cpu() == f(xc)
    if dev.type == "cuda":
        assert reduce(xt.float(), "sum", "tree").cpu() == xc.float().sum()
        with pytest.raises(TypeError):
            reduce(xt, "sum", "tree")  # int64: "vector" only
    with pytest.raises(KeyError):
        reduce(torch.zeros(4, dtype=torch.uint32, device=dev))  # its dtype table has no uint32


# ------------------------------------------------------------------ GPU only
@pytest.mark.gpu
def test_launch_info_names_the_regimes(gpu):
    keys = {"form", "outer", "n", "inner", "chunks", "chunk", "tile", "vector", "waves", "workgroups", "ws_bytes"}
    flat = reduce_dim_launch_info((1 << 22,), None, device=gpu)
    assert keys <= set(flat) and flat["form"] == "flat" and flat["waves"] == 4
    assert flat["chunks"] > 1 and flat["ws_bytes"] == flat["chunks"] * 4 and flat["workgroups"] == flat["chunks"]
    pair = reduce_dim_launch_info((1 << 22,), 0, device=gpu, indices=True)
    assert pair["chunks"] == flat["chunks"] and pair["ws_bytes"] == flat["chunks"] * 12
    row = reduce_dim_launch_info((65536, 2048), -1, device=gpu)
    assert (row["form"], row["outer"], row["n"], row["inner"], row["chunks"], row["ws_bytes"]) == ("row", 65536, 2048, 1, 1, 0)
    long_rows = reduce_dim_launch_info((16, 1 << 22), -1, dtype=torch.float64, device=gpu)
    assert long_rows["chunks"] > 1 and long_rows["ws_bytes"] == 16 * long_rows["chunks"] * 8
    assert long_rows["chunks"] * long_rows["chunk"] >= 1 << 22 and long_rows["chunk"] % long_rows["tile"] == 0
    wide = reduce_dim_launch_info((64, 1 << 21), 0, device=gpu)
    assert (wide["form"], wide["chunks"]) == ("col", 1)
    thin = reduce_dim_launch_info((1 << 21, 64), 0, dtype=torch.int64, device=gpu, indices=True)
    assert thin["form"] == "col" and thin["chunks"] > 1 and thin["vector"] == 2
    assert thin["ws_bytes"] == thin["chunks"] * 64 * 16
    assert reduce_dim_launch_info((4, 0, 3), 1, device=gpu)["workgroups"] == 0
    with pytest.raises(IndexError):
        reduce_dim_launch_info((4, 3), 2, device=gpu)


@pytest.mark.gpu
def test_natural_chunking_of_long_lines(gpu):
    """No knob: a single line of 2^20 elements, 16 long rows and a few long
    columns split along n by the plan's own rule; sum, values-only and indexed
    extremes."""
    for shape, dim in (((1 << 20,), 0), ((16, 1 << 16), 1), ((1 << 16, 8), 0)):
        assert reduce_dim_launch_info(shape, dim, device=gpu)["chunks"] > 1
        check(gpu, shape, dim, "f32")
    check(gpu, (1 << 16, 6), 0, "i64")
