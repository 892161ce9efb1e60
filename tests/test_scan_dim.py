"""Scans along one dimension (``scan(x, dim=d)``, ``cummax`` / ``cummin`` with
``dim=``, ``summed_area_table``) on the HIP and the CPU backend.

Oracles, none of them the code under test:

* integers: ``numpy.cumsum(axis=)`` in int64, reduced modulo 2^32 for the
  32-bit types; exact comparison;
* float sums, exact tier: integer values in [-8, 8] on lines of at most 2^20
  elements, so every partial sum in any association is an integer below 2^24
  (asserted on the float64 oracle); bitwise comparison, the sign of a zero
  left out as in ``scan_util.bits``;
* float sums, rounding tier: uniform(1, 2) values on lines of at most 1024
  elements against a longdouble ``cumsum`` under ``1.01 * m * u * cumsum|v|``
  (``m`` the 1-based position on the line). The bound is at most 0.127 while
  every element, hence every non-empty chunk total, is at least 1: a lost,
  doubled or misplaced carry cannot hide under it. Asserted on the oracle;
* max / min: ``torch.cummax`` / ``torch.cummin`` on CPU tensors and
  ``numpy.maximum.accumulate`` for uint32; every bit compared. The data is a
  noisy ramp along the scanned dimension (mirrored for "min"), so the running
  value changes all along the line and a dropped carry shows.

The GPU shapes are the smallest at which each mechanism can go wrong, and
their edges come from ``scan_dim_launch_info``: the tile of the row form (a
workgroup per line, and a wave per line where there are many short lines), the
width of a workgroup and the unroll depth of the column form, and -- through
the ``scan_dim_chunks`` / ``scan_dim_maxblocks`` knobs -- the chunked
reduce-then-scan and the grid-stride loops. The CPU backend chunks by its
thread count; it runs the same shapes. Tensors above 2^31 elements are not
tested: the 64-bit index arithmetic is checked by reading the code.
"""
import contextlib

import numpy as np
import pytest
import torch

from cme213x.ops.scan import cummax, cummin, scan, scan_dim_launch_info, summed_area_table
from scan_util import bits, to_numpy, to_torch

NP = {"f32": np.float32, "i32": np.int32, "u32": np.uint32, "i64": np.int64, "f64": np.float64}
TORCH = {"f32": torch.float32, "i32": torch.int32, "u32": torch.uint32, "i64": torch.int64, "f64": torch.float64}
ALL = list(NP)
MAIN = ["f32", "i64"]
OPS = ["sum", "max", "min"]
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]


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
    """Structural sizes of the launch, from the launch-info query on the GPU.
    The CPU backend walks blocks of 512 columns and has no tile along a row;
    it gets fixed stand-ins of the same magnitude."""
    if dev.type != "cuda":
        return {"tile": 1024, "wave_tile": 256, "wave_rows": 1024, "vector": 4, "width": 512, "unroll": 8}
    d = TORCH[dt]
    block = scan_dim_launch_info((3, 1 << 20), -1, dtype=d, device=dev)
    assert block["form"] == "row" and block["waves"] == 4
    rows = next(o for o in (1 << k for k in range(4, 14))
                if scan_dim_launch_info((o, 65), -1, dtype=d, device=dev)["waves"] == 1)
    wave = scan_dim_launch_info((rows, 65), -1, dtype=d, device=dev)
    col = scan_dim_launch_info((3, 50, 64), 1, dtype=d, device=dev)
    assert col["form"] == "col" and col["vector"] == 16 // np.dtype(NP[dt]).itemsize
    return {"tile": block["tile"], "wave_tile": wave["tile"], "wave_rows": rows, "vector": col["vector"],
            "width": 256 * col["vector"], "unroll": col["tile"]}


# ------------------------------------------------------------------- data
def identity(op: str, dtype):
    dtype = np.dtype(dtype)
    if op == "sum":
        return dtype.type(0)
    if dtype.kind == "f":
        return dtype.type(-np.inf if op == "max" else np.inf)
    info = np.iinfo(dtype)
    return dtype.type(info.min if op == "max" else info.max)


def make(shape, axis: int, dt: str, op: str, seed: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed + 17 * len(shape) + sum(shape))
    dtype = NP[dt]
    if op == "sum":
        if dt in ("f32", "f64"):
            return rng.integers(-8, 9, shape).astype(dtype)  # exact tier
        if dt == "i64":
            return rng.integers(-2 ** 62, 2 ** 62, shape, dtype=np.int64)  # sums wrap modulo 2^64
        return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32).view(dtype)  # wrap modulo 2^32
    # noisy ramp along the scanned axis, a different offset on every line
    idx = np.arange(shape[axis], dtype=np.int64).reshape([-1 if a == axis else 1 for a in range(len(shape))])
    v = 3 * idx + rng.integers(-50, 51, shape) + rng.integers(0, 1000, shape).take([0], axis)
    if dt == "u32":
        v = v + 100
        return (v if op == "max" else 0xFFFFFFFF - v).astype(np.uint32)
    if dt[0] == "f":
        v = v + rng.uniform(-0.5, 0.5, shape)
        v[rng.random(shape) < 0.02] = 0.0  # zeros of both signs: the later of two equal values wins
        v[rng.random(shape) < 0.02] = -0.0
    return (v if op == "max" else -v).astype(dtype)


def oracle(x: np.ndarray, axis: int, op: str) -> np.ndarray:
    """Inclusive result in x's dtype."""
    if op == "sum":
        if x.dtype.kind == "f":
            c = np.cumsum(x.astype(np.float64), axis=axis)
            assert x.shape[axis] <= 2 ** 20 and np.all(c == np.rint(c)) and np.abs(c).max(initial=0) < 2.0 ** 23
            return c.astype(x.dtype)
        c = np.cumsum(x.astype(np.int64), axis=axis, dtype=np.int64)
        if x.itemsize == 4:
            return (c & 0xFFFFFFFF).astype(np.uint32).view(x.dtype)
        return c
    if x.dtype == np.uint32:
        return (np.maximum if op == "max" else np.minimum).accumulate(x, axis=axis)
    f = torch.cummax if op == "max" else torch.cummin
    return f(torch.from_numpy(x.copy()), axis).values.numpy()


def excl_of(inc: np.ndarray, axis: int, op: str) -> np.ndarray:
    first = np.full_like(inc.take([0], axis), identity(op, inc.dtype))
    return np.concatenate([first, inc.take(np.arange(inc.shape[axis] - 1), axis)], axis=axis)


def raw(a: np.ndarray) -> np.ndarray:
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "f" else a


def assert_same(got, want: np.ndarray, op: str, what) -> None:
    g = to_numpy(got) if isinstance(got, torch.Tensor) else got
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    key = bits if op == "sum" else raw  # sums: the sign of a zero is left out
    bad = np.flatnonzero(key(g).reshape(-1) != key(want).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at flat index {bad[0]}: "
                           f"{g.reshape(-1)[bad[0]]!r} != {want.reshape(-1)[bad[0]]!r}")


def check(dev, shape, dim: int, dt: str, op: str, seed: int = 0, offset: int = 0, both=(False, True)) -> None:
    """scan(dim=) of fresh data against the oracle, inclusive and exclusive.
    ``offset``: the operand starts that many elements into its buffer."""
    axis = dim % len(shape)
    x = make(shape, axis, dt, op, seed)
    inc = oracle(x, axis, op)
    if offset:
        base = torch.zeros(x.size + offset, dtype=TORCH[dt], device=dev)
        xt = base[offset:].view(shape)
        xt.copy_(to_torch(x, dev))
        assert xt.is_contiguous() and xt.data_ptr() == base.data_ptr() + offset * x.itemsize
    else:
        xt = to_torch(x, dev)
    for e in both:
        got = scan(xt, exclusive=e, op=op, dim=dim)
        assert got.shape == xt.shape and got.is_contiguous()
        assert_same(got, excl_of(inc, axis, op) if e else inc, op, (shape, dim, dt, op, e, offset))


# --------------------------------------------------------------- row form
def row_ns(tile: int) -> list:
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 3]


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_workgroup_per_line(dev, dt, op):
    """Every n around the structural sizes, odd n (rows start off 16-byte
    alignment) included, for 1 (the 1-D path), 2, 3, 5 and 67 rows."""
    tile = edges(dev, dt)["tile"]
    for outer in (1, 2, 3, 5, 67):
        for n in row_ns(tile):
            if op != "sum" and outer in (2, 5) and n not in (65, tile + 1):
                continue  # max / min: every n for three row counts
            check(dev, (outer, n), -1, dt, op)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_wave_per_line(dev, dt, op):
    """Many short rows: a wave per row on the GPU."""
    e = edges(dev, dt)
    rows, tile = e["wave_rows"], e["wave_tile"]
    if dev.type == "cuda":
        assert scan_dim_launch_info((rows + 3, 2 * tile + 3), -1, dtype=TORCH[dt], device=dev)["waves"] == 1
    for n in (1, 3, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3):
        check(dev, (rows + 3, n), -1, dt, op, both=(n % 2 == 0,))
    check(dev, (rows + 3, 65), -1, dt, op)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_grid_stride(dev, dt):
    """Two workgroups for all the rows: each goes round its row loop many
    times, in both row kernels."""
    e = edges(dev, dt)
    with knobs(dev, scan_dim_maxblocks=2):
        if dev.type == "cuda":
            assert scan_dim_launch_info((67, 257), -1, dtype=TORCH[dt], device=dev)["workgroups"] == 2
        for op in OPS:
            check(dev, (67, 257), -1, dt, op)
            check(dev, (67, e["tile"] + 1), -1, dt, op, both=(False,))
            check(dev, (e["wave_rows"] + 3, 65), -1, dt, op, both=(True,))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [2, 3, 7])
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_chunked(dev, dt, chunks):
    """Reduce-then-scan along the rows: n not divisible by K, n < K (empty
    chunks), chunks of several tiles."""
    tile = edges(dev, dt)["tile"]
    with knobs(dev, scan_dim_chunks=chunks):
        if dev.type == "cuda":
            info = scan_dim_launch_info((3, 100), -1, dtype=TORCH[dt], device=dev)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * np.dtype(NP[dt]).itemsize
        for n in (2, 5, 100, tile + 1, 3 * tile + 5, 7 * tile + 1):
            for op in OPS:
                check(dev, (3, n), -1, dt, op)


# ------------------------------------------------------------ column form
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form(dev, dt, op):
    """Every inner around the vector width, the wave and the workgroup, every
    n around the unroll depth; inner divisible by the lane vector takes the
    vector path, the others the scalar one."""
    e = edges(dev, dt)
    w, u = e["width"], e["unroll"]
    for outer in (1, 3):
        for inner in (2, 3, 4, 5, 63, 64, 65, 255, 257, w - 1, w, w + 1):
            for n in (1, 2, 7, u - 1, u, u + 1, 129):
                if op != "sum" and n not in (1, u + 1, 129):
                    continue
                check(dev, (outer, n, inner), 1, dt, op, both=(False, True) if n in (1, u + 1) else ((outer == 1),))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_forced_scalar(dev, dt):
    """inner divisible by the lane vector, but the operand starts one element
    off 16-byte alignment: the scalar mapping."""
    if dev.type == "cuda":
        info = scan_dim_launch_info((3, 9, 64), 1, dtype=TORCH[dt], device=dev)
        assert info["vector"] > 1  # what an aligned operand of this shape takes
    for op in OPS:
        for shape in ((3, 9, 64), (1, 129, 4), (2, 10, 256)):
            check(dev, shape, 1, dt, op, offset=1)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [2, 3, 7])
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_chunked(dev, dt, chunks):
    with knobs(dev, scan_dim_chunks=chunks):
        if dev.type == "cuda":
            info = scan_dim_launch_info((3, 100, 64), 1, dtype=TORCH[dt], device=dev)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * 64 * np.dtype(NP[dt]).itemsize
        for outer in (1, 3):
            for inner in (3, 64, 65):
                for n in (2, 5, 100, 129):
                    for op in OPS:
                        check(dev, (outer, n, inner), 1, dt, op, both=(n != 100,))
        check(dev, (2, 100, 64), 1, dt, "sum", offset=1)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_grid_stride(dev, dt):
    with knobs(dev, scan_dim_maxblocks=2):
        for op in OPS:
            check(dev, (3, 17, 1025), 1, dt, op)
            check(dev, (3, 17, 1024), 1, dt, op, both=(True,))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_middle_dimensions(dev, dt):
    """A 3-D and a 4-D tensor along a middle dimension, every dim of the 4-D
    one by its negative index as well."""
    for op in OPS:
        check(dev, (5, 37, 9), 1, dt, op)
        check(dev, (2, 3, 19, 8), 2, dt, op)
        check(dev, (2, 3, 19, 8), 1, dt, op)
        for d in (-4, -3, -2, -1):
            check(dev, (2, 3, 19, 8), d, dt, op, both=(False,))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", ALL)
def test_every_dtype_in_every_regime(dev, dt, op):
    tile = edges(dev, dt)["tile"]
    e = edges(dev, dt)
    check(dev, (5, 301), -1, dt, op)  # row, single pass
    check(dev, (e["wave_rows"] + 1, 67), -1, dt, op)  # row, a wave per line
    check(dev, (3, 50, 64), 1, dt, op)  # column, lane vectors
    check(dev, (3, 50, 65), 1, dt, op)  # column, scalar lanes
    with knobs(dev, scan_dim_chunks=3):
        check(dev, (3, 2 * tile + 3), -1, dt, op)  # row, chunked
        check(dev, (3, 129, 64), 1, dt, op)  # column, chunked
        check(dev, (3, 129, 65), 1, dt, op)


# ---------------------------------------------------------- rounding tier
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_float_sums_round_within_the_bound(dev, dt, chunks):
    u = 2.0 ** -24 if dt == "f32" else 2.0 ** -53
    rng = np.random.default_rng(5)
    for shape, dim in (((5, 1024), 1), ((3, 1021), 1), ((1024, 67), 0), ((2, 1000, 4), 1)):
        v = rng.uniform(1.0, 2.0, shape).astype(NP[dt])
        wide = v.astype(np.longdouble)
        ref = np.cumsum(wide, axis=dim)
        m = np.arange(1, shape[dim] + 1).reshape([-1 if a == dim else 1 for a in range(len(shape))])
        bound = (1.01 * u * m * np.cumsum(np.abs(wide), axis=dim)).astype(np.float64)
        # on the oracle alone: a whole element (hence a whole chunk) does not fit under the bound
        assert shape[dim] <= 1024 and bound.max() <= 0.127 and v.min() >= 1.0
        with knobs(dev, scan_dim_chunks=chunks):
            got = to_numpy(scan(to_torch(v, dev), dim=dim)).astype(np.longdouble)
            exc = to_numpy(scan(to_torch(v, dev), dim=dim, exclusive=True)).astype(np.longdouble)
        err = np.abs(got - ref).astype(np.float64)
        assert np.all(err <= bound), (shape, dim, float((err - bound).max()))
        err = np.abs(exc - (ref - wide)).astype(np.float64)
        assert np.all(err <= bound), (shape, dim, "exclusive", float((err - bound).max()))


# ------------------------------------------------------ isolation and edges
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("dt", ALL)
def test_a_poisoned_line_stays_alone(dev, dt, chunks):
    """A NaN (integers: a huge value) planted in one line shows in that line
    from its position on and in no other line; sum and max, both forms."""
    tile = edges(dev, dt)["tile"]
    floating = dt[0] == "f"
    poison = np.nan if floating else (2 ** 31 - 5 if dt != "i64" else 2 ** 62 + 12345)
    for shape, dim, at in (((5, tile + 77), 1, (2, 40)), ((3, 40, 65), 1, (1, 7, 33)), ((3, 40, 64), 1, (2, 0, 63)),
                           ((40, 8), 0, (5, 3))):
        for op in ("sum", "max"):
            axis = dim
            x = make(shape, axis, dt, op, seed=3)
            if not floating and op == "sum":
                x = (x.astype(np.int64) % 1000).astype(NP[dt])  # small values: the huge one stands out
            clean = oracle(x, axis, op)
            y = x.copy()
            y[at] = poison
            with knobs(dev, scan_dim_chunks=chunks):
                got = to_numpy(scan(to_torch(y, dev), op=op, dim=dim))
            line = tuple(slice(None) if a == axis else at[a] for a in range(len(shape)))
            mask = np.ones(shape, dtype=bool)
            mask[line] = False
            assert_same(got[mask], clean[mask], op, (shape, dt, op, "other lines"))
            before, after = got[line][:at[axis]], got[line][at[axis]:]
            assert_same(before, clean[line][:at[axis]], op, (shape, dt, op, "before the poison"))
            if floating:
                assert np.isnan(after).all()
            elif op == "max":
                assert (after == poison).all()
            else:
                diff = (after.astype(np.int64) - clean[line][at[axis]:].astype(np.int64))
                want = int(poison) - int(x[at])
                # 32-bit sums wrap; the int64 line stays far below 2^63
                assert ((diff - want) % 2 ** 32 == 0).all() if x.itemsize == 4 else (diff == want).all()


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
def test_out_view_leaves_its_guards_alone(dev, chunks):
    """out as a view inside a sentinel-filled buffer, ragged n and inner: the
    elements before and after it keep the sentinel."""
    for dt in MAIN:
        for shape, dim in (((5, 301), 1), ((3, 37, 13), 1), ((2, 45, 16), 1), ((67, 3), 0)):
            x = make(shape, dim, dt, "sum")
            size, lead, sentinel = int(np.prod(shape)), 37, 77
            buf = torch.full((lead + size + 64,), sentinel, dtype=TORCH[dt], device=dev)
            out = buf[lead:lead + size].view(shape)
            with knobs(dev, scan_dim_chunks=chunks):
                got = scan(to_torch(x, dev), dim=dim, out=out)
            assert got is out
            assert_same(out, oracle(x, dim, "sum"), "sum", (shape, dt))
            assert (buf[:lead] == sentinel).all() and (buf[lead + size:] == sentinel).all()


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
def test_in_place(dev, chunks):
    for dt in MAIN:
        tile = edges(dev, dt)["tile"]
        for shape, dim in (((3, 2 * tile + 3), 1), ((3, 129, 64), 1), ((3, 129, 5), 1)):
            for op, e in (("sum", False), ("sum", True), ("max", False)):
                x = make(shape, dim, dt, op)
                inc = oracle(x, dim, op)
                xt = to_torch(x, dev)
                with knobs(dev, scan_dim_chunks=chunks):
                    assert scan(xt, exclusive=e, op=op, dim=dim, out=xt) is xt
                assert_same(xt, excl_of(inc, dim, op) if e else inc, op, (shape, dt, op, e))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", ALL)
def test_operands_aligned_to_the_element_only(dev, dt):
    for off in (1, 3):
        check(dev, (5, 301), 1, dt, "sum", offset=off)
        check(dev, (3, 50, 64), 1, dt, "max", offset=off)
        check(dev, (3, 21, 5), 1, dt, "sum", offset=off)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_empty_shapes_and_rejected_arguments(dev):
    for shape, dim in (((3, 0), 1), ((0, 4), 1), ((0, 4), 0), ((2, 3, 0), 1), ((2, 0, 3), 1), ((0,), 0)):
        for op in OPS:
            got = scan(torch.zeros(shape, device=dev), op=op, dim=dim, exclusive=True)
            assert got.shape == torch.Size(shape) and got.dtype == torch.float32
    x = torch.arange(12, dtype=torch.float32, device=dev).view(3, 4)
    assert torch.equal(scan(x, dim=-1), scan(x, dim=1)) and torch.equal(scan(x, dim=-2), scan(x, dim=0))
    assert torch.equal(scan(x, dim=0).cpu(), torch.cumsum(x.cpu(), 0))
    assert torch.equal(scan(x.t(), dim=0).cpu(), torch.cumsum(x.cpu().t(), 0))  # a non-contiguous x is copied
    for d in (2, -3):
        with pytest.raises(IndexError):
            scan(x, dim=d)
    with pytest.raises(ValueError):
        scan(torch.tensor(1.0, device=dev), dim=0)
    with pytest.raises(TypeError, match="auto"):
        scan(x, dim=0, algo="lookback")
    with pytest.raises(ValueError, match="out"):
        scan(x, dim=0, out=torch.empty(4, 3, device=dev))
    with pytest.raises(ValueError, match="out"):
        scan(x, dim=0, out=torch.empty(3, 4, dtype=torch.float64, device=dev))
    with pytest.raises(TypeError):
        scan(x.half(), dim=0)
    with pytest.raises(ValueError, match="op"):
        scan(x, dim=0, op="prod")
    # n == 1: a copy, or the identity
    y = torch.arange(6, dtype=torch.int64, device=dev).view(2, 1, 3) - 2
    assert torch.equal(scan(y, dim=1), y) and torch.equal(cummin(y, dim=1), y)
    assert (scan(y, dim=1, exclusive=True) == 0).all()
    assert (cummax(y, dim=1, exclusive=True) == -2 ** 63).all() and (cummin(y, dim=1, exclusive=True) == 2 ** 63 - 1).all()
    assert torch.equal(cummax(y, dim=2).cpu(), torch.cummax(y.cpu(), 2).values)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_one_line_is_the_1d_scan_and_the_default_stays_flat(dev):
    """outer == inner == 1 with dim= is the 1-D scan bit for bit and takes its
    algo; scan(x) of a 2-D tensor without dim is still the flattened scan."""
    rng = np.random.default_rng(9)
    v = rng.uniform(-1, 1, 40_000).astype(np.float32)
    x = to_torch(v, dev)
    algos = ("auto", "lookback", "rts") if dev.type == "cuda" else ("auto",)
    for algo in algos:
        for shape, dim in (((40_000,), 0), ((1, 40_000, 1), 1), ((1, 1, 40_000), -1)):
            got = scan(x.view(shape), dim=dim, algo=algo)
            assert got.shape == torch.Size(shape)
            assert np.array_equal(raw(to_numpy(got).reshape(-1)), raw(to_numpy(scan(x, algo=algo))))
    assert np.array_equal(raw(to_numpy(cummax(x.view(1, -1), dim=1)).reshape(-1)), raw(to_numpy(cummax(x))))
    if dev.type == "cuda":  # the CPU backend has one algorithm and does not read algo
        with pytest.raises((ValueError, TypeError)):
            scan(x.view(1, -1), dim=1, algo="no such algo")
    a = make((7, 300), 1, "i64", "sum")
    flat = to_numpy(scan(to_torch(a, dev)))
    assert flat.shape == (7, 300)
    assert np.array_equal(flat.reshape(-1), np.cumsum(a.reshape(-1), dtype=np.int64))
    assert not np.array_equal(flat, np.cumsum(a, axis=1, dtype=np.int64))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", ALL)
def test_summed_area_table(dev, dt):
    """Every box sum from four corner look-ups equals the direct sum, and the
    table is numpy's cumsum over both axes."""
    rng = np.random.default_rng(11)
    h, w = 37, 53
    img = rng.integers(0, 16, (2, h, w)).astype(NP[dt])
    sat = to_numpy(summed_area_table(to_torch(img, dev)))
    want = np.cumsum(np.cumsum(img.astype(np.int64), axis=-1), axis=-2)
    assert sat.dtype == img.dtype and np.array_equal(sat.astype(np.int64), want)
    s = np.zeros((2, h + 1, w + 1), dtype=np.int64)
    s[:, 1:, 1:] = sat
    direct = np.zeros_like(s)
    direct[:, 1:, 1:] = want
    i0, i1 = np.triu_indices(h + 1, 1)
    for j0 in range(0, w, 5):
        for j1 in range(j0 + 1, w + 1, 7):
            box = s[:, i1, j1] - s[:, i0, j1] - s[:, i1, j0] + s[:, i0, j0]
            ref = np.stack([img[:, a:b, j0:j1].astype(np.int64).sum(axis=(1, 2)) for a, b in zip(i0[::41], i1[::41])], 1)
            assert np.array_equal(box[:, ::41], ref)
    out = torch.empty_like(to_torch(img, dev))
    assert summed_area_table(to_torch(img, dev), out=out) is out and np.array_equal(to_numpy(out), sat)
    with pytest.raises(ValueError):
        summed_area_table(torch.zeros(5, device=dev))


# ------------------------------------------------------------------ GPU only
@pytest.mark.gpu
def test_launch_info_names_the_regimes(gpu):
    keys = {"form", "outer", "n", "inner", "chunks", "tile", "vector", "workgroups", "ws_bytes"}
    flat = scan_dim_launch_info((1, 1000, 1), 1, device=gpu)
    assert keys <= set(flat) and flat["form"] == "flat"
    row = scan_dim_launch_info((65536, 2048), -1, device=gpu)
    assert (row["form"], row["outer"], row["n"], row["inner"], row["chunks"], row["ws_bytes"]) == ("row", 65536, 2048, 1, 1, 0)
    long_rows = scan_dim_launch_info((16, 1 << 22), -1, device=gpu)
    assert long_rows["chunks"] > 1 and long_rows["ws_bytes"] == 16 * long_rows["chunks"] * 4
    assert long_rows["chunks"] * long_rows["chunk"] >= 1 << 22 and long_rows["chunk"] % long_rows["tile"] == 0
    wide = scan_dim_launch_info((64, 1 << 21), 0, device=gpu)
    assert (wide["form"], wide["chunks"]) == ("col", 1)  # enough columns for a single pass
    thin = scan_dim_launch_info((1 << 21, 64), 0, dtype=torch.int64, device=gpu)
    assert thin["form"] == "col" and thin["chunks"] > 1 and thin["vector"] == 2
    assert thin["ws_bytes"] == thin["chunks"] * 64 * 8
    narrow = scan_dim_launch_info((1 << 22, 3), 0, device=gpu)
    assert narrow["vector"] == 1 and narrow["chunks"] > 1
    assert scan_dim_launch_info((4, 0, 3), 1, device=gpu)["workgroups"] == 0
    with pytest.raises(IndexError):
        scan_dim_launch_info((4, 3), 2, device=gpu)


@pytest.mark.gpu
def test_chunked_float_sums_repeat_bit_for_bit_and_workspaces_do_not_mix(gpu):
    """Two identical float32 launches of a chunked shape give identical bits;
    fifty alternating row / column / 1-D look-back launches on one stream stay
    correct (the chunk totals and the look-back descriptors are apart)."""
    from cme213x.ops.scan import check_lookback
    from cme213x.utils import tuning

    rng = np.random.default_rng(21)
    v = rng.uniform(-1, 1, (3, 20_011)).astype(np.float32)
    c = rng.uniform(-1, 1, (3, 1001, 64)).astype(np.float32)
    with tuning.override(scan_dim_chunks=7):
        for a, dim in ((to_torch(v, gpu), 1), (to_torch(c, gpu), 1)):
            first, second = scan(a, dim=dim), scan(a, dim=dim)
            assert np.array_equal(raw(to_numpy(first)), raw(to_numpy(second)))
        ri, ci, li = (make(s, 1, "i64", "sum", seed=k) for k, s in enumerate(((3, 9001), (3, 301, 33), (1, 70_001))))
        want = [np.cumsum(a, axis=1, dtype=np.int64) for a in (ri, ci, li)]
        dev = [to_torch(a, gpu) for a in (ri, ci, li)]
        outs = []
        for k in range(50):
            j = k % 3
            outs.append((j, scan(dev[j], dim=1) if j < 2 else scan(dev[j].view(-1), algo="lookback")))
        check_lookback(gpu)
        for j, o in outs:
            assert np.array_equal(to_numpy(o).reshape(want[j].shape), want[j])


@pytest.mark.gpu
def test_graph_capture_of_a_chunked_column_scan(gpu):
    """One capture, replayed on changed inputs; the chunk totals were sized by
    the warm-up launch outside the capture."""
    from cme213x.utils import tuning

    shape = (3, 301, 64)
    x = torch.zeros(shape, dtype=torch.int64, device=gpu)
    out = torch.empty_like(x)
    with tuning.override(scan_dim_chunks=5):
        scan(x, dim=1, out=out)
        torch.cuda.synchronize(gpu)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            scan(x, dim=1, out=out)
    for seed in (1, 2):
        a = make(shape, 1, "i64", "sum", seed=seed)
        x.copy_(to_torch(a, gpu))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert np.array_equal(to_numpy(out), np.cumsum(a, axis=1, dtype=np.int64))
