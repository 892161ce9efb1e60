"""Sort along one dimension (``sort(x, dim=d, descending=)`` -> ``(values,
indices)``, ``argsort(x, dim=d)``) on the HIP and the CPU backend.

Oracle, never the code under test: ``numpy.argsort(codes, axis, kind="stable")``
over order codes computed here from the integer view of the data (unsigned as
is, signed with the sign bit flipped, floats in IEEE total order; complemented
for descending order), and ``numpy.take_along_axis`` for the values.
``indices`` are compared exactly, ``values`` on their bits. On data without NaN
and ``-0.0`` the oracle is additionally asserted equal to ``torch.sort(x_cpu,
dim, stable=True, descending=)``.

Data, cycled over the lines: draws from four distinct keys (heavy ties:
stability), full-range random bit patterns (for floats: NaNs of both signs with
varied payloads, zeros of both signs, infinities), all keys equal, already
sorted, reversed, and lines salted with the key whose code is all-ones in the
direction under test -- the code the kernel's padding carries.

The GPU shapes are the smallest at which each mechanism can go wrong; their
edges come from ``sort_dim_launch_info``: ``T`` is the tile (the longest line
of the tile regime), ``Lm(n)`` the lines a tile holds. Row form: one line per
tile, full and partial; two lines with slack at the tile's end; many short
lines with a last tile that holds fewer, and a single partial tile. Column
form: fewer columns than a tile takes, more (a partial last tile per slice),
and one more or less than ``Lm``. Above ``T``, and under the knob
``sort_dim_max_n``, the result is composed from the 1-D sorts; the knob
``sort_dim_lanes=0`` selects the ballot-match ranks. The CPU backend has one
path; it runs the same shapes with fixed stand-ins for ``T`` and ``Lm``.
Nothing above 2^20 elements is tested."""
import contextlib

import numpy as np
import pytest
import torch

from cme213x.ops.sort import SortWithIndices, argsort, sort, sort_dim_launch_info

NP = {"u32": np.uint32, "i32": np.int32, "f32": np.float32, "u64": np.uint64, "i64": np.int64, "f64": np.float64}
TORCH = {"u32": torch.uint32, "i32": torch.int32, "f32": torch.float32, "u64": torch.uint64, "i64": torch.int64,
         "f64": torch.float64}
ALL = list(NP)
MAIN = ["f32", "i64"]
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
DESC = [pytest.param(False, id="asc"), pytest.param(True, id="desc")]
CPU_T = 8192  # stand-ins of the CPU backend, which has no tile
CPU_LMAX = 256


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def knobs(dev, **kw):
    """The knobs of the HIP backend (the CPU backend has none)."""
    if dev.type != "cuda" or not kw:
        return contextlib.nullcontext()
    from cme213x.utils import tuning

    return tuning.override(**kw)


# ------------------------------------------------------------------ edges
def tile_of(dev, dt: str) -> int:
    if dev.type != "cuda":
        return CPU_T
    info = sort_dim_launch_info((3, 64), -1, dtype=TORCH[dt], device=dev)
    assert info["regime"] == "tile" and info["tile"] >= 1024
    return info["tile"]


def lines_per_tile(dev, dt: str, n: int) -> int:
    """Lm: the lines of a full tile at line length ``n`` (asked for a shape
    with more lines than any tile holds)."""
    if dev.type != "cuda":
        return max(1, min(CPU_T // n, CPU_LMAX))
    info = sort_dim_launch_info((1 << 16, n), -1, dtype=TORCH[dt], device=dev)
    assert info["regime"] == "tile" and info["lines_per_tile"] >= 1
    return info["lines_per_tile"]


# ------------------------------------------------------------------ oracle
def unsigned(dtype):
    return np.uint32 if np.dtype(dtype).itemsize == 4 else np.uint64


def bits(a: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(a).view(unsigned(a.dtype))


def codes(a: np.ndarray, descending: bool) -> np.ndarray:
    u = bits(a)
    sign = u.dtype.type(1) << u.dtype.type(8 * u.itemsize - 1)
    if a.dtype.kind == "i":
        c = u ^ sign
    elif a.dtype.kind == "f":
        c = np.where((u & sign) != 0, ~u, u ^ sign)
    else:
        c = u
    return ~c if descending else c


def oracle(a: np.ndarray, axis: int, descending: bool):
    idx = np.argsort(codes(a, descending), axis=axis, kind="stable").astype(np.int64)
    return np.take_along_axis(a, idx, axis), idx


# -------------------------------------------------------------------- data
def all_ones_key(dtype, descending: bool):
    """The bits of the key whose order code is all ones."""
    u = unsigned(dtype)
    sign = u(1) << u(8 * np.dtype(u).itemsize - 1)
    kind = np.dtype(dtype).kind
    if kind == "u":
        return u(0) if descending else ~u(0)
    if kind == "i":
        return sign if descending else ~sign  # the minimum / the maximum
    return ~u(0) if descending else ~sign     # -NaN / +NaN with every payload bit


def finite(rng, dtype, size):
    """Values without NaN, infinities and zeros."""
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        v = rng.standard_normal(size) * 10.0 ** rng.integers(-3, 4, size)
        return np.where(v == 0, 1.0, v).astype(dtype)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size, dtype=dtype, endpoint=True)


def make(shape, axis: int, dt: str, descending: bool, clean: bool = False, seed: int = 0) -> np.ndarray:
    """Data of ``shape`` whose lines along ``axis`` cycle through the kinds of
    the module docstring. ``clean``: no NaN, no ``-0.0`` (torch.sort agrees)."""
    dtype = np.dtype(NP[dt])
    u = unsigned(dtype)
    rng = np.random.default_rng(seed + 31 * len(shape) + sum(shape) + 7 * axis)
    n = shape[axis]
    lines = int(np.prod(shape, dtype=np.int64)) // max(n, 1)
    out = np.empty((lines, n), dtype=u)
    four = bits(finite(rng, dtype, 4))
    for i in range(lines):
        kind = i % 6
        if kind == 0:
            row = four[rng.integers(0, 4, n)]
        elif kind == 1:
            if clean:
                row = bits(finite(rng, dtype, n))
            else:
                row = rng.integers(0, np.iinfo(u).max, n, dtype=u, endpoint=True)
                if dtype.kind == "f":  # specials among the random patterns
                    sp = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan], dtype=dtype)
                    hit = rng.random(n) < 0.2
                    row[hit] = bits(sp)[rng.integers(0, 6, int(hit.sum()))]
        elif kind == 2:
            row = np.full(n, four[0], dtype=u)
        elif kind in (3, 4):
            v = finite(rng, dtype, n)
            v = np.sort(v)
            row = bits(v if kind == 3 else v[::-1].copy())
        else:
            row = bits(finite(rng, dtype, n)).copy()
            salt = bits(np.array([np.finfo(dtype).max], dtype=dtype))[0] if clean and dtype.kind == "f" else \
                all_ones_key(dtype, descending)
            row[rng.random(n) < 0.3] = salt
            row[-1] = salt
        out[i] = row
    outer = int(np.prod(shape[:axis], dtype=np.int64))
    inner = int(np.prod(shape[axis + 1:], dtype=np.int64))
    a = np.ascontiguousarray(out.reshape(outer, inner, n).transpose(0, 2, 1)).reshape(shape)
    return a.view(dtype)


# -------------------------------------------------------------- conversion
def to_torch(a: np.ndarray, dev) -> torch.Tensor:
    if a.dtype.kind == "u":
        signed = np.int32 if a.itemsize == 4 else np.int64
        return torch.from_numpy(np.ascontiguousarray(a).view(signed)).to(dev).view(TORCH["u%d" % (8 * a.itemsize)])
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def to_numpy(t: torch.Tensor) -> np.ndarray:
    if t.dtype in (torch.uint32, torch.uint64):
        signed = torch.int32 if t.dtype == torch.uint32 else torch.int64
        return t.contiguous().view(signed).cpu().numpy().view(np.uint32 if t.dtype == torch.uint32 else np.uint64)
    return t.cpu().numpy()


def check(res, a: np.ndarray, axis: int, descending: bool, what: str = "") -> None:
    """``res`` against the oracle of ``a``: indices exactly, values bit for bit."""
    want_v, want_i = oracle(a, axis, descending)
    assert isinstance(res, SortWithIndices)
    v, i = res.values, res.indices
    assert v.dtype == TORCH[_name(a.dtype)] and i.dtype == torch.int64, what
    assert tuple(v.shape) == a.shape and tuple(i.shape) == a.shape, what
    assert v.is_contiguous() and i.is_contiguous(), what
    gi, gv = i.cpu().numpy(), to_numpy(v)
    bad = np.flatnonzero(gi.reshape(-1) != want_i.reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} indices differ, first at flat {bad[0]}: " \
                          f"{gi.reshape(-1)[bad[0]]} != {want_i.reshape(-1)[bad[0]]}"
    bad = np.flatnonzero(bits(gv).reshape(-1) != bits(want_v).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first at flat {bad[0]}"


def _name(dtype) -> str:
    return next(k for k, v in NP.items() if np.dtype(v) == np.dtype(dtype))


def run(dev, shape, dim: int, dt: str, descending: bool, **kw) -> None:
    axis = dim % len(shape)
    a = make(shape, axis, dt, descending)
    with knobs(dev, **kw):
        res = sort(to_torch(a, dev), dim=dim, descending=descending)
    check(res, a, axis, descending, f"{dt} {shape} dim {dim} descending {descending} {kw}")


# --------------------------------------------------------------- row form
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", MAIN)
def test_row_long_lines(dev, dt, descending):
    """One line per tile, full and one short; two lines; slack at the tile's end."""
    T = tile_of(dev, dt)
    for n in (T, T - 1, T // 2, T // 2 + 1, T // 3):
        run(dev, (3, n), -1, dt, descending)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", MAIN)
def test_row_short_lines(dev, dt, descending):
    """Many lines per tile: a last tile that holds fewer lines, and a single
    partial tile."""
    for n in (2, 3, 63, 64, 65, 100):
        lm = lines_per_tile(dev, dt, n)
        assert lm > 2
        run(dev, (2 * lm + 1, n), -1, dt, descending)
        run(dev, (lm - 1, n), -1, dt, descending)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_trivial_shapes(dev, dt):
    for shape, dim in (((7, 1), -1), ((1, 5), 0), ((0, 5), -1), ((0, 5), 0), ((5, 0), -1), ((5, 0), 0), ((9,), 0)):
        run(dev, shape, dim, dt, False)
        run(dev, shape, dim, dt, True)


# ------------------------------------------------------------ column form
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form(dev, dt, descending):
    T = tile_of(dev, dt)
    for n in (37, T // 2 - 3):
        lm = lines_per_tile(dev, dt, n)
        for inner in sorted({2, 5, 64, lm - 1, lm + 1}):  # lm - 1 == 1 is the row form
            run(dev, (3, n, inner), 1, dt, descending)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_middle_dim_of_rank4(dev, dt):
    shape = (2, 3, 50, 7)
    a = make(shape, 2, dt, False)
    x = to_torch(a, dev)
    pos, neg = sort(x, dim=2), sort(x, dim=-2)
    check(pos, a, 2, False, "dim 2")
    check(neg, a, 2, False, "dim -2")
    run(dev, shape, 1, dt, True)
    run(dev, shape, 0, dt, True)


# ----------------------------------------------------------------- layout
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
def test_non_contiguous_input(dev, descending):
    a = make((40, 67), 1, "f32", descending)
    x = to_torch(a, dev).t()  # (67, 40), strides (1, 67)
    assert not x.is_contiguous()
    check(sort(x, dim=0, descending=descending), a.T, 0, descending, "transposed, dim 0")
    check(sort(x, dim=1, descending=descending), a.T, 1, descending, "transposed, dim 1")


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", ["f32", "i64", "u32", "f64"])
def test_element_aligned_views(dev, dt):
    """``base[1:]``: storage aligned to the element only."""
    for shape, dim in (((5, 333), -1), ((3, 41, 6), 1)):
        axis = dim % len(shape)
        a = make(shape, axis, dt, False)
        base = torch.zeros(a.size + 1, dtype=TORCH[dt], device=dev)
        v = base[1:]
        v.copy_(to_torch(a.reshape(-1), dev))
        x = v.view(shape)
        assert x.is_contiguous() and x.data_ptr() == base.data_ptr() + a.itemsize
        check(sort(x, dim=dim), a, axis, False, f"{dt} {shape} view")


# --------------------------------------------------------- composed regime
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", MAIN)
def test_lines_above_the_tile(dev, dt, descending):
    T = tile_of(dev, dt)
    if dev.type == "cuda":
        assert sort_dim_launch_info((3, T + 1), -1, dtype=TORCH[dt], device=dev)["regime"] == "composed"
        assert sort_dim_launch_info((3, T), -1, dtype=TORCH[dt], device=dev)["regime"] == "tile"
    run(dev, (3, T + 1), -1, dt, descending)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", ALL)
def test_composed_under_knob(dev, dt, descending):
    if dev.type == "cuda":
        with knobs(dev, sort_dim_max_n=64):
            assert sort_dim_launch_info((5, 100), -1, dtype=TORCH[dt], device=dev)["regime"] == "composed"
            assert sort_dim_launch_info((5, 64), -1, dtype=TORCH[dt], device=dev)["regime"] == "tile"
    run(dev, (5, 100), -1, dt, descending, sort_dim_max_n=64)
    run(dev, (2, 100, 3), 1, dt, descending, sort_dim_max_n=64)
    run(dev, (1, 100, 1), 1, dt, descending, sort_dim_max_n=64)  # a single line


# ---------------------------------------------------------- fallback ranks
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", MAIN)
def test_ballot_match_ranks(dev, dt, descending):
    run(dev, (40, 100), -1, dt, descending, sort_dim_lanes=0)
    run(dev, (3, 2049, 5), 1, dt, descending, sort_dim_lanes=0)
    run(dev, (3, 37, 70), 1, dt, descending, sort_dim_lanes=0)


# ---------------------------------------------------------------- coverage
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", ALL)
def test_every_dtype(dev, dt, descending):
    T = tile_of(dev, dt)
    lm = lines_per_tile(dev, dt, 100)
    for shape, dim in (((lm + 3, 100), -1), ((3, T // 2 + 1), -1), ((2, T), 1), ((3, 37, 5), 1), ((2, 300, 33), -2),
                       ((600, 2), 1)):
        run(dev, shape, dim, dt, descending)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", ["i32", "f32", "i64", "f64"])
def test_clean_data_matches_torch(dev, dt, descending):
    """Without NaN and ``-0.0`` the oracle, ``torch.sort(stable=True)`` and the
    sort agree."""
    for shape, dim in (((37, 100), -1), ((3, 41, 6), 1)):
        axis = dim % len(shape)
        a = make(shape, axis, dt, descending, clean=True)
        assert not (a.dtype.kind == "f" and (np.isnan(a).any() or (np.signbit(a) & (a == 0)).any()))
        want_v, want_i = oracle(a, axis, descending)
        tv, ti = torch.sort(torch.from_numpy(a), dim=dim, stable=True, descending=descending)
        assert np.array_equal(ti.numpy(), want_i) and np.array_equal(bits(tv.numpy()), bits(want_v))
        check(sort(to_torch(a, dev), dim=dim, descending=descending), a, axis, descending, f"clean {dt} {shape}")


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", DESC)
@pytest.mark.parametrize("dt", MAIN)
def test_argsort_and_gather(dev, dt, descending):
    for shape, dim in (((50, 129), -1), ((4, 77, 9), 1)):
        axis = dim % len(shape)
        a = make(shape, axis, dt, descending)
        x = to_torch(a, dev)
        res = sort(x, dim=dim, descending=descending)
        idx = argsort(x, dim=dim, descending=descending)
        assert idx.dtype == torch.int64 and torch.equal(idx, res.indices)
        signed = torch.int32 if a.itemsize == 4 else torch.int64
        gathered = torch.gather(x.view(signed), axis, res.indices)
        assert torch.equal(gathered, res.values.view(signed))
        assert np.array_equal(idx.cpu().numpy(), oracle(a, axis, descending)[1])


# ------------------------------------------------------------------ errors
@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_errors(dev):
    x = torch.zeros((4, 6), dtype=torch.float32, device=dev)
    with pytest.raises(ValueError):
        sort(torch.zeros((), dtype=torch.float32, device=dev), dim=0)
    with pytest.raises(ValueError):
        argsort(torch.zeros((), dtype=torch.float32, device=dev), dim=0)
    for d in (2, -3):
        with pytest.raises(IndexError):
            sort(x, dim=d)
        with pytest.raises(IndexError):
            argsort(x, dim=d)
    for bad in (torch.float16, torch.int16, torch.bool):
        with pytest.raises(TypeError):
            sort(torch.zeros((4, 6), dtype=bad, device=dev), dim=1)
        with pytest.raises(TypeError):
            argsort(torch.zeros((4, 6), dtype=bad, device=dev), dim=1)
    pos = torch.zeros((4, 6), dtype=torch.int32, device=dev)
    for kw in ({"values": pos}, {"algo": "merge"}, {"num_bits": 4}, {"key_bits": 8}):
        with pytest.raises(TypeError, match="indices replace"):
            sort(x, dim=1, **kw)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_without_dim_nothing_changes(dev):
    x = torch.arange(24, dtype=torch.float32, device=dev).flip(0)
    with pytest.raises(ValueError, match="1-D keys expected"):
        sort(x.view(4, 6))
    with pytest.raises(ValueError, match="1-D keys expected"):
        argsort(x.view(4, 6))
    out = sort(x)
    assert isinstance(out, torch.Tensor) and torch.equal(out, x.flip(0))
    k, v = sort(x, torch.arange(24, dtype=torch.int32, device=dev))
    assert torch.equal(k, x.flip(0)) and torch.equal(v, torch.arange(23, -1, -1, dtype=torch.int32, device=dev))
    # a 1-D tensor with dim= is the new function: a named pair
    res = sort(x, dim=0)
    assert isinstance(res, SortWithIndices) and torch.equal(res.values, out)
    assert torch.equal(res.indices, argsort(x))


# ------------------------------------------------------------- launch info
def test_launch_info_cpu():
    d = sort_dim_launch_info((3, 50, 7), 1, dtype=torch.int64, device="cpu")
    assert (d["form"], d["outer"], d["n"], d["inner"]) == ("col", 3, 50, 7)
    assert sort_dim_launch_info((50,), 0, device="cpu")["form"] == "flat"
    assert sort_dim_launch_info((4, 50), -1, device="cpu")["form"] == "row"
    with pytest.raises(IndexError):
        sort_dim_launch_info((4, 50), 2, device="cpu")
    with pytest.raises(TypeError):
        sort_dim_launch_info((4, 50), 1, dtype=torch.float16, device="cpu")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ALL)
def test_launch_info_gpu(gpu, dt):
    d = TORCH[dt]
    T = tile_of(gpu, dt)
    esize = np.dtype(NP[dt]).itemsize
    one = sort_dim_launch_info((5, T), -1, dtype=d, device=gpu)
    assert (one["form"], one["regime"], one["lines_per_tile"], one["workgroups"]) == ("row", "tile", 1, 5)
    assert one["passes"] == esize  # no line pass for one line per tile
    two = sort_dim_launch_info((5, T // 2), -1, dtype=d, device=gpu)
    assert (two["lines_per_tile"], two["workgroups"], two["passes"]) == (2, 3, esize + 1)
    lm = lines_per_tile(gpu, dt, 100)
    assert lm == min(T // 100, 256)
    many = sort_dim_launch_info((2 * lm + 1, 100), -1, dtype=d, device=gpu)
    assert (many["lines_per_tile"], many["workgroups"]) == (lm, 3)
    col = sort_dim_launch_info((3, 100, lm + 1), 1, dtype=d, device=gpu)
    assert (col["form"], col["lines_per_tile"], col["workgroups"]) == ("col", lm, 6)
    assert sort_dim_launch_info((1 << 16, 2), -1, dtype=d, device=gpu)["lines_per_tile"] == 256
    assert sort_dim_launch_info((0, 5), -1, dtype=d, device=gpu)["workgroups"] == 0
    big = sort_dim_launch_info((3, T + 1), -1, dtype=d, device=gpu)
    assert (big["regime"], big["workgroups"]) == ("composed", 0)
