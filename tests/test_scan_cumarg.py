"""``cummax`` / ``cummin`` with ``return_indices=True`` (and ``scan(...,
return_indices=True)``): the ``(values, indices)`` of ``torch.cummax`` /
``torch.cummin`` along any dimension and over the flattened tensor, on the HIP
and the CPU backend.

The rule under test: the carry is a pair (value, index); the later element
replaces it iff ``b >= a or b != b`` (max; mirrored for min). So NaN is sticky,
a later NaN and the later of two equal values take the index, and every output
has a real index.

Oracles, none of them the code under test:

* float32, int32, int64, float64: ``torch.cummax`` / ``torch.cummin`` on CPU
  tensors; values compared bit for bit, indices exactly;
* uint32 (torch has no kernel): ``numpy.maximum.accumulate`` for the values, a
  record is ``x >= values``, the index the running maximum of the record
  positions;
* ``test_the_rule_and_the_oracles``: a sequential Python loop of the rule on
  short lines with NaN, zeros of both signs and ties, against both oracles;
* the values are also compared bitwise with the call without indices.

Data along the scanned axis, a different seed per shape and different content
per line: an early spike (the index must stay at the spike to the end of the
line -- a lost carry INDEX shows, which the noisy ramp cannot show), a plateau
of values in {0, 1, 2, 3} (ties everywhere: the index moves while the value
stands still), monotone the wrong way (every index 0), the noisy ramp of
test_scan_dim.py, and special lines: NaN on either side of each structural
edge with a second NaN later, alternating ``+0.0`` / ``-0.0``, all ``-inf``,
all type-minimum, int64 beyond 2^53 and uint32 across 2^31.

The GPU shapes are the smallest at which each mechanism can go wrong; their
edges come from ``scan_dim_launch_info(..., indices=True)``, and the
``scan_dim_chunks`` / ``scan_dim_maxblocks`` knobs force the chunked regime
and the grid-stride loops. The CPU backend runs the same shapes with fixed
stand-ins for the edges. Tensors above 2^31 elements are not run: the 64-bit
index arithmetic is checked by reading the code.
"""
import contextlib

import numpy as np
import pytest
import torch

from cme213x.ops.scan import cummax, cummin, scan, scan_dim_launch_info
from scan_util import cached, to_numpy, to_torch

NP = {"f32": np.float32, "i32": np.int32, "u32": np.uint32, "i64": np.int64, "f64": np.float64}
TORCH = {"f32": torch.float32, "i32": torch.int32, "u32": torch.uint32, "i64": torch.int64, "f64": torch.float64}
ALL = list(NP)
MAIN = ["f32", "i64"]
OPS = ["max", "min"]
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
PATTERNS = ("plateau", "mono", "ramp")


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


def info_of(dev, shape, dim, dt):
    return scan_dim_launch_info(shape, dim, dtype=TORCH[dt], op="max", device=dev, indices=True)


# ------------------------------------------------------------------ edges
def edges(dev, dt: str) -> dict:
    """Structural sizes of the indexed launch, from the launch-info query on
    the GPU; fixed stand-ins of the same magnitude on the CPU."""
    if dev.type != "cuda":
        return {"tile": 1024, "wave_tile": 256, "wave_rows": 1024, "vector": 4, "width": 512, "unroll": 8}
    block = info_of(dev, (3, 1 << 20), -1, dt)
    assert block["form"] == "row" and block["waves"] == 4
    rows = next(o for o in (1 << k for k in range(4, 14)) if info_of(dev, (o, 65), -1, dt)["waves"] == 1)
    wave = info_of(dev, (rows, 65), -1, dt)
    col = info_of(dev, (3, 50, 64), 1, dt)
    assert col["form"] == "col" and col["vector"] == 16 // np.dtype(NP[dt]).itemsize
    return {"tile": block["tile"], "wave_tile": wave["tile"], "wave_rows": rows, "vector": col["vector"],
            "width": 256 * col["vector"], "unroll": col["tile"]}


# ------------------------------------------------------------------- data
def finish(v: np.ndarray, dt: str, op: str) -> np.ndarray:
    """Integer-valued data written for "max", mirrored for "min"."""
    if dt == "u32":
        v = v - min(int(v.min(initial=0)), 0) + 100
        return (v if op == "max" else 0xFFFFFFFF - v).astype(np.uint32)
    return (v if op == "max" else -v).astype(NP[dt])


def make(shape, axis: int, dt: str, op: str, pattern: str, seed: int = 0, p: int = 0) -> np.ndarray:
    rng = np.random.default_rng(seed + 17 * len(shape) + sum(shape))
    idx = np.arange(shape[axis], dtype=np.int64).reshape([-1 if a == axis else 1 for a in range(len(shape))])
    line = rng.integers(0, 1000, shape).take([0], axis)  # a different offset on every line
    if pattern == "plateau":
        return finish(rng.integers(0, 4, shape), dt, op)
    if pattern == "mono":  # strictly the wrong way: the first element wins to the end
        return finish(line - 3 * idx + np.zeros(shape, dtype=np.int64), dt, op)
    if pattern == "spike":  # small values and one dominating element at p
        v = rng.integers(-50, 51, shape)
        v[tuple(p if a == axis else slice(None) for a in range(len(shape)))] = 10_000 + line.squeeze(axis)
        return finish(v, dt, op)
    assert pattern == "ramp"
    v = 3 * idx + rng.integers(-50, 51, shape) + line
    if dt[0] != "f":
        return finish(v, dt, op)
    v = v + rng.uniform(-0.5, 0.5, shape)
    v[rng.random(shape) < 0.02] = 0.0
    v[rng.random(shape) < 0.02] = -0.0
    return (v if op == "max" else -v).astype(NP[dt])


def special_lines(x: np.ndarray, axis: int, op: str, at) -> np.ndarray:
    """A copy of ``x`` whose lines, in turn, become special. Floats: a NaN just
    before an edge and a second one later; a NaN on the edge and a second one
    later; alternating zeros of both signs; all -inf (max) / +inf (min).
    Integers: all type-minimum (max) / type-maximum (min); values that differ
    only in bits a float conversion would drop (int64 beyond 2^53, 32-bit
    across 2^31). ``at``: the edges, taken in turn."""
    n = x.shape[axis]
    lines = np.moveaxis(x.copy(), axis, -1)
    flat = lines.reshape(-1, n)
    at = [e for e in at if 0 < e < n] or [n // 2]
    rng = np.random.default_rng(n)
    for l in range(flat.shape[0]):
        kind, e = l % 4, at[(l // 4) % len(at)]
        later = min(n - 1, e + 1 + (n - e) // 2)
        if x.dtype.kind == "f":
            if kind == 0:
                flat[l, [e - 1, later]] = np.nan
            elif kind == 1:
                flat[l, [e, later]] = np.nan
            elif kind == 2:
                flat[l, 0::2], flat[l, 1::2] = 0.0, -0.0
            else:
                flat[l] = -np.inf if op == "max" else np.inf
        elif kind == 0:
            flat[l] = np.iinfo(x.dtype).min if op == "max" else np.iinfo(x.dtype).max
        elif kind == 1:
            big = {np.dtype(np.int64): 2 ** 53, np.dtype(np.int32): 2 ** 31 - 4, np.dtype(np.uint32): 2 ** 31 - 2}[x.dtype]
            v = big + rng.integers(0, 4, n)
            flat[l] = v if op == "max" or x.dtype == np.uint32 else -v
    return np.ascontiguousarray(np.moveaxis(flat.reshape(lines.shape), -1, axis))


# ----------------------------------------------------------------- oracles
def oracle(x: np.ndarray, axis: int, op: str):
    """(values, int64 indices) along ``axis``."""
    if x.dtype == np.uint32:
        acc = np.maximum if op == "max" else np.minimum
        vals = acc.accumulate(x, axis=axis)
        rec = x >= vals if op == "max" else x <= vals
        pos = np.arange(x.shape[axis], dtype=np.int64).reshape([-1 if a == axis else 1 for a in range(x.ndim)])
        return vals, np.maximum.accumulate(np.where(rec, pos, -1), axis=axis)
    f = torch.cummax if op == "max" else torch.cummin
    r = f(torch.from_numpy(x.copy()), axis)
    return r.values.numpy(), r.indices.numpy()


def by_the_rule(line, op: str):
    """The rule itself, one element after the other."""
    vals, idx = [], []
    av, ai = None, -1
    for i, b in enumerate(line):
        if ai < 0 or (b >= av if op == "max" else b <= av) or b != b:
            av, ai = b, i
        vals.append(av)
        idx.append(ai)
    return vals, idx


def raw(a: np.ndarray) -> np.ndarray:
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "f" else a


def assert_pair(values, indices, want, what) -> None:
    wv, wi = want
    v, i = to_numpy(values), to_numpy(indices)
    assert v.dtype == wv.dtype and v.shape == wv.shape and i.dtype == np.int64 and i.shape == wi.shape, what
    bad = np.flatnonzero(raw(v).reshape(-1) != raw(wv).reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} values differ, first at flat index {bad[0]}: "
                           f"{v.reshape(-1)[bad[0]]!r} != {wv.reshape(-1)[bad[0]]!r}")
    bad = np.flatnonzero(i.reshape(-1) != wi.reshape(-1))
    assert bad.size == 0, (f"{what}: {bad.size} indices differ, first at flat index {bad[0]}: "
                           f"{i.reshape(-1)[bad[0]]} != {wi.reshape(-1)[bad[0]]}")


def place(x: np.ndarray, dev, offset: int = 0) -> torch.Tensor:
    """``x`` on ``dev``, ``offset`` elements into its buffer."""
    if not offset:
        return to_torch(x, dev)
    base = torch.zeros(x.size + offset, dtype=TORCH[{v: k for k, v in NP.items()}[x.dtype.type]], device=dev)
    xt = base[offset:].view(x.shape)
    xt.copy_(to_torch(x, dev))
    assert xt.is_contiguous() and xt.data_ptr() == base.data_ptr() + offset * x.itemsize
    return xt


def run(dev, x: np.ndarray, dim, op: str, offset: int = 0, what=None):
    """The indexed scan of ``x`` against the oracle and against the values of
    the call without indices. ``dim=None``: the flattened tensor."""
    f = cummax if op == "max" else cummin
    xt = place(x, dev, offset)
    got = f(xt, dim=dim, return_indices=True)
    assert isinstance(got, tuple) and got._fields == ("values", "indices") and got.values is got[0]
    for t in got:
        assert t.shape == xt.shape and t.is_contiguous() and t.device == xt.device
    assert got.values.dtype == xt.dtype and got.indices.dtype == torch.int64
    what = what or (x.shape, dim, x.dtype.name, op, offset)
    if dim is None:
        wv, wi = oracle(x.reshape(-1), 0, op)
        want = wv.reshape(x.shape), wi.reshape(x.shape)
    else:
        want = oracle(x, dim % x.ndim, op)
    assert_pair(got.values, got.indices, want, what)
    plain = to_numpy(f(xt, dim=dim))
    assert np.array_equal(raw(plain), raw(to_numpy(got.values))), (what, "values without indices")
    return got


def check(dev, shape, dim: int, dt: str, op: str, patterns=PATTERNS, seed: int = 0, offset: int = 0) -> None:
    axis = dim % len(shape)
    for pat in patterns:
        x = cached(("cumarg", shape, axis, dt, op, pat, seed), lambda: make(shape, axis, dt, op, pat, seed))
        run(dev, x, dim, op, offset, (shape, dim, dt, op, pat, offset))


def check_spikes(dev, shape, dim: int, dt: str, op: str, positions) -> None:
    """One dominating element at p: the index stays p to the end of the line."""
    axis = dim % len(shape)
    n = shape[axis]
    for p in sorted({p for p in positions if 0 <= p < n}):
        x = make(shape, axis, dt, op, "spike", seed=p, p=p)
        got = run(dev, x, dim, op, what=(shape, dim, dt, op, "spike", p))
        tail = to_numpy(got.indices).take(np.arange(p, n), axis)
        assert (tail == p).all()


def check_specials(dev, shape, dim: int, dt: str, op: str, at) -> None:
    axis = dim % len(shape)
    x = special_lines(make(shape, axis, dt, op, "plateau", seed=5), axis, op, at)
    run(dev, x, dim, op, what=(shape, dim, dt, op, "special lines", tuple(at)))


# ------------------------------------------------------------- the oracles
def test_the_rule_and_the_oracles():
    """A sequential loop of the rule on short lines with NaN, zeros of both
    signs and ties, against torch's CPU kernels and the numpy construction;
    and the three lines the rule is stated with."""
    nan = float("nan")
    assert torch.cummax(torch.tensor([1, 1, nan, 5, nan, -0.0, 0.0]), 0).indices.tolist() == [0, 1, 2, 2, 4, 4, 4]
    assert torch.cummax(torch.tensor([0.0, -0.0, 0.0, -0.0]), 0).indices.tolist() == [0, 1, 2, 3]
    for dtype, low in ((torch.float32, -np.inf), (torch.int64, -2 ** 63)):
        assert torch.cummax(torch.full((5,), low, dtype=dtype), 0).indices.tolist() == [0, 1, 2, 3, 4]
    rng = np.random.default_rng(1)
    pool = np.array([0.0, -0.0, 1.0, 1.0, 2.0, -1.0, np.nan, np.inf, -np.inf])
    cpu = torch.device("cpu")
    for trial in range(60):
        n = int(rng.integers(1, 24))
        for op in OPS:
            for dt in ("f32", "f64"):
                line = rng.choice(pool, n).astype(NP[dt])
                v, i = by_the_rule(line.tolist(), op)
                wv, wi = oracle(line, 0, op)
                assert wi.tolist() == i, (line, op)
                assert np.array_equal(raw(np.array(v, dtype=NP[dt])), raw(wv)), (line, op)
                run(cpu, line, 0, op)  # and the CPU backend on the same line
            for dt in ("i32", "i64", "u32"):
                lo = 0 if dt == "u32" else -3
                line = rng.integers(lo, lo + 5, n).astype(NP[dt])
                v, i = by_the_rule(line.tolist(), op)
                wv, wi = oracle(line, 0, op)
                assert wi.tolist() == i and wv.tolist() == v, (line, op, dt)
                run(cpu, line, 0, op)
    # the numpy construction against torch where both exist
    x = rng.integers(0, 4, (5, 200)).astype(np.int32)
    for op in OPS:
        a = oracle(x.astype(np.uint32), 1, op)
        b = oracle(x, 1, op)
        assert np.array_equal(a[0], b[0].astype(np.uint32)) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_the_stated_lines(dev):
    nan = float("nan")
    x = torch.tensor([1, 1, nan, 5, nan, -0.0, 0.0], device=dev)
    assert cummax(x, return_indices=True).indices.tolist() == [0, 1, 2, 2, 4, 4, 4]
    assert cummax(x, dim=0, return_indices=True).indices.tolist() == [0, 1, 2, 2, 4, 4, 4]
    z = torch.tensor([0.0, -0.0, 0.0, -0.0], device=dev)
    assert cummax(z, return_indices=True).indices.tolist() == [0, 1, 2, 3]
    assert cummin(z, return_indices=True).indices.tolist() == [0, 1, 2, 3]
    for dtype, low, high in ((torch.float32, -np.inf, np.inf), (torch.int64, -2 ** 63, 2 ** 63 - 1)):
        assert cummax(torch.full((9,), low, dtype=dtype, device=dev), return_indices=True).indices.tolist() == list(range(9))
        assert cummin(torch.full((9,), high, dtype=dtype, device=dev), return_indices=True).indices.tolist() == list(range(9))
    both = scan(x, op="max", dim=0, return_indices=True)
    assert both.indices.tolist() == [0, 1, 2, 2, 4, 4, 4]


# --------------------------------------------------------------- row form
def row_ns(tile: int) -> list:
    return [1, 2, 3, 63, 64, 65, 255, 256, 257, tile - 1, tile, tile + 1, 2 * tile + 3]


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_workgroup_per_line(dev, dt, op):
    """Every n around the structural sizes, odd n (rows start off 16-byte
    alignment) included, for 1 row (a single line), 3 and 67; spikes around the
    first tile edge; special lines around it."""
    tile = edges(dev, dt)["tile"]
    for outer in (1, 3, 67):
        for n in row_ns(tile):
            check(dev, (outer, n), -1, dt, op)
    n = 2 * tile + 3
    if dev.type == "cuda":
        info = info_of(dev, (3, n), -1, dt)
        assert (info["form"], info["chunks"], info["waves"], info["tile"]) == ("row", 1, 4, tile)
    check_spikes(dev, (3, n), -1, dt, op, (0, 1, tile - 1, tile, 2 * tile - 1, 2 * tile, n - 1))
    check_specials(dev, (16, n), -1, dt, op, (tile, 2 * tile, 64, tile // 4))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_wave_per_line(dev, dt, op):
    """Many short rows: a wave per row on the GPU."""
    e = edges(dev, dt)
    rows, tile = e["wave_rows"] + 3, e["wave_tile"]
    if dev.type == "cuda":
        assert info_of(dev, (rows, 2 * tile + 3), -1, dt)["waves"] == 1
        assert info_of(dev, (e["wave_rows"] // 2, 65), -1, dt)["waves"] == 4  # the smallest row count
    for n in (1, 3, 64, 65, tile - 1, tile, tile + 1, 2 * tile + 3):
        check(dev, (rows, n), -1, dt, op, patterns=("plateau", "mono") if n % 2 else ("plateau", "ramp"))
    check_spikes(dev, (rows, 2 * tile + 3), -1, dt, op, (0, tile - 1, tile, 2 * tile))
    check_specials(dev, (rows, 2 * tile + 3), -1, dt, op, (tile, 2 * tile, 64))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_grid_stride(dev, dt):
    """Two workgroups for all the rows, in both row kernels."""
    e = edges(dev, dt)
    with knobs(dev, scan_dim_maxblocks=2):
        if dev.type == "cuda":
            assert info_of(dev, (67, 257), -1, dt)["workgroups"] == 2
            assert info_of(dev, (e["wave_rows"] + 3, 65), -1, dt)["workgroups"] == 2
        for op in OPS:
            check(dev, (67, 257), -1, dt, op)
            check(dev, (67, e["tile"] + 1), -1, dt, op, patterns=("plateau",))
            check(dev, (e["wave_rows"] + 3, 65), -1, dt, op, patterns=("plateau", "mono"))
            check_spikes(dev, (67, e["tile"] + 1), -1, dt, op, (1, e["tile"] - 1, e["tile"]))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [2, 3, 7])
@pytest.mark.parametrize("dt", MAIN)
def test_row_form_chunked(dev, dt, chunks):
    """Reduce-then-scan over pairs along the rows: n not divisible by K, n < K
    (empty chunks), chunks of several tiles; a spike at the last element of a
    chunk and the first of the next has to reach the end of the line through
    the totals."""
    tile = edges(dev, dt)["tile"]
    esize = np.dtype(NP[dt]).itemsize
    with knobs(dev, scan_dim_chunks=chunks):
        chunk = -(-(3 * tile + 5) // chunks)
        if dev.type == "cuda":
            info = info_of(dev, (3, 100), -1, dt)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * (esize + 8)
            assert info_of(dev, (3, 3 * tile + 5), -1, dt)["chunk"] == chunk
        for op in OPS:
            for n in (2, 5, 100, tile + 1, 3 * tile + 5, 7 * tile + 1):
                check(dev, (3, n), -1, dt, op)
            n = 3 * tile + 5
            check_spikes(dev, (3, n), -1, dt, op, (0, 1, tile - 1, tile, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk))
            check_specials(dev, (16, n), -1, dt, op, (chunk, tile, 2 * chunk, chunk + tile))
        check_specials(dev, (16, 5), -1, dt, "max", (1, 2))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_flattened_default(dev, dt):
    """dim=None indexes the flattened tensor: a single line, which the plan
    chunks across the device on its own."""
    tile = edges(dev, dt)["tile"]
    big = (1 << 20) + 5
    if dev.type == "cuda":
        info = info_of(dev, (big,), 0, dt)
        assert info["form"] == "flat" and info["chunks"] > 1 and info["ws_bytes"] == info["chunks"] * (
            np.dtype(NP[dt]).itemsize + 8)
        chunk = info["chunk"]
    else:
        chunk = big // 7
    for op in OPS:
        for pat in PATTERNS:
            run(dev, make((8 * tile + 3,), 0, dt, op, pat), None, op)
        for pat in ("plateau", "mono"):
            run(dev, make((big,), 0, dt, op, pat), None, op)
            run(dev, make((big,), 0, dt, op, pat), 0, op)
        check_spikes(dev, (big,), 0, dt, op, (1, chunk - 1, chunk))
        x = make((37, 301), 1, dt, op, "plateau")
        got = run(dev, x, None, op)  # against the oracle on x.reshape(-1)
        assert int(got.indices.max()) > 301  # positions in the flattened tensor, not along a dimension
        check_specials(dev, (1, 8 * tile + 3), 1, dt, op, (tile,))


# ------------------------------------------------------------ column form
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form(dev, dt, op):
    """inner around the workgroup's width (an odd inner forces scalar lanes),
    n around the unroll depth, a middle dimension of a 4-D shape."""
    e = edges(dev, dt)
    w, u = e["width"], e["unroll"]
    check(dev, (3, 50, 64), 1, dt, op)
    check_spikes(dev, (3, 50, 64), 1, dt, op, (0, 1, u - 1, u, 49))
    for inner in (2, 3, 63, 65, w - 1, w, w + 1):
        for n in (1, 2, u - 1, u, u + 1, 2 * u + 3):
            check(dev, (2, n, inner), 1, dt, op, patterns=("plateau", "mono") if n % 2 else ("plateau", "ramp"))
    if dev.type == "cuda":
        assert info_of(dev, (2, u + 1, w), 1, dt)["vector"] == e["vector"]
        assert info_of(dev, (2, u + 1, w + 1), 1, dt)["vector"] == 1
    check(dev, (2, 3, 33, 5), 2, dt, op)
    check(dev, (2, 3, 33, 5), 1, dt, op)
    check(dev, (2, 3, 33, 5), -4, dt, op)
    check_spikes(dev, (2, 3, 33, 5), 2, dt, op, (0, u, 32))
    check_specials(dev, (3, 50, 64), 1, dt, op, (u, 1, 2 * u))
    check_specials(dev, (3, 50, 5), 1, dt, op, (u, 1, 2 * u))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [2, 3, 7])
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_chunked(dev, dt, chunks):
    esize = np.dtype(NP[dt]).itemsize
    with knobs(dev, scan_dim_chunks=chunks):
        if dev.type == "cuda":
            info = info_of(dev, (3, 100, 64), 1, dt)
            assert info["chunks"] == chunks and info["ws_bytes"] == 3 * chunks * 64 * (esize + 8)
        for op in OPS:
            for inner in (3, 64, 65):
                for n in (5, 100, 257):
                    check(dev, (3, n, inner), 1, dt, op)
            chunk = -(-257 // chunks)
            check_spikes(dev, (3, 257, 64), 1, dt, op, (0, 1, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk))
            check_spikes(dev, (2, 257, 3), 1, dt, op, (chunk - 1, chunk))
            check_specials(dev, (3, 257, 64), 1, dt, op, (chunk, 2 * chunk, 8))
            check_specials(dev, (3, 257, 3), 1, dt, op, (chunk, 2 * chunk, 8))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dt", MAIN)
def test_column_form_grid_stride(dev, dt):
    with knobs(dev, scan_dim_maxblocks=2):
        if dev.type == "cuda":
            assert info_of(dev, (3, 17, 1025), 1, dt)["workgroups"] == 2
        for op in OPS:
            check(dev, (3, 17, 1025), 1, dt, op)
            check(dev, (3, 17, 1024), 1, dt, op, patterns=("plateau",))
            check_spikes(dev, (3, 17, 1025), 1, dt, op, (1, 16))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", ALL)
def test_every_dtype_in_every_regime(dev, dt, op):
    e = edges(dev, dt)
    tile = e["tile"]
    n = 2 * tile + 3
    check(dev, (5, 301), -1, dt, op)  # row, single pass
    check_specials(dev, (8, tile + 70), -1, dt, op, (tile, 64))
    check(dev, (e["wave_rows"] + 1, 67), -1, dt, op, patterns=("plateau",))  # row, a wave per line
    check(dev, (3, 50, 64), 1, dt, op)  # column, lane vectors
    check(dev, (3, 50, 65), 1, dt, op)  # column, scalar lanes
    check_specials(dev, (3, 50, 64), 1, dt, op, (8, 9))
    with knobs(dev, scan_dim_chunks=3):
        chunk = -(-n // 3)
        check(dev, (3, n), -1, dt, op)  # row, chunked
        check_spikes(dev, (3, n), -1, dt, op, (chunk - 1, chunk))
        check_specials(dev, (8, n), -1, dt, op, (chunk, 2 * chunk))
        check(dev, (3, 129, 64), 1, dt, op)  # column, chunked
        check(dev, (3, 129, 65), 1, dt, op)
        check_spikes(dev, (3, 129, 64), 1, dt, op, (42, 43))
        check_specials(dev, (3, 129, 64), 1, dt, op, (43, 86))


# ---------------------------------------------------------------- operands
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
@pytest.mark.parametrize("dt", ALL)
def test_operands_off_alignment_and_guards(dev, dt, chunks):
    """x one element off a 16-byte boundary; indices_out 8 bytes off one;
    values_out and indices_out as views inside sentinel-filled buffers whose
    elements on both sides stay as they were."""
    tile = edges(dev, dt)["tile"]
    for shape, dim in (((5, 301), 1), ((3, tile + 70), 1), ((3, 37, 13), 1), ((2, 45, 16), 1), ((67, 3), 0)):
        for op, off in (("max", 1), ("min", 3)):
            with knobs(dev, scan_dim_chunks=chunks):
                check(dev, shape, dim, dt, op, patterns=("plateau",), offset=off)
        x = make(shape, dim, dt, "max", "plateau", seed=2)
        size, lead, sentinel = int(np.prod(shape)), 37, 77
        vbuf = torch.full((lead + size + 64,), sentinel, dtype=torch.int64, device=dev).to(
            TORCH[dt] if dt != "u32" else torch.int32)
        if dt == "u32":
            vbuf = vbuf.view(torch.uint32)
        ibuf = torch.full((lead + size + 64,), sentinel, dtype=torch.int64, device=dev)
        vout = vbuf[lead:lead + size].view(shape)
        iout = ibuf[lead:lead + size].view(shape)
        assert iout.data_ptr() % 16 == 8
        with knobs(dev, scan_dim_chunks=chunks):
            got = cummax(place(x, dev, 1), dim=dim, return_indices=True, out=(vout, iout))
        assert got.values is vout and got.indices is iout
        assert_pair(vout, iout, oracle(x, dim, "max"), (shape, dt, "out views"))
        for buf in (vbuf, ibuf):
            b = to_numpy(buf)
            assert (b[:lead] == sentinel).all() and (b[lead + size:] == sentinel).all()


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("chunks", [0, 3])
def test_values_in_place_and_non_contiguous_input(dev, chunks):
    for dt in MAIN:
        tile = edges(dev, dt)["tile"]
        for shape, dim in (((3, 2 * tile + 3), 1), ((3, 129, 64), 1), ((3, 129, 5), 1)):
            for op in OPS:
                x = make(shape, dim, dt, op, "plateau", seed=4)
                want = oracle(x, dim, op)
                xt = to_torch(x.copy(), dev)  # (a CPU tensor shares the array's memory)
                iout = torch.empty(shape, dtype=torch.int64, device=dev)
                with knobs(dev, scan_dim_chunks=chunks):
                    got = scan(xt, op=op, dim=dim, return_indices=True, out=(xt, iout))
                assert got.values is xt and got.indices is iout
                assert_pair(xt, iout, want, (shape, dt, op, "in place"))
        x = make((40, 33), 0, dt, "max", "plateau")
        xt = to_torch(x, dev).t()  # (33, 40), not contiguous: copied
        assert not xt.is_contiguous()
        got = cummax(xt, dim=1, return_indices=True)
        assert_pair(got.values, got.indices, oracle(np.ascontiguousarray(x.T), 1, "max"), (dt, "transposed"))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_empty_shapes_and_rejected_arguments(dev):
    for shape, dim in (((3, 0), 1), ((0, 4), 1), ((0, 4), 0), ((2, 3, 0), 1), ((2, 0, 3), 1), ((0,), 0), ((0, 4), None)):
        for f in (cummax, cummin):
            got = f(torch.zeros(shape, device=dev), dim=dim, return_indices=True)
            assert got.values.shape == torch.Size(shape) and got.values.dtype == torch.float32
            assert got.indices.shape == torch.Size(shape) and got.indices.dtype == torch.int64
    x = torch.arange(12, dtype=torch.float32, device=dev).view(3, 4)
    y = torch.arange(6, dtype=torch.int64, device=dev).view(2, 1, 3) - 2
    got = cummin(y, dim=1, return_indices=True)  # n == 1: a copy and zeros
    assert torch.equal(got.values, y) and (got.indices == 0).all()
    assert torch.equal(cummax(x, dim=-1, return_indices=True).indices, cummax(x, dim=1, return_indices=True).indices)
    with pytest.raises(ValueError, match="sum"):
        scan(x, dim=0, return_indices=True)
    with pytest.raises(ValueError, match="exclusive"):
        cummax(x, dim=0, exclusive=True, return_indices=True)
    for algo in ("lookback", "rts"):
        with pytest.raises(TypeError, match="auto"):
            cummax(x.view(-1), algo=algo, return_indices=True)
        with pytest.raises(TypeError, match="auto"):
            cummin(x, dim=1, algo=algo, return_indices=True)
    good_v, good_i = torch.empty_like(x), torch.empty(3, 4, dtype=torch.int64, device=dev)
    assert cummax(x, dim=0, return_indices=True, out=(good_v, good_i)).indices is good_i
    bad = [(torch.empty(3, 4, dtype=torch.float64, device=dev), good_i),  # values: dtype
           (torch.empty(4, 3, device=dev), good_i),  # values: shape
           (good_v, torch.empty(3, 4, dtype=torch.int32, device=dev)),  # indices: dtype
           (good_v, torch.empty(12, dtype=torch.int64, device=dev)),  # indices: shape
           (good_v, torch.empty(4, 3, dtype=torch.int64, device=dev).t()),  # indices: not contiguous
           good_v]  # not a pair
    if dev.type == "cuda":
        bad += [(good_v.cpu(), good_i), (good_v, good_i.cpu())]  # device
    for out in bad:
        with pytest.raises(ValueError, match="out"):
            cummax(x, dim=0, return_indices=True, out=out)
    for d in (2, -3):
        with pytest.raises(IndexError):
            cummax(x, dim=d, return_indices=True)
    for d in (0, None):
        with pytest.raises(ValueError):
            cummax(torch.tensor(1.0, device=dev), dim=d, return_indices=True)
    with pytest.raises(TypeError):
        cummax(x.half(), dim=0, return_indices=True)
    with pytest.raises(ValueError, match="exclusive"):
        scan_dim_launch_info((3, 4), 0, exclusive=True, device=dev, indices=True)


# ------------------------------------------------------------------ GPU only
@pytest.mark.gpu
def test_launch_info_of_the_indexed_kernels(gpu):
    """The plan is the one of the values-only scans; only the workspace and the
    reading of a single line differ."""
    for shape, dim, dt in (((65536, 2048), -1, "f32"), ((16, 1 << 22), -1, "f32"), ((1 << 21, 64), 0, "i64"),
                           ((64, 1 << 21), 0, "f32"), ((1 << 22, 3), 0, "f32")):
        a = scan_dim_launch_info(shape, dim, dtype=TORCH[dt], op="max", device=gpu)
        b = info_of(gpu, shape, dim, dt)
        esize = np.dtype(NP[dt]).itemsize
        assert set(a) == set(b)
        for key in a:
            if key != "ws_bytes":
                assert a[key] == b[key], (shape, key)
        assert b["ws_bytes"] * esize == a["ws_bytes"] * (esize + 8)
    assert info_of(gpu, (4, 0, 3), 1, "f32")["workgroups"] == 0


@pytest.mark.gpu
def test_launch_mix_streams_and_repeats(gpu):
    """Fifty launches on one stream alternating an indexed row scan, an indexed
    column scan, a values-only chunked scan along a dimension and a 1-D
    look-back scan, all checked at the end: the totals of the two kinds and the
    look-back descriptors are apart. Then the same indexed scans on two
    streams, and a second run with identical bits."""
    from cme213x.ops.scan import check_lookback
    from cme213x.utils import tuning

    ri = make((3, 9001), 1, "f32", "max", "plateau")
    ci = make((3, 301, 33), 1, "i64", "min", "plateau")
    vs = np.random.default_rng(3).integers(-2 ** 40, 2 ** 40, (3, 7001))
    lb = np.random.default_rng(4).integers(-2 ** 40, 2 ** 40, 70_001)
    want = [oracle(ri, 1, "max"), oracle(ci, 1, "min"), np.cumsum(vs, axis=1), np.cumsum(lb)]
    dev = [to_torch(a, gpu) for a in (ri, ci, vs, lb)]
    calls = [lambda: cummax(dev[0], dim=1, return_indices=True), lambda: cummin(dev[1], dim=1, return_indices=True),
             lambda: scan(dev[2], dim=1), lambda: scan(dev[3], algo="lookback")]
    with tuning.override(scan_dim_chunks=7):
        assert info_of(gpu, (3, 9001), -1, "f32")["chunks"] == 7
        outs = [(k % 4, calls[k % 4]()) for k in range(50)]
        check_lookback(gpu)
        for j, o in outs:
            if j < 2:
                assert_pair(o.values, o.indices, want[j], ("mix", j))
            else:
                assert np.array_equal(to_numpy(o), want[j])
        # two streams, each with its own totals
        streams = [torch.cuda.Stream(gpu), torch.cuda.Stream(gpu)]
        res = []
        for rnd in range(4):
            for s, j in zip(streams, (0, 1)):
                s.wait_stream(torch.cuda.current_stream(gpu))
                with torch.cuda.stream(s):
                    res.append((j, calls[j]()))
        for s in streams:
            torch.cuda.current_stream(gpu).wait_stream(s)
        torch.cuda.synchronize(gpu)
        for j, o in res:
            assert_pair(o.values, o.indices, want[j], ("streams", j))
        first, second = calls[0](), calls[0]()
        assert np.array_equal(raw(to_numpy(first.values)), raw(to_numpy(second.values)))
        assert torch.equal(first.indices, second.indices)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 301, 64), (3, 9001)])
def test_graph_capture_of_a_chunked_indexed_scan(gpu, shape):
    """One capture, replayed on changed inputs; the totals were sized by the
    warm-up launch outside the capture, and a values-only scan in between does
    not touch them."""
    from cme213x.utils import tuning

    x = torch.zeros(shape, dtype=torch.int64, device=gpu)
    vout = torch.empty_like(x)
    iout = torch.empty_like(x)
    with tuning.override(scan_dim_chunks=5):
        cummax(x, dim=1, return_indices=True, out=(vout, iout))
        torch.cuda.synchronize(gpu)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            cummax(x, dim=1, return_indices=True, out=(vout, iout))
        other = to_torch(make(shape, 1, "i64", "max", "ramp", seed=9), gpu)
        for seed in (1, 2):
            a = make(shape, 1, "i64", "max", "plateau", seed=seed)
            x.copy_(to_torch(a, gpu))
            scan(other, dim=1)
            graph.replay()
            torch.cuda.synchronize(gpu)
            assert_pair(vout, iout, oracle(a, 1, "max"), ("graph", shape, seed))
