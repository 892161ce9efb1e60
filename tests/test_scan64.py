"""64-bit scan / reduce (int64, float64) on the HIP and the CPU backend.

int64 results are compared exactly against ``numpy.cumsum`` in int64 (which
wraps modulo 2^64, as the kernels do). float64 is compared bitwise where every
summation order is exact (integer-valued data with prefixes below 2^44) and
otherwise against a ``numpy.longdouble`` running sum under the worst-case
bound of any summation order, |y_i - ref_i| <= 1.01 * i * 2^-53 * sum_{j<=i}
|x_j| (i terms; the factor 1.01 covers the second-order term)."""
import numpy as np
import pytest
import torch

from cme213x.ops.scan import TILE64, lookback_timed_out, reduce, scan

T = TILE64
# T is the look-back tile; the reduce-then-scan tile is T // 2, so its tile
# edges are covered by T // 2 + 1 and by the multiples of T
EDGE_SIZES = [1, 2, 3, T // 2 + 1, T - 1, T, T + 1, 64 * T - 1, 64 * T + 1]
LARGE = 9_000_011
ALGOS = ["rts", "lookback"]
INT_PATTERNS = ["small", "wide", "minus1", "lowmax", "wrap"]
U = 2.0 ** -53


def _int_data(pattern: str, n: int) -> np.ndarray:
    rng = np.random.default_rng(n % 1000 + 17 * INT_PATTERNS.index(pattern))
    if pattern == "small":
        return rng.integers(-3, 4, n, dtype=np.int64)
    if pattern == "wide":  # prefixes cross 32-bit boundaries in both directions
        return rng.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    if pattern == "minus1":  # high word all ones from the first element
        return np.full(n, -1, dtype=np.int64)
    if pattern == "lowmax":  # the low half carries into the high half all the time
        return np.full(n, 2 ** 32 - 1, dtype=np.int64)
    sign = rng.integers(0, 2, n, dtype=np.int64) * 2 - 1  # near +-2^62: sums wrap modulo 2^64
    return sign * (2 ** 62) + rng.integers(-1000, 1000, n, dtype=np.int64)


_cache: dict = {}


def _case(kind: str, n: int):
    """(input, inclusive reference[, bound]) of one (data kind, size), computed
    once and shared by the algorithm / exclusive cases that follow it (one
    entry is kept: the parametrisation visits a (kind, size) consecutively)."""
    key = (kind, n)
    if key not in _cache:
        _cache.clear()
        if kind in INT_PATTERNS:
            x = _int_data(kind, n)
            with np.errstate(over="ignore"):
                _cache[key] = (x, np.cumsum(x, dtype=np.int64))
        elif kind == "f64_exact":
            x = np.floor(np.random.default_rng(n % 1000).uniform(0, 2 ** 20, n))
            _cache[key] = (x, np.cumsum(x))  # every prefix < 2^44: exact in any order
        else:  # f64_uniform
            x = np.random.default_rng(n % 1000 + 5).uniform(-1, 1, n)
            ref = np.cumsum(x.astype(np.longdouble))
            bound = 1.01 * np.arange(1, n + 1) * U * np.cumsum(np.abs(x))
            _cache[key] = (x, ref, bound)
    return _cache[key]


def _excl(inc: np.ndarray) -> np.ndarray:
    return np.concatenate([np.zeros(1, dtype=inc.dtype), inc[:-1]])


def _check_uniform(y: np.ndarray, ref, bound, exclusive: bool) -> None:
    if exclusive:  # element i holds the prefix of i terms: the bound of the preceding element
        ref, bound = _excl(ref), _excl(bound)
    err = np.abs(y.astype(np.longdouble) - ref)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"element {worst}: error {float(err[worst]):.3e} > bound {float(bound[worst]):.3e}"


# --------------------------------------------------------------------- GPU scans
@pytest.mark.gpu
def test_large_size_covers_both_launch_shapes(gpu):
    """The large size must give the look-back more tiles than it has
    workgroups (so blocks walk several tiles) and the reduce-then-scan at
    least three tiles per chunk (first / middle / last tile of a chunk)."""
    from cme213x.ops.scan import scan64_launch_info

    info = scan64_launch_info(LARGE, gpu)
    assert info["tile"] == T
    assert info["tiles"] == (LARGE + T - 1) // T
    assert info["tiles"] > info["lookback_workgroups"] >= 1, info
    assert info["rts_tiles_per_chunk"] >= 3, info
    assert info["rts_chunks"] <= 1024 and info["rts_tile"] == T // 2


@pytest.mark.gpu
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", EDGE_SIZES + [LARGE])
@pytest.mark.parametrize("pattern", INT_PATTERNS)
def test_scan_int64_gpu(gpu, pattern, n, algo, exclusive):
    x, ref = _case(pattern, n)
    y = scan(torch.from_numpy(x).to(gpu), exclusive, algo=algo)
    assert y.dtype == torch.int64
    np.testing.assert_array_equal(y.cpu().numpy(), _excl(ref) if exclusive else ref)
    if algo == "lookback":
        assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", EDGE_SIZES + [LARGE])
def test_scan_float64_exact_gpu(gpu, n, algo, exclusive):
    x, ref = _case("f64_exact", n)
    y = scan(torch.from_numpy(x).to(gpu), exclusive, algo=algo)
    assert y.dtype == torch.float64
    want = _excl(ref) if exclusive else ref
    assert np.array_equal(y.cpu().numpy().view(np.int64), want.view(np.int64))  # bitwise
    if algo == "lookback":
        assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", EDGE_SIZES + [LARGE])
def test_scan_float64_uniform_gpu(gpu, n, algo, exclusive):
    x, ref, bound = _case("f64_uniform", n)
    y = scan(torch.from_numpy(x).to(gpu), exclusive, algo=algo).cpu().numpy()
    _check_uniform(y, ref, bound, exclusive)
    if algo == "lookback":
        assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [T + 1, LARGE])
def test_scan_float64_rts_bitwise_reproducible(gpu, n):
    x = torch.from_numpy(_case("f64_uniform", n)[0]).to(gpu)
    a = scan(x, algo="rts")
    b = scan(x, algo="rts")
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert torch.equal(a.view(torch.int64), scan(x).view(torch.int64))  # "auto" is rts for float64


@pytest.mark.gpu
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("n", [T + 1, LARGE])
@pytest.mark.parametrize("kind", ["wide", "f64_exact"])
def test_scan_8_byte_aligned_views(gpu, kind, n, algo, exclusive):
    """x[1:] of a 64-bit tensor is contiguous and 8-byte but not 16-byte
    aligned; so is the out= view."""
    xs, ref = _case(kind, n)
    base = torch.empty(n + 1, dtype=torch.from_numpy(xs).dtype, device=gpu)
    x = base[1:]
    x.copy_(torch.from_numpy(xs))
    out = torch.empty_like(base)[1:]
    assert x.is_contiguous() and x.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
    y = scan(x, exclusive, out=out, algo=algo)
    assert y.data_ptr() == out.data_ptr()
    want = _excl(ref) if exclusive else ref
    assert np.array_equal(out.cpu().numpy().view(np.int64), want.view(np.int64))
    if algo == "lookback":
        assert not lookback_timed_out(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("kind", ["wide", "f64_exact"])
def test_scan_in_place(gpu, kind, algo, exclusive):
    n = 64 * T + 1
    xs, ref = _case(kind, n)
    x = torch.from_numpy(xs).to(gpu)
    y = scan(x, exclusive, out=x, algo=algo)
    assert y is x
    want = _excl(ref) if exclusive else ref
    assert np.array_equal(x.cpu().numpy().view(np.int64), want.view(np.int64))
    if algo == "lookback":
        assert not lookback_timed_out(gpu)


# ------------------------------------------------------------- look-back state
@pytest.mark.gpu
def test_lookback64_epochs_reuse_workspace(gpu):
    """200 back-to-back int64 look-back scans on one stream share one
    descriptor array, a new epoch per launch and no memset."""
    n = 3 * T + 5
    g = torch.Generator().manual_seed(11)
    xs = torch.randint(-2 ** 40, 2 ** 40, (200, n), generator=g, dtype=torch.int64)
    xd = xs.to(gpu)
    outs = [scan(xd[i], exclusive=bool(i % 3 == 1), algo="lookback") for i in range(200)]
    assert not lookback_timed_out(gpu)
    got = torch.stack(outs).cpu()
    ref = torch.cumsum(xs, 1)
    excl = torch.arange(200) % 3 == 1
    ref[excl] -= xs[excl]
    assert torch.equal(got, ref)


@pytest.mark.gpu
def test_lookback_int32_and_int64_alternate_on_one_stream(gpu):
    """32-bit and 64-bit look-back scans issued back to back never read each
    other's descriptor words; both sizes span more than 64 tiles (several
    groups of the two-level look-back)."""
    n32, n64 = 65 * 16384 + 7, 65 * T + 3
    g = torch.Generator().manual_seed(12)
    pairs = []
    for i in range(6):
        a = torch.randint(-50, 50, (n32,), generator=g, dtype=torch.int32)
        b = torch.randint(-2 ** 40, 2 ** 40, (n64,), generator=g, dtype=torch.int64)
        ya = scan(a.to(gpu), exclusive=bool(i & 1), algo="lookback")
        yb = scan(b.to(gpu), exclusive=bool(i & 2), algo="lookback")
        pairs.append((ya, torch.cumsum(a.long(), 0) - (a.long() if i & 1 else 0),
                      yb, torch.cumsum(b, 0) - (b if i & 2 else 0)))
    assert not lookback_timed_out(gpu)
    for ya, ra, yb, rb in pairs:
        assert torch.equal(ya.cpu().long(), ra)
        assert torch.equal(yb.cpu(), rb)


@pytest.mark.gpu
def test_lookback64_two_streams(gpu):
    n = 300 * T + 1
    g = torch.Generator().manual_seed(13)
    xs = [torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64) for _ in range(2)]
    xd = [x.to(gpu) for x in xs]
    torch.cuda.synchronize(gpu)
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    outs = []
    for x, s in zip(xd, streams):
        with torch.cuda.stream(s):
            outs.append(scan(x, algo="lookback"))
    assert not lookback_timed_out(gpu)  # synchronises the device
    for x, y in zip(xs, outs):
        assert torch.equal(y.cpu(), torch.cumsum(x, 0))


@pytest.mark.gpu
def test_graph_capture_int64_lookback_and_float64_rts(gpu):
    """One int64 look-back scan (epoch 0: the descriptors are zeroed inside the
    graph) and one float64 reduce-then-scan captured on a single stream; two
    replays on changed inputs equal numpy exactly."""
    n = 70 * T + 9
    g = torch.Generator().manual_seed(14)
    xi = torch.zeros(n, dtype=torch.int64, device=gpu)
    xf = torch.zeros(n, dtype=torch.float64, device=gpu)
    oi, of = torch.empty_like(xi), torch.empty_like(xf)
    scan(xi, out=oi, algo="lookback")  # warm-up outside the capture
    scan(xf, out=of, algo="rts")
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scan(xi, out=oi, algo="lookback")
        scan(xf, out=of, algo="rts")
    for _ in range(2):
        a = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64)
        b = torch.randint(0, 2 ** 20, (n,), generator=g, dtype=torch.int64).double()
        xi.copy_(a.to(gpu))
        xf.copy_(b.to(gpu))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert torch.equal(oi.cpu(), torch.cumsum(a, 0))
        assert torch.equal(of.cpu(), torch.cumsum(b, 0))  # integer-valued, < 2^44: exact
        assert torch.equal(scan(xi, algo="lookback").cpu(), torch.cumsum(a, 0))  # eager, between replays
    assert not lookback_timed_out(gpu)


# --------------------------------------------------------------------- reduce
def _reduce_cases(dev):
    rng = np.random.default_rng(3)
    n = 3_000_017
    xi = rng.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    ti = torch.from_numpy(xi).to(dev)
    assert reduce(ti, "sum").item() == int(xi.sum())
    assert reduce(ti, "max").item() == int(xi.max())
    assert reduce(ti, "min").item() == int(xi.min())
    xw = _int_data("wrap", 100_003)  # the sum wraps modulo 2^64, like numpy's
    with np.errstate(over="ignore"):
        assert reduce(torch.from_numpy(xw).to(dev), "sum").item() == int(xw.sum(dtype=np.int64))
    xf = rng.uniform(-1, 1, n)
    tf = torch.from_numpy(xf).to(dev)
    assert reduce(tf, "max").item() == xf.max()
    assert reduce(tf, "min").item() == xf.min()
    ref = float(np.sum(xf.astype(np.longdouble)))
    bound = 1.01 * n * U * float(np.abs(xf).sum())
    got = reduce(tf, "sum")
    assert got.dtype == torch.float64 and got.dim() == 0
    assert abs(got.item() - ref) <= bound, (got.item(), ref, bound)
    for k in (1, 2):  # n = 1 and n = 2
        assert reduce(ti[:k], "sum").item() == int(xi[:k].sum())
        assert reduce(ti[:k], "max").item() == int(xi[:k].max())
        assert reduce(ti[:k], "min").item() == int(xi[:k].min())
        assert reduce(tf[:k], "sum").item() == float(xf[:k].sum())
        assert reduce(tf[:k], "max").item() == xf[:k].max()
        assert reduce(tf[:k], "min").item() == xf[:k].min()
    neg = torch.full((5,), -7, dtype=torch.int64).to(dev)  # all negative: the max identity is INT64_MIN
    assert reduce(neg, "max").item() == -7 and reduce(-neg, "min").item() == 7
    for t in (ti[:100], tf[:100]):
        with pytest.raises(TypeError):
            reduce(t, "sum", algo="tree")


@pytest.mark.gpu
def test_reduce64_gpu(gpu):
    _reduce_cases(gpu)


def test_reduce64_cpu():
    _reduce_cases(torch.device("cpu"))


# ---------------------------------------------------------- rejected algorithms
@pytest.mark.parametrize("algo", ["blelloch", "hillis", "blelloch_mlevel", "hillis_mlevel"])
def test_tree_algorithms_reject_64_bit_cpu(algo):
    for dt in (torch.int64, torch.float64):
        with pytest.raises(TypeError, match="rts.*lookback"):
            scan(torch.ones(100, dtype=dt), algo=algo)


@pytest.mark.gpu
def test_tree_algorithms_reject_64_bit_gpu(gpu):
    with pytest.raises(TypeError, match="rts.*lookback"):
        scan(torch.ones(100, dtype=torch.int64, device=gpu), algo="blelloch")


# ------------------------------------------------------------------ CPU backend
CPU_SIZES = [1, 1000, 1_000_003]


@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("n", CPU_SIZES)
@pytest.mark.parametrize("pattern", INT_PATTERNS)
def test_scan_int64_cpu(pattern, n, exclusive):
    x, ref = _case(pattern, n)
    y = scan(torch.from_numpy(x), exclusive)
    assert y.dtype == torch.int64
    np.testing.assert_array_equal(y.numpy(), _excl(ref) if exclusive else ref)


@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("n", CPU_SIZES)
def test_scan_float64_cpu(n, exclusive):
    x, ref = _case("f64_exact", n)
    y = scan(torch.from_numpy(x), exclusive)
    want = _excl(ref) if exclusive else ref
    assert np.array_equal(y.numpy().view(np.int64), want.view(np.int64))
    x, ref, bound = _case("f64_uniform", n)
    _check_uniform(scan(torch.from_numpy(x), exclusive).numpy(), ref, bound, exclusive)


def test_scan_cpu_in_place_and_out():
    x, ref = _case("wide", 1000)
    t = torch.from_numpy(x.copy())
    assert scan(t, out=t) is t
    np.testing.assert_array_equal(t.numpy(), ref)
    with pytest.raises(ValueError):
        scan(torch.from_numpy(x), out=torch.empty(1000, dtype=torch.int32))
