"""Running max / min scans (``scan(..., op="max" / "min")``, ``cummax``,
``cummin``) on the HIP and the CPU backend, every scan dtype.

Every comparison is on bit patterns (the sign of a zero and the bits of a NaN
included). The oracle is ``torch.cummax`` / ``torch.cummin`` on CPU tensors for
float32 / float64 / int32 / int64 and ``numpy.maximum.accumulate`` /
``minimum.accumulate`` for uint32 (which torch does not scan); an exclusive
result is the operator's identity followed by ``inclusive[:-1]``. One small
case checks the torch oracle itself against a sequential loop of the rule
``(b >= a or b != b) ? b : a``.

Max is idempotent: on i.i.d. data the running max freezes inside the first
tile and a kernel that drops every carry still passes. The data here keeps the
carry visible -- a noisy ramp (the running max changes in every tile),
strictly decreasing data (every output is x[0]: the carry crosses every tile,
group and round), late spikes on both sides of every structural edge, and
one-signed ramps (a zero pad or a zero identity would win). "min" data is the
mirror image of the "max" data.

GPU sizes are the smallest that reach each mechanism: the 4096-element
reduce-then-scan tile, the look-back tile (16384 elements of 32 bits, 8192 of
64), the 64-tile group of the two-level look-back, and -- from the launch-info
query -- one size per width at which every workgroup of the persistent grid
goes round its tile loop at least three times.
"""
import numpy as np
import pytest
import torch

from cme213x.ops.scan import TILE64, check_lookback, cummax, cummin, scan, scan64_launch_info, scan_launch_info
from scan_util import to_numpy, to_torch, view_of

T32, T64, RTS = 16384, TILE64, 4096
DTYPES = {"f32": np.float32, "i32": np.int32, "u32": np.uint32, "i64": np.int64, "f64": np.float64}
TORCH = {"f32": torch.float32, "i32": torch.int32, "u32": torch.uint32, "i64": torch.int64, "f64": torch.float64}
FLOATS = ["f32", "f64"]
OPS = ["max", "min"]
PATTERNS = ["ramp", "decreasing", "spike", "onesigned"]
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]


def tile_of(dt: str) -> int:
    return T64 if dt in ("i64", "f64") else T32


def sizes_of(dt: str) -> list[int]:
    t = tile_of(dt)
    return [1, 3, 63, 64, 65, RTS - 1, RTS, RTS + 1, t - 1, t, t + 1, 64 * t - 1, 64 * t, 64 * t + 1]


SIZE_CASES = [(dt, n) for dt in DTYPES for n in sizes_of(dt)]


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def algos(dev) -> tuple:
    return ("lookback", "rts") if dev.type == "cuda" else ("auto",)


def finish(dev) -> None:
    """Every GPU test ends with the look-back give-up word still clear."""
    if dev.type == "cuda":
        check_lookback(dev)


# ---------------------------------------------------------------- oracle
def identity(op: str, dtype) -> np.generic:
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(-np.inf if op == "max" else np.inf)
    info = np.iinfo(dtype)
    return dtype.type(info.min if op == "max" else info.max)


def oracle(x: np.ndarray, op: str) -> np.ndarray:
    if x.dtype == np.uint32:
        return (np.maximum if op == "max" else np.minimum).accumulate(x)
    f = torch.cummax if op == "max" else torch.cummin
    return f(torch.from_numpy(x), 0).values.numpy()


def excl(inc: np.ndarray, op: str) -> np.ndarray:
    return np.concatenate([np.array([identity(op, inc.dtype)], dtype=inc.dtype), inc[:-1]])


def raw(a: np.ndarray) -> np.ndarray:
    """The bits of every element, signs of zeros and NaN payloads included."""
    return a.view({4: np.int32, 8: np.int64}[a.itemsize]) if a.dtype.kind == "f" else a


def assert_same_bits(got, want: np.ndarray, what: str) -> None:
    g = to_numpy(got) if isinstance(got, torch.Tensor) else got
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    bad = np.flatnonzero(raw(g) != raw(want))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[0]}: {g[bad[0]]!r} != {want[bad[0]]!r}"


def mirror(x: np.ndarray) -> np.ndarray:
    """The "min" data of "max" data: the order of the values reversed."""
    return (np.uint32(0xFFFFFFFF) - x) if x.dtype == np.uint32 else -x


def edges_of(dt: str, n: int, rounds: int = 0) -> list[int]:
    t = tile_of(dt)
    return [e for e in (64, RTS, t, 2 * t, 64 * t, rounds) if 1 < e and e + 1 < n]


def make_max_data(dt: str, pattern: str, n: int, rounds: int = 0) -> np.ndarray:
    """Data for op="max" (mirror() gives the "min" data). Integer-valued in
    float64 first, then offset / scaled into the dtype."""
    rng = np.random.default_rng(n % 9973 + 31 * PATTERNS.index(pattern))
    dtype = DTYPES[dt]
    i = np.arange(n, dtype=np.int64)
    if pattern == "ramp":  # the running max changes in every tile
        v = i + rng.integers(-50, 51, n)
        if dt == "u32":
            v += 100
        elif dt[0] == "f":
            return (v + rng.uniform(-0.5, 0.5, n)).astype(dtype)
        return v.astype(dtype)
    if pattern == "decreasing":  # every output is x[0]
        v = 3 * (n - i) if dt != "f32" else (n - i)  # float32: exact (strict) up to 2^24 elements
        if dt in ("i32", "i64", "f32", "f64"):
            v = v - n  # both signs
        return v.astype(dtype)
    if pattern == "spike":  # low noisy floor, rising spikes one element before and after every edge
        v = rng.integers(-100, -50, n)
        for k, e in enumerate(edges_of(dt, n, rounds)):
            v[e - 1] = 1000 + 2 * k
            v[e + 1] = 1001 + 2 * k
        if dt == "u32":
            v += 200
        return v.astype(dtype)
    # one-signed: an all-negative rising ramp (a zero pad or identity would win)
    v = i - n - 60 + rng.integers(-50, 51, n)
    assert v.max() < 0
    if dt == "u32":  # a rising ramp across 2^31: a signed comparison would order its two halves wrongly
        return (v + n // 2 + 2 ** 31).astype(np.uint32)
    if dt == "i64":  # beyond -2^53, in odd steps: exact in int64 only
        return (7 * v - 2 ** 53).astype(np.int64)
    return v.astype(dtype)


_cache: dict = {}


def case(dt: str, pattern: str, op: str, n: int, rounds: int = 0):
    """(input, inclusive reference), computed once for the algorithm / exclusive
    cases that share it (one entry is kept)."""
    key = (dt, pattern, op, n, rounds)
    if key not in _cache:
        _cache.clear()
        x = make_max_data(dt, pattern, n, rounds)
        if op == "min":
            x = mirror(x)
        _cache[key] = (x, oracle(x, op))
    return _cache[key]


def run_all(x: np.ndarray, ref: np.ndarray, op: str, dev, what: str, exclusives=(False, True)) -> None:
    xt = to_torch(x, dev)
    for algo in algos(dev):
        for e in exclusives:
            y = scan(xt, e, algo=algo, op=op)
            assert y.dtype == xt.dtype
            assert_same_bits(y, excl(ref, op) if e else ref, f"{what} {op} {algo} exclusive={e}")
    finish(dev)


# ------------------------------------------------------------ every dtype
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dt,n", SIZE_CASES)
def test_scan_minmax(dev, dt, n, pattern, op):
    x, ref = case(dt, pattern, op, n)
    if pattern == "decreasing":
        assert np.all(ref == x[0])
    if pattern == "onesigned" and dt != "u32":
        assert np.all(x < 0) if op == "max" else np.all(x > 0)
    if pattern == "onesigned" and dt == "u32" and n > 200:
        assert x.min() < 2 ** 31 <= x.max()
    run_all(x, ref, op, dev, f"{dt} {pattern} n={n}")


def test_data_makes_a_dropped_carry_visible():
    """On the oracle alone: in every pattern the reference changes (ramp,
    spike, one-signed) or depends on element 0 (decreasing) beyond the first
    tile, so a scan that restarts at a tile edge cannot pass."""
    for dt in DTYPES:
        t, n = tile_of(dt), 64 * tile_of(dt) + 1
        for pattern in PATTERNS:
            for op in OPS:
                x, ref = case(dt, pattern, op, n)
                restarted = oracle(x[t:], op)  # a scan that lost the carry into tile 1
                assert np.any(restarted != ref[t:]), (dt, pattern, op)
                if pattern in ("ramp", "onesigned"):  # the running value keeps changing: every tile has a new one
                    assert np.unique(ref[::RTS]).size == ref[::RTS].size, (dt, pattern, op)


def test_wrappers_are_scan_with_op():
    x = torch.tensor([1.0, 3.0, 2.0, -5.0])
    assert torch.equal(cummax(x), torch.tensor([1.0, 3.0, 3.0, 3.0]))
    assert torch.equal(cummin(x), torch.tensor([1.0, 1.0, 1.0, -5.0]))
    assert torch.equal(cummax(x, exclusive=True), torch.tensor([-np.inf, 1.0, 3.0, 3.0]))
    assert torch.equal(cummin(x, exclusive=True), torch.tensor([np.inf, 1.0, 1.0, 1.0]))
    u = to_torch(np.array([5, 2 ** 31 + 1, 7], dtype=np.uint32), "cpu")
    assert to_numpy(cummax(u, exclusive=True)).tolist() == [0, 5, 2 ** 31 + 1]
    assert to_numpy(cummin(u, exclusive=True)).tolist() == [0xFFFFFFFF, 5, 5]
    i = torch.tensor([-3, -7], dtype=torch.int64)
    assert cummax(i, exclusive=True).tolist() == [-2 ** 63, -3] and cummin(i, exclusive=True).tolist() == [2 ** 63 - 1, -3]


# ------------------------------------------------- three rounds of the grid
def three_round_size(dt: str, op: str, gpu) -> tuple[int, int]:
    """(n, elements per round): the smallest size that sends every workgroup of
    the persistent look-back grid round its tile loop three times and gives the
    reduce-then-scan three tiles per chunk -- asserted on the launch-info
    query of the max / min kernels themselves."""
    t = tile_of(dt)
    wide = t == T64
    info = (lambda n, e: scan64_launch_info(n, gpu, op=op, dtype=TORCH[dt], exclusive=e)) if wide else \
        (lambda n, e: scan_launch_info(n, exclusive=e, device=gpu, dtype=TORCH[dt], op=op))
    key = "lookback_workgroups" if wide else "workgroups"
    cap = max(info(2 ** 31, e)[key] for e in (False, True))  # the co-resident grid of a long scan
    n = max(3 * cap * t, 3 * 1024 * RTS) + t + 3
    for e in (False, True):
        d = info(n, e)
        assert d["tile"] == t and d["tiles"] == (n + t - 1) // t
        assert d["tiles"] >= 3 * d[key] >= 3, d
        assert d["rts_tile"] == RTS and d["rts_tiles_per_chunk"] >= 3 and d["rts_chunks"] <= 1024, d
    return n, cap * t


@pytest.mark.gpu
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", ["f32", "i64"])
def test_three_rounds_of_the_persistent_grid(gpu, dt, op):
    n, rounds = three_round_size(dt, op, gpu)
    x, ref = case(dt, "ramp", op, n)
    run_all(x, ref, op, gpu, f"{dt} ramp n={n}")
    x, ref = case(dt, "decreasing", op, n)
    assert np.all(ref == x[0])
    run_all(x, ref, op, gpu, f"{dt} decreasing n={n}", exclusives=(False,))
    x, ref = case(dt, "spike", op, n, rounds)
    assert x[rounds - 1] != x[rounds] and x[rounds + 1] != x[rounds]  # spikes at the round edge
    run_all(x, ref, op, gpu, f"{dt} spike n={n}", exclusives=(True,))


# -------------------------------------------------------------- floats
def structural_positions(dt: str, dev) -> dict:
    """An element index inside each structure a carry crosses: the tile, the
    64-tile group and (GPU) the round of the persistent grid."""
    t = tile_of(dt)
    pos = {"tile": t, "group": 64 * t}
    if dev.type == "cuda":
        wide = t == T64
        for op in OPS:
            for e in (False, True):
                d = scan64_launch_info(2 ** 31, dev, op=op, dtype=TORCH[dt], exclusive=e) if wide else \
                    scan_launch_info(2 ** 31, exclusive=e, device=dev, dtype=TORCH[dt], op=op)
                pos[f"round_{op}_{int(e)}"] = t * d["lookback_workgroups" if wide else "workgroups"]
    return pos


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", FLOATS)
def test_nan_is_sticky_across_every_edge(dev, dt, op):
    """One (default, quiet) NaN just before and just after a tile, a group and
    a round edge: finite before it, NaN from it on."""
    t = tile_of(dt)
    for edge in sorted(set(structural_positions(dt, dev).values())):
        for p in (edge - 1, edge):
            n = p + t + 3
            x = make_max_data(dt, "ramp", n)
            x = mirror(x) if op == "min" else x
            x[p] = np.nan
            ref = oracle(x, op)
            assert np.all(np.isfinite(ref[:p])) and np.all(np.isnan(ref[p:]))
            run_all(x, ref, op, dev, f"{dt} NaN at {p}")


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", FLOATS)
def test_infinities(dev, dt, op):
    t = tile_of(dt)
    n = 3 * t + 5
    x = make_max_data(dt, "ramp", n)
    x[[0, 7, t, t + 1]] = -np.inf  # the identity itself, as data
    x[2 * t + 1] = np.inf
    x = mirror(x) if op == "min" else x
    ref = oracle(x, op)
    assert np.isinf(ref[0]) and np.all(np.isfinite(ref[1:2 * t + 1])) and np.all(np.isinf(ref[2 * t + 1:]))
    run_all(x, ref, op, dev, f"{dt} inf")


def zero_pairs(dt: str, dev) -> dict:
    t = tile_of(dt)
    pairs = {"lane_vector": (8, 9), "waves": (10, t // 2 + 3), "tiles": (t - 2, t + 5), "tile_edge": (t - 1, t),
             "groups": (t + 1, 65 * t + 2)}
    for k, r in structural_positions(dt, dev).items():
        if k.startswith("round"):
            pairs[k] = (7, r + 7)  # tiles 0 and G: two rounds of workgroup 0
    return pairs


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("order", ["plus_first", "minus_first"])
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", FLOATS)
def test_signed_zeros_later_wins(dev, dt, op, order):
    """All -1.0 (max; +1.0 for min) but one +0.0 and one -0.0: among equal
    values the LATER element wins, wherever the two lie -- in one lane vector,
    in two waves of a tile, in adjacent tiles, in two groups, in two rounds of
    one workgroup. A look-back window or a carry folded in the wrong operand
    order returns the earlier zero."""
    done = set()
    for where, (p, q) in zero_pairs(dt, dev).items():
        if (p, q) in done:
            continue
        done.add((p, q))
        n = q + 77
        x = np.full(n, -1.0 if op == "max" else 1.0, dtype=DTYPES[dt])
        first, second = (0.0, -0.0) if order == "plus_first" else (-0.0, 0.0)
        x[p], x[q] = first, second
        ref = oracle(x, op)
        assert np.signbit(ref[q - 1]) == np.signbit(x[p]) and np.all(np.signbit(ref[q:]) == np.signbit(x[q]))
        run_all(x, ref, op, dev, f"{dt} zeros {where} {order}")


def test_torch_oracle_follows_the_rule():
    """A few thousand mixed values (both zeros, infinities, a NaN) scanned by a
    plain sequential loop of the rule: the torch oracle agrees bit for bit, and
    so does the CPU backend."""
    rng = np.random.default_rng(5)
    vals = np.array([-2.0, -1.0, -0.0, 0.0, 0.5, 1.0, -np.inf], dtype=np.float64)
    x = vals[rng.integers(0, vals.size, 3000)]
    x[1500:1510] = [0.0, -0.0, 1.0, -0.0, 0.0, 1.0, -2.0, np.inf, -np.inf, 0.0]
    x[2500] = np.nan
    for dtype in (np.float32, np.float64):
        xs = x.astype(dtype)
        for op in OPS:
            run, out = identity(op, dtype), []
            for b in xs:
                later = (b >= run) if op == "max" else (b <= run)
                run = b if (later or b != b) else run
                out.append(run)
            want = np.array(out, dtype=dtype)
            assert_same_bits(oracle(xs, op), want, f"torch {op}")
            assert_same_bits(scan(torch.from_numpy(xs), op=op), want, f"cpu {op}")
            assert_same_bits(scan(torch.from_numpy(xs), True, op=op), excl(want, op), f"cpu exclusive {op}")


# ------------------------------------------------------------ plumbing
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_in_place(dev, dt, op):
    n = 64 * tile_of(dt) + 1
    x, ref = case(dt, "ramp", op, n)
    for algo in algos(dev):
        for e in (False, True):
            xt = to_torch(x, dev)
            assert scan(xt, e, out=xt, algo=algo, op=op) is xt
            assert_same_bits(xt, excl(ref, op) if e else ref, f"{dt} in place {algo} {e}")
    finish(dev)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("dt", list(DTYPES))
def test_element_aligned_views(dev, dt, op):
    """buf[1:] as input and as output: 4-byte aligned for 32-bit elements
    (staged through an aligned copy on the GPU), 8-byte aligned for 64-bit."""
    n = tile_of(dt) + 1
    x, ref = case(dt, "onesigned", op, n)
    xv = view_of(x, 1, dev)
    assert xv.data_ptr() % 16 == x.itemsize
    for algo in algos(dev):
        for e in (False, True):
            out = torch.zeros(n + 1, dtype=xv.dtype, device=dev)[1:]
            y = scan(xv, e, out=out, algo=algo, op=op)
            assert y.data_ptr() == out.data_ptr()
            assert_same_bits(out, excl(ref, op) if e else ref, f"{dt} views {algo} {e}")
            assert_same_bits(scan(xv, e, algo=algo, op=op), excl(ref, op) if e else ref, f"{dt} view in {algo} {e}")
    finish(dev)


def sum_oracle(x: np.ndarray) -> np.ndarray:
    with np.errstate(over="ignore"):
        return np.cumsum(x, dtype=x.dtype)


@pytest.mark.gpu
@pytest.mark.parametrize("width", [32, 64])
def test_sum_max_min_alternate_on_one_stream(gpu, width):
    """50 back-to-back look-back launches on one stream, alternating sum, max
    and min scans and the dtypes of one width: they share one descriptor array
    and one epoch count. More than 64 tiles each (several look-back groups)."""
    t = T32 if width == 32 else T64
    n = 65 * t + 7
    sums, mm = (("i32", "u32"), ("f32", "i32", "u32")) if width == 32 else (("i64",), ("f64", "i64"))
    plan = []
    for k in range(50):
        op = ("sum", "max", "min")[k % 3]
        dt = (sums if op == "sum" else mm)[(k // 3) % len(sums if op == "sum" else mm)]
        e = bool(k % 2)
        if op == "sum":
            x = np.random.default_rng(k).integers(-50, 50, n).astype(DTYPES[dt])
            inc = sum_oracle(x)
            want = np.concatenate([np.zeros(1, dtype=x.dtype), inc[:-1]]) if e else inc
        else:
            x, inc = case(dt, "ramp", op, n)
            x = np.roll(x, k) if dt[0] != "f" else x + DTYPES[dt](k)  # a new input per launch
            inc = oracle(x, op)
            want = excl(inc, op) if e else inc
        plan.append((op, dt, e, to_torch(x, gpu), want))
    torch.cuda.synchronize(gpu)
    outs = [scan(xt, e, algo="lookback", op=op) for op, dt, e, xt, want in plan]
    check_lookback(gpu)
    for k, ((op, dt, e, xt, want), y) in enumerate(zip(plan, outs)):
        assert_same_bits(y, want, f"launch {k}: {op} {dt} exclusive={e}")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "i64"])
def test_two_streams(gpu, dt):
    n = 300 * tile_of(dt) + 1
    cases = [case(dt, "ramp", "max", n), case(dt, "decreasing", "min", n)]
    xs = [to_torch(x, gpu) for x, _ in cases]
    torch.cuda.synchronize(gpu)
    streams = [torch.cuda.Stream(gpu) for _ in range(2)]
    outs = []
    for xt, s, op in zip(xs, streams, OPS):
        with torch.cuda.stream(s):
            outs.append(scan(xt, algo="lookback", op=op))
    check_lookback(gpu)  # synchronises the device
    for (x, ref), y, op in zip(cases, outs, OPS):
        assert_same_bits(y, ref, f"{dt} {op} on its own stream")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ["f32", "i64"])
def test_graph_capture_of_a_max_scan(gpu, dt):
    """A max look-back scan captured into a HIP graph (epoch 0: the descriptors
    are zeroed inside the graph) and replayed on changed input, with an eager
    scan between the replays."""
    n = 70 * tile_of(dt) + 9
    xt = torch.zeros(n, dtype=TORCH[dt], device=gpu)
    out = torch.empty_like(xt)
    scan(xt, out=out, algo="lookback", op="max")  # warm-up outside the capture
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        scan(xt, out=out, algo="lookback", op="max")
    for pattern in ("ramp", "spike"):
        x, ref = case(dt, pattern, "max", n)
        xt.copy_(to_torch(x, gpu))
        graph.replay()
        torch.cuda.synchronize(gpu)
        assert_same_bits(out, ref, f"{dt} replay on {pattern}")
        assert_same_bits(scan(xt, algo="lookback", op="min"), oracle(x, "min"), f"{dt} eager between replays")
    check_lookback(gpu)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_auto_is_lookback_and_reproducible(dev):
    for dt in DTYPES:
        x, ref = case(dt, "ramp", "max", tile_of(dt) + 1)
        xt = to_torch(x, dev)
        assert_same_bits(scan(xt, op="max"), ref, f"{dt} auto")
        assert_same_bits(cummax(xt), ref, f"{dt} cummax")
    finish(dev)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_rejected_arguments(dev):
    x = torch.ones(100, dtype=torch.float32, device=dev)
    with pytest.raises(ValueError, match="op"):
        scan(x, op="prod")
    for algo in ("blelloch", "hillis", "blelloch_mlevel"):
        with pytest.raises(TypeError, match="rts.*lookback"):
            scan(x, algo=algo, op="max")
    with pytest.raises(TypeError, match="rts.*lookback"):
        cummin(x.to(torch.int64), algo="blelloch")
    with pytest.raises(ValueError, match="out"):
        scan(x, out=torch.empty(100, dtype=torch.int32, device=dev), op="max")
    with pytest.raises(ValueError, match="out"):
        cummax(x, out=torch.empty(99, dtype=torch.float32, device=dev))
    finish(dev)
