"""``ops.algorithms.bincount`` on both backends against ``numpy.bincount`` of
the in-range elements, exactly.

The oracle of ``bincount(x, nbins=K)`` is ``np.bincount(a[(a >= 0) & (a < K)],
minlength=K)`` on the elements widened to int64; the data-dependent form
(``nbins=None``) must also equal ``torch.bincount`` of the CPU copy.

Shapes are the smallest at which each mechanism of ``csrc/hip/bincount.hip``
can go wrong, and their edges come from ``bincount_launch_info``: ``V`` the
elements of a 16-byte lane vector, ``P`` the elements of one workgroup pass,
``W`` the bins of one LDS table, ``R`` the last bin count whose table is still
replicated. Lengths: 0, 1, ``V`` and ``P`` minus, exactly and plus one, three
grid strides under ``bincount_maxblocks=2``. Bin counts: 0, 1, 2, 255, 256, 257,
``R``, ``R + 1``, ``W - 1``, ``W``, ``W + 1`` (a second window of one bin), three
windows with a partial last one under ``bincount_window=64``, every regime
forced at 5 and 1000 bins. The CPU backend has no plan and no knobs: it runs
the same cases at fixed stand-ins, and its three forms are forced through
``BINCOUNT_CPU_PATH``. Nothing is above 2^20 elements.

The cases are the ``_case_*`` functions; ``test_counts`` and ``test_contract``
at the end run all of them on each backend (two GPU-marked ids, a few seconds
in all), so the suite's id count grows by a handful, not by seventy."""
import contextlib

import numpy as np
import pytest
import torch

import cme213x  # noqa: F401
from cme213x.ops import algorithms as alg
from cme213x.ops.algorithms import bincount, bincount_launch_info

NP = {"u8": np.uint8, "i32": np.int32, "i64": np.int64}
TORCH = {"u8": torch.uint8, "i32": torch.int32, "i64": torch.int64}
ALL = list(NP)
DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
CPU_PASS_VECTORS = 1024  # stand-ins of the CPU backend, which has no plan
CPU_W = 16384
CPU_R = 2047
REGIMES = {"lds": 1, "window": 2, "global": 3, "sorted": 4}


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
def edges(dev, dt: str) -> tuple[int, int, int, int]:
    """(V, P, W, R) of the backend."""
    v = 16 // np.dtype(NP[dt]).itemsize
    if dev.type != "cuda":
        return v, CPU_PASS_VECTORS * v, CPU_W, CPU_R
    info = bincount_launch_info(1 << 16, 16, dtype=TORCH[dt], device=dev)
    assert info["regime"] == "lds" and info["vector"] == v and info["pass"] % v == 0
    W = info["window"]
    lo, hi = 1, W  # copies falls with nbins: bisect the last nbins with more than one copy
    assert bincount_launch_info(1 << 16, lo, dtype=TORCH[dt], device=dev)["copies"] > 1
    assert bincount_launch_info(1 << 16, hi, dtype=TORCH[dt], device=dev)["copies"] == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if bincount_launch_info(1 << 16, mid, dtype=TORCH[dt], device=dev)["copies"] > 1:
            lo = mid
        else:
            hi = mid
    return v, info["pass"], W, lo


# ------------------------------------------------------------------ oracle
def oracle(a: np.ndarray, K: int) -> np.ndarray:
    w = a.astype(np.int64)
    return np.bincount(w[(w >= 0) & (w < K)], minlength=K).astype(np.int64)[:K]


def draw(dt: str, n: int, lo: int, hi: int, seed: int = 0) -> np.ndarray:
    """n values uniform in [lo, hi), clipped to the dtype's range."""
    ii = np.iinfo(NP[dt])
    lo, hi = max(lo, int(ii.min)), min(hi, int(ii.max) + 1)
    return np.random.default_rng(seed).integers(lo, max(hi, lo + 1), size=n, dtype=np.int64).astype(NP[dt])


def check(dev, a: np.ndarray, K: int, what: str = "", **kw) -> torch.Tensor:
    x = torch.from_numpy(a).to(dev)
    with knobs(dev, **kw):
        r = bincount(x, nbins=K)
    assert r.dtype == torch.int64 and tuple(r.shape) == (K,) and r.device == x.device, what
    got, want = r.cpu().numpy(), oracle(a, K)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"{what} {a.dtype} n={a.size} K={K} {kw}: bin {bad[:1]}: {got[bad[:1]]} != {want[bad[:1]]}"
    return r


# ------------------------------------------------------------------ lengths
def _case_lengths(dev, dt):
    V, P, W, R = edges(dev, dt)
    for n in (0, 1, V - 1, V, V + 1, P - 1, P, P + 1, P + V + 1):
        for K in (5, 300):
            check(dev, draw(dt, n, -2, K + 2, seed=n), K, "length")


def _case_three_grid_strides(dev, dt):
    V, P, W, R = edges(dev, dt)
    n = 2 * 3 * P - P // 2 + 3  # chunks 0 and 1 take three passes each, the last pass partial
    if dev.type == "cuda":
        with knobs(dev, bincount_maxblocks=2):
            assert bincount_launch_info(n, 300, dtype=TORCH[dt], device=dev)["chunks"] == 2
    for regime in (0, REGIMES["window"], REGIMES["global"]):
        check(dev, draw(dt, n, -2, 302, seed=7), 300, "grid stride", bincount_maxblocks=2, bincount_regime=regime)
    check(dev, draw(dt, n, -2, 200, seed=8), 150, "grid stride, windows", bincount_maxblocks=2, bincount_window=64)


# ------------------------------------------------------------------ bin counts
def _case_bin_counts(dev, dt):
    V, P, W, R = edges(dev, dt)
    if dev.type == "cuda":
        d = TORCH[dt]
        assert bincount_launch_info(3001, R, dtype=d, device=dev)["copies"] > 1
        assert bincount_launch_info(3001, R + 1, dtype=d, device=dev)["copies"] == 1
        assert bincount_launch_info(3001, W, dtype=d, device=dev)["regime"] == "lds"
        two = bincount_launch_info(3001, W + 1, dtype=d, device=dev)
        assert (two["regime"], two["windows"]) == ("window", 2)
    for K in (0, 1, 2, 255, 256, 257, R, R + 1, W - 1, W, W + 1):
        a = draw(dt, 3001, -1, K + 1, seed=K)
        if K:  # both ends of the table, and (W + 1: of each window) are present
            a[:6] = np.array([0, K - 1, min(K, W) - 1, min(K - 1, W), K, -1]).astype(NP[dt])
        check(dev, a, K, "bin count")


def _case_three_windows_last_partial(dev, dt):
    K, Wk = 2 * 64 + 10, 64
    if dev.type == "cuda":
        with knobs(dev, bincount_window=Wk):
            info = bincount_launch_info(5000, K, dtype=TORCH[dt], device=dev)
        assert (info["regime"], info["window"], info["windows"]) == ("window", Wk, 3)
    edge = [v for lo in (0, 64, 128) for v in (lo - 1, lo, lo + Wk - 1, lo + Wk)] + [K - 1, K]
    ii = np.iinfo(NP[dt])
    edge = [v for v in edge if ii.min <= v <= ii.max]
    a = np.array(edge * 300, dtype=np.int64).astype(NP[dt])  # every element on a window edge
    check(dev, a, K, "window edges", bincount_window=Wk)
    check(dev, np.sort(a), K, "window edges, sorted", bincount_window=Wk)
    check(dev, draw(dt, 5000, -3, K + 3), K, "three windows", bincount_window=Wk)


def _case_regimes_agree(dev, dt, K):
    a = draw(dt, 20011, -5, K + 5, seed=K)
    results = []
    for name, code in REGIMES.items():
        if name == "sorted" and dt == "u8" and dev.type == "cuda":
            with knobs(dev, bincount_regime=code), pytest.raises(ValueError):
                bincount(torch.from_numpy(a).to(dev), nbins=K)  # the sort takes no bytes: an error, not a fallback
            continue
        if dev.type == "cuda":
            with knobs(dev, bincount_regime=code):
                assert bincount_launch_info(a.size, K, dtype=TORCH[dt], device=dev)["regime"] == name
        results.append(check(dev, a, K, name, bincount_regime=code))
    for r in results[1:]:
        assert torch.equal(r, results[0])


@pytest.mark.parametrize("path", [1, 2, 3])
@pytest.mark.parametrize("dt", ALL)
def test_cpu_forms(dt, path, monkeypatch):
    """The serial, per-thread-table and partitioned-bin forms of the CPU backend."""
    monkeypatch.setattr(alg, "BINCOUNT_CPU_PATH", path)
    cpu = torch.device("cpu")
    for n, K in ((0, 4), (1, 1), (5000, 3), (5000, 300), (40000, 1), (40000, 70000)):
        check(cpu, draw(dt, n, -3, K + 3, seed=n + K), K, f"cpu form {path}")


# ------------------------------------------------------------------ views
def _case_views(dev, dt):
    V, P, W, R = edges(dev, dt)
    K = 200
    a = draw(dt, P + 3 * V + 5, 0, K + 2, seed=3)  # no negatives: the data-dependent form runs on the views too
    base = torch.from_numpy(a).to(dev)
    views = {"x[1:]": (base[1:], a[1:]), "x[3:]": (base[3:], a[3:]), "x[1:-2]": (base[1:-2], a[1:-2]),
             "ragged": (base[:P + V + 1], a[:P + V + 1]), "stride 2": (base[::2], a[::2]),
             "x[V-1:][::3]": (base[V - 1:][::3], a[V - 1:][::3])}
    for what, (x, ref) in views.items():
        for regime in (0, REGIMES["global"]):
            with knobs(dev, bincount_regime=regime):
                r = bincount(x, nbins=K)
            assert np.array_equal(r.cpu().numpy(), oracle(ref, K)), f"{what} {dt} regime {regime}"
        assert torch.equal(bincount(x).cpu(), torch.bincount(x.cpu())), what
    assert torch.equal(base, torch.from_numpy(a).to(dev))  # the operand is left alone


# ------------------------------------------------------------------ data
def _case_all_equal_is_exact(dev, dt):
    """Maximum contention: 2^20 elements of one value."""
    n = 1 << 20
    x = torch.full((n,), 3, dtype=TORCH[dt], device=dev)
    want = torch.tensor([0, 0, 0, n, 0, 0, 0, 0], dtype=torch.int64)
    for kw in ({}, {"bincount_regime": REGIMES["global"]}, {"bincount_regime": REGIMES["window"], "bincount_window": 2}):
        with knobs(dev, **kw):
            assert torch.equal(bincount(x, nbins=8).cpu(), want), kw
    assert torch.equal(bincount(x).cpu(), want[:4])


def _case_uniform_and_sorted(dev, dt):
    V, P, W, R = edges(dev, dt)
    for K in (256, 1000, 2 * W + 100, 33 * W):  # replicated table, one table, three windows, past the windows
        a = draw(dt, 50021, -K // 8, K + K // 8, seed=K)
        check(dev, a, K, "uniform")
        check(dev, np.sort(a), K, "sorted")
        check(dev, np.sort(a)[::-1].copy(), K, "descending")


def _case_out_of_range_is_not_counted(dev, dt):
    ii = np.iinfo(NP[dt])
    for K in (8, 100, 300):
        vals = [-1, -2, K, K - 1, K + 1, 0, 1, int(ii.min), int(ii.max), int(ii.max) - 1, int(ii.min) + 1]
        vals = [v for v in vals if ii.min <= v <= ii.max]
        a = np.array(vals * 37, dtype=np.int64).astype(NP[dt])
        for regime in (0, REGIMES["window"], REGIMES["global"]):
            check(dev, a, K, "range", bincount_regime=regime)
            check(dev, a, K, "range, narrow windows", bincount_regime=regime, bincount_window=3)


def _case_int64_is_compared_before_narrowing(dev):
    """2^32 + j and -2^32 + j are not bin j."""
    js = np.arange(-3, 12, dtype=np.int64)
    a = np.concatenate([2 ** 32 + js, -2 ** 32 + js, 2 ** 40 + js, 2 ** 63 - 1 - js[3:], js, js[5:]]).astype(np.int64)
    a = np.tile(a, 11)
    for K in (8, 300):
        for name in REGIMES:
            r = check(dev, a, K, "wide " + name, bincount_regime=REGIMES[name])
            assert int(r.sum()) == int(((a >= 0) & (a < K)).sum())
    check(dev, a, 70000, "wide, windows")


def _case_uint8_top_value(dev):
    a = draw("u8", 4099, 0, 256, seed=5)
    a[:9] = 255
    r255, r256 = check(dev, a, 255, "u8 255"), check(dev, a, 256, "u8 256")
    assert int(r256[255]) == int((a == 255).sum()) >= 9 and torch.equal(r255, r256[:255])
    full = bincount(torch.from_numpy(a).to(dev))
    assert full.numel() == 256 and torch.equal(full, r256)


# ------------------------------------------------------------------ the data-dependent form
def _case_matches_torch_bincount(dev, dt):
    for n, hi, seed in ((1, 1, 0), (17, 3, 1), (5003, 200, 2), (5003, 256, 3), (70001, 40000, 4)):
        a = draw(dt, n, 0, hi, seed=seed)
        x = torch.from_numpy(a).to(dev)
        top = int(a.max()) + 1
        for minlength in (0, 1, top - 1, top, top + 1, 300):
            r = bincount(x, minlength=minlength)
            want = np.bincount(a.astype(np.int64), minlength=minlength)
            assert r.dtype == torch.int64 and r.device == x.device
            assert np.array_equal(r.cpu().numpy(), want), (dt, n, hi, minlength)
            assert torch.equal(r.cpu(), torch.bincount(x.cpu(), minlength=minlength))


def _case_empty_input(dev, dt):
    x = torch.empty(0, dtype=TORCH[dt], device=dev)
    for r, k in ((bincount(x, minlength=7), 7), (bincount(x), 0), (bincount(x, nbins=5), 5), (bincount(x, nbins=0), 0)):
        assert r.dtype == torch.int64 and r.device == x.device and tuple(r.shape) == (k,) and not r.any()


def _case_negative_element_raises(dev, dt):
    x = torch.tensor([3, 1, -1, 2], dtype=TORCH[dt], device=dev)
    with pytest.raises(ValueError, match="negative"):
        bincount(x)
    with pytest.raises(ValueError, match="negative"):
        bincount(x, minlength=9)
    assert bincount(x, nbins=4).tolist() == [0, 1, 1, 1]


# ------------------------------------------------------------------ contract
def _case_out_is_overwritten_and_returned(dev, dt):
    a = draw(dt, 3000, -2, 60, seed=9)
    x = torch.from_numpy(a).to(dev)
    for K in (0, 1, 50):
        out = torch.full((K,), -(2 ** 62) + 12345, dtype=torch.int64, device=dev)
        for regime in REGIMES.values():
            if regime == REGIMES["sorted"] and dt == "u8":
                continue
            out.fill_(-(2 ** 62) + 12345)
            with knobs(dev, bincount_regime=regime):
                r = bincount(x, nbins=K, out=out)
            assert r is out and np.array_equal(out.cpu().numpy(), oracle(a, K)), (K, regime)
    big = torch.full((64,), 77, dtype=torch.int64, device=dev)
    r = bincount(x, nbins=50, out=big[7:57])  # a view: its neighbours stay
    assert np.array_equal(r.cpu().numpy(), oracle(a, 50))
    assert (big[:7] == 77).all() and (big[57:] == 77).all()


def _case_bad_out(dev):
    x = torch.arange(10, dtype=torch.int32, device=dev)
    with pytest.raises(TypeError):
        bincount(x, nbins=10, out=torch.zeros(10, dtype=torch.int32, device=dev))
    with pytest.raises(TypeError):
        bincount(x, nbins=10, out=[0] * 10)
    with pytest.raises(ValueError):
        bincount(x, nbins=10, out=torch.zeros(11, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        bincount(x, nbins=10, out=torch.zeros(2, 5, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        bincount(x, nbins=10, out=torch.zeros(20, dtype=torch.int64, device=dev)[::2])
    with pytest.raises(ValueError):
        bincount(x, nbins=10, out=torch.zeros(10, dtype=torch.int64, device="meta"))
    with pytest.raises(ValueError):
        bincount(x, out=torch.zeros(10, dtype=torch.int64, device=dev))  # out= needs nbins


def _case_bad_arguments(dev):
    x = torch.arange(10, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        bincount(x, minlength=3, nbins=10)
    for bad in (-1, 2.0, True, "8"):
        with pytest.raises(ValueError):
            bincount(x, nbins=bad)
    with pytest.raises(ValueError):
        bincount(x, minlength=-1)
    for d in (torch.float32, torch.float64, torch.bool, torch.int16, torch.int8, torch.uint32, torch.float16):
        with pytest.raises(TypeError, match="uint8, int32, int64"):
            bincount(torch.zeros(4, device=dev).to(d), nbins=4)
        with pytest.raises(TypeError, match="uint8, int32, int64"):
            bincount(torch.zeros(4, device=dev).to(d))
    for shape in ((), (2, 5), (1, 10), (0, 3)):
        with pytest.raises(ValueError):
            bincount(torch.zeros(shape, dtype=torch.int64, device=dev), nbins=4)
    with pytest.raises(TypeError):
        bincount_launch_info(10, 10, dtype=torch.int16, device=dev)


def _case_forced_regime_that_cannot_run(gpu, dt):
    """More bins than one table holds under a forced ``lds`` is an error, not a fallback."""
    V, P, W, R = edges(gpu, dt)
    x = torch.zeros(100, dtype=TORCH[dt], device=gpu)
    with knobs(gpu, bincount_regime=REGIMES["lds"]):
        assert bincount(x, nbins=W).tolist()[0] == 100
        with pytest.raises(ValueError):
            bincount(x, nbins=W + 1)
        with pytest.raises(ValueError):
            bincount_launch_info(100, W + 1, dtype=TORCH[dt], device=gpu)
    with knobs(gpu, bincount_regime=REGIMES["lds"], bincount_window=64):
        assert bincount(x, nbins=64).tolist()[0] == 100
        with pytest.raises(ValueError):
            bincount(x, nbins=65)
    with knobs(gpu, bincount_regime=9), pytest.raises(ValueError):
        bincount(x, nbins=5)


# ------------------------------------------------------------------ the plan
def test_launch_info_cpu():
    d = bincount_launch_info(1000, 10, dtype=torch.int32, device="cpu")
    assert (d["regime"], d["vector"], d["workgroups"]) == ("cpu", 4, 0)
    assert bincount_launch_info(1000, 10, dtype=torch.uint8, device="cpu")["vector"] == 16
    assert bincount_launch_info(1000, 10, device="cpu")["vector"] == 2


def _case_launch_info_gpu(gpu, dt):
    d = TORCH[dt]
    V, P, W, R = edges(gpu, dt)
    one = bincount_launch_info(10 * P, 256, dtype=d, device=gpu)
    assert (one["regime"], one["windows"], one["chunks"], one["workgroups"]) == ("lds", 1, 10, 10)
    assert one["copies"] > 1 and one["copies"] & (one["copies"] - 1) == 0
    assert one["copies"] * 257 * 4 == one["lds_bytes"] <= 65536 and one["threads"] == 256
    full = bincount_launch_info(10 * P, W, dtype=d, device=gpu)
    assert (full["copies"], full["lds_bytes"]) == (1, 4 * W) and full["lds_bytes"] <= 65536
    win = bincount_launch_info(10 * P, 3 * W - 1, dtype=d, device=gpu)
    assert (win["regime"], win["windows"], win["workgroups"]) == ("window", 3, 30)
    far = bincount_launch_info(10 * P, 1 << 30, dtype=d, device=gpu)
    assert far["regime"] in ("global", "sorted") and far["lds_bytes"] == 0
    assert bincount_launch_info(0, 256, dtype=d, device=gpu)["workgroups"] == 0
    assert bincount_launch_info(10 * P, 0, dtype=d, device=gpu)["workgroups"] == 0
    # a workgroup's share stays below 2^32 elements whatever the grid cap
    with knobs(gpu, bincount_maxblocks=1):
        huge = bincount_launch_info(2 ** 35, 256, dtype=d, device=gpu)
        assert huge["chunks"] >= 2 ** 35 // 2 ** 31 and 2 ** 35 / huge["chunks"] + 2 * P + 32 < 2 ** 32
        assert bincount_launch_info(10 * P, 256, dtype=d, device=gpu)["chunks"] == 1


# ------------------------------------------------------------------ the tests
# The cases above run from two tests per backend: a GPU case costs
# milliseconds, and one id each would add some seventy GPU-marked ids to the
# suite. A failure names its case, dtype, length, bin count and knobs.
PER_DTYPE = (_case_lengths, _case_three_grid_strides, _case_bin_counts, _case_three_windows_last_partial, _case_views,
             _case_all_equal_is_exact, _case_uniform_and_sorted, _case_out_of_range_is_not_counted,
             _case_matches_torch_bincount, _case_empty_input)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_counts(dev):
    """Every length, bin-count, regime, view and data case, for every dtype."""
    for dt in ALL:
        for case in PER_DTYPE:
            case(dev, dt)
        for K in (5, 1000):
            _case_regimes_agree(dev, dt, K)
    _case_int64_is_compared_before_narrowing(dev)
    _case_uint8_top_value(dev)
    for dt in ("i32", "i64"):
        _case_negative_element_raises(dev, dt)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_contract(dev):
    """``out=``, rejected arguments, a forced regime that cannot run, the launch plan."""
    for dt in ALL:
        _case_out_is_overwritten_and_returned(dev, dt)
    _case_bad_out(dev)
    _case_bad_arguments(dev)
    if dev.type == "cuda":
        for dt in ALL:
            _case_forced_regime_that_cannot_run(dev, dt)
            _case_launch_info_gpu(dev, dt)
