"""The Thrust-equivalent layer (ops/algorithms.py) at its edges, against
oracles that share no code with it.

Every case runs on the CPU backend (unmarked) and on the GPU; the select
family runs on the GPU under both ``SELECT_ALGO`` arms. The oracles
(``alg_util.py``) are numpy in the native integer dtype or on bit patterns:
select, unique and remove compare bits (so -0.0 != 0.0 and two NaNs are equal
iff their bits are), search is numeric (``numpy.searchsorted`` in the native
dtype; NaN keys are out of scope), arg-reduce skips NaN.

Tolerances: every comparison is exact except
* the float32 segment sums of non-representable values: against a float64 sum
  under ``(len - 1) * 2^-24 * sum |v|`` per segment, the bound of any
  summation order;
* ``inner_product(op="mul")``: products of two float32 are exact in float64,
  so kernel and float64 reference differ by summation rounding only:
  ``2 * n * 2^-53 * sum |a b|``.
"""
import math

import numpy as np
import pytest
import torch

import cme213x  # noqa: F401
from cme213x.ops import algorithms as A
from alg_util import (BIG, CPU, T, TILE_SIZES, assert_exact_sums, bits, bitwise_specials, cached, flag_mask, from_bits,
                      from_ids, gen, head_mask, nan_bits, ora_indices, ora_partition, ora_search, ora_segments,
                      ora_values, rand_data, run_ids, scalar_bits, search_keys, search_queries, to_numpy, to_torch,
                      view_of, NP)

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
# (device, SELECT_ALGO): reduce-then-scan and the single-pass look-back
ARMS = [pytest.param(("cpu", "rts"), id="cpu"), pytest.param(("gpu", "rts"), marks=pytest.mark.gpu, id="gpu-rts"),
        pytest.param(("gpu", "lookback"), marks=pytest.mark.gpu, id="gpu-lookback")]

SEL_DT = [torch.uint8, torch.int32, torch.float32, torch.int64, torch.float64]
RED_DT = [torch.int32, torch.int64, torch.float32, torch.float64]
SEARCH_DT = [torch.uint32, torch.int32, torch.int64, torch.float32, torch.float64]
N_PAT = 2 * T + 17
B = 2048 * 256  # kArgBlocks * kThreads: above it arg_partial_kernel walks more than one item per lane


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return CPU


@pytest.fixture
def arm(request, monkeypatch):
    name, algo = request.param
    monkeypatch.setattr(A, "SELECT_ALGO", algo)
    if name == "cpu":
        yield CPU
        return
    device = request.getfixturevalue("gpu")
    yield device
    from cme213x.ops.scan import lookback_timed_out
    assert not lookback_timed_out(device)


def _eq(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Same dtype width, length and bits."""
    g = bits(got)
    assert g.dtype == want.dtype and g.shape == want.shape, (what, g.dtype, want.dtype, g.shape, want.shape)
    bad = torch.nonzero(g != want).view(-1)
    assert bad.numel() == 0, f"{what}: {bad.numel()} elements differ, first at {int(bad[0])}"


# =================================================================== select
def _check_flags(x: torch.Tensor, fl: torch.Tensor, device, xd=None, fd=None) -> None:
    """copy_if (and inverted), nonzero, stable_partition and split of CPU
    ``x`` / ``fl`` on ``device`` (``xd`` / ``fd``: the device operands, when
    the caller built views) against the bit-pattern oracle."""
    xd = x.to(device) if xd is None else xd
    fd = fl.to(device) if fd is None else fd
    n = x.numel()
    m = flag_mask(fl)
    _eq(A.copy_if(xd, fd), ora_values(x, m), "copy_if")
    _eq(A.copy_if(xd, fd, invert=True), ora_values(x, ~m), "copy_if invert")
    got = A.nonzero(fd)
    assert got.dtype == torch.int64
    _eq(got, ora_indices(m), "nonzero")
    for f, mm, what in ((A.stable_partition, m, "stable_partition"), (A.split, ~m, "split")):
        p, c = f(xd, fd)
        want, cw = ora_partition(x, mm)
        assert c == cw and p.numel() == n and p.dtype == x.dtype, what
        _eq(p, want, what)
    _eq(xd, bits(x), "x untouched")
    _eq(fd, bits(fl), "flags untouched")


def _check_heads(x: torch.Tensor, device, xd=None, values=()) -> None:
    """unique, run_starts and remove_value of CPU ``x`` on ``device``."""
    xd = x.to(device) if xd is None else xd
    xb = bits(x).numpy()
    h = head_mask(xb)
    got = A.unique(xd)
    assert got.dtype == x.dtype
    _eq(got, ora_values(x, h), "unique")
    got = A.run_starts(xd)
    assert got.dtype == torch.int64
    _eq(got, ora_indices(h), "run_starts")
    for v in values:
        _eq(A.remove_value(xd, v), ora_values(x, xb != xb.dtype.type(scalar_bits(x, v))), f"remove_value {v!r}")
    _eq(xd, bits(x), "x untouched")


def _sel_data(dtype, n):
    def make():
        g = gen(1000 + n % 9973)
        x = rand_data(dtype, n, g)
        fl = torch.rand(n, generator=g) < 0.5
        runs = from_ids(run_ids(n, g), dtype)
        return x, fl, runs
    return cached(("sel", dtype, n), make)


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("dtype", SEL_DT, ids=str)
@pytest.mark.parametrize("n", TILE_SIZES + [BIG])
def test_select_sizes(arm, dtype, n):
    """Tile-edge sizes and one multi-round size; flags at p = 0.5; random
    runs for the head predicate; n = 0 gives empty outputs and count 0."""
    x, fl, runs = _sel_data(dtype, n)
    _check_flags(x, fl, arm)
    _check_heads(runs, arm, values=[runs[n // 2].item()] if n else [0])
    if n == 0:
        xd, fd = x.to(arm), fl.to(arm)
        for out in (A.copy_if(xd, fd), A.nonzero(fd), A.unique(xd), A.run_starts(xd), A.remove_value(xd, 0)):
            assert out.numel() == 0
        assert A.stable_partition(xd, fd)[1] == 0 and A.split(xd, fd)[1] == 0


def _density(name: str, n: int) -> torch.Tensor:
    g = gen(7)
    if name == "none":
        return torch.zeros(n, dtype=torch.bool)
    if name == "all":
        return torch.ones(n, dtype=torch.bool)
    if name == "half":
        return torch.rand(n, generator=g) < 0.5
    fl = torch.rand(n, generator=g) < 0.5  # "tiles": tile 0 all set, tile 1 all clear (tile_sel = T and 0)
    fl[:T] = True
    fl[T:2 * T] = False
    return fl


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("dtype", SEL_DT, ids=str)
@pytest.mark.parametrize("density", ["none", "all", "half", "tiles"])
def test_select_flag_densities(arm, dtype, density):
    x = rand_data(dtype, N_PAT, gen(11))
    fl = _density(density, N_PAT)
    _check_flags(x, fl, arm)
    bytes_ = torch.tensor([1, 2, 0x80, 0xFF], dtype=torch.uint8)[torch.randint(0, 4, (N_PAT,), generator=gen(12))]
    _check_flags(x, torch.where(fl, bytes_, torch.zeros_like(bytes_)), arm)  # uint8 flags: any non-zero byte


def _wide_flags(kind: str, n: int) -> torch.Tensor:
    """Flags whose low byte is zero (int) or that are no integers (float)."""
    g = gen(13)
    pick = torch.randint(0, 6, (n,), generator=g)
    if kind == "int32":
        return torch.tensor([0, 256, 512, -1, 1, 0], dtype=torch.int32)[pick]
    if kind == "int64":
        return torch.tensor([0, 256, 2 ** 32, -1, 1, -2 ** 63], dtype=torch.int64)[pick]
    if kind == "float32":
        return torch.tensor([0.0, 0.5, -0.25, 1.0, -0.0, 1e-30], dtype=torch.float32)[pick]
    return torch.tensor([0.0, 0.5, -0.25, 1.0, -0.0, 1e-300], dtype=torch.float64)[pick]


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("kind", ["int32", "int64", "float32", "float64"])
def test_select_wide_flags(arm, kind):
    """A flag of any dtype is set iff it is != 0: 256, 512 and -1 (a zero low
    byte, or all ones), 0.5 and -0.25 (zero after truncation), -0.0 (clear)."""
    assert A.nonzero(torch.tensor([0, 256, 1, 512, 0, -1], dtype=torch.int32).to(arm)).tolist() == [1, 2, 3, 5]
    x4 = torch.tensor([10, 11, 12, 13], dtype=torch.int32).to(arm)
    assert A.copy_if(x4, torch.tensor([0.0, 0.5, 1.0, -0.25]).to(arm)).tolist() == [11, 12, 13]
    for dtype in (torch.int32, torch.float64):
        x = rand_data(dtype, N_PAT, gen(14))
        _check_flags(x, _wide_flags(kind, N_PAT), arm)


def _head_ids(name: str) -> torch.Tensor:
    n = N_PAT
    i = torch.arange(n, dtype=torch.int64)
    if name == "all_equal":
        return torch.full((n,), 5, dtype=torch.int64)
    if name == "all_distinct":
        return i
    if name == "boundary_at_T":  # two runs; the second starts exactly at T
        return (i >= T).to(torch.int64)
    if name == "run_spans_T":  # distinct items, but for one run over [T - 5, T + 5)
        ids = i.clone()
        ids[T - 5:T + 5] = T - 5
        return ids
    if name == "run_spans_T_pair":  # the shortest such run: T - 1 | T
        ids = i.clone()
        ids[T] = T - 1
        return ids
    if name == "thread_edges":  # runs of 16 that start at 8 mod 16: every one crosses a thread's 16 items
        return (i + 8) // 16
    if name == "thread_aligned":  # runs of 16 on the thread boundaries: every head is a thread's first item
        return i // 16
    raise KeyError(name)


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("dtype", SEL_DT, ids=str)
@pytest.mark.parametrize("name", ["all_equal", "all_distinct", "boundary_at_T", "run_spans_T", "run_spans_T_pair",
                                  "thread_edges", "thread_aligned"])
def test_select_head_predicate(arm, dtype, name):
    x = from_ids(_head_ids(name), dtype)
    _check_heads(x, arm, values=[x[0].item(), x[T].item()])
    if name == "all_equal":
        assert A.unique(x.to(arm)).numel() == 1 and A.remove_value(x.to(arm), x[0].item()).numel() == 0


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_select_bitwise_semantics(arm, dtype):
    """0.0 / -0.0, NaNs of equal bits and NaNs of different payloads at the
    start, across the tile boundary T and at the end: unique, run_starts and
    remove_value compare bit patterns."""
    sp = bitwise_specials(dtype)
    lit = torch.tensor([0.0, -0.0, -0.0, math.nan, math.nan, 1.0], dtype=dtype).to(arm)
    got = A.unique(lit).cpu()
    assert got.numel() == 4 and torch.equal(got.isnan(), torch.tensor([False, False, True, False]))
    assert math.copysign(1.0, got[0].item()) == 1.0 and math.copysign(1.0, got[1].item()) == -1.0
    x = torch.ones(N_PAT, dtype=dtype)
    for at in (0, T - 7, N_PAT - sp.numel()):
        x[at:at + sp.numel()] = sp
    _check_heads(x, arm, values=[0.0, -0.0, math.nan, 1.0])
    a, b, c = bits(from_bits(torch.tensor(nan_bits(dtype), dtype=torch.int64), dtype)).tolist()
    kept = bits(A.remove_value(x.to(arm), math.nan))
    assert not bool((kept == a).any()) and bool((kept == b).any()) and bool((kept == c).any())
    _check_flags(x, x != x, arm)  # NaNs compacted as they are


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("dtype", SEL_DT, ids=str)
@pytest.mark.parametrize("n", [N_PAT, BIG])
@pytest.mark.parametrize("mis", ["flags", "x", "both"])
def test_select_misaligned_views(arm, dtype, n, mis):
    """``big[1:1+n]``: 1, 4 or 8 bytes past a 16-byte boundary, so full tiles
    take the guarded scalar path instead of 16-byte vector loads; values,
    indices and partition."""
    x, fl, runs = _sel_data(dtype, n)
    xd = view_of(x, 1 if mis in ("x", "both") else 0, arm)
    fd = view_of(fl, 1 if mis in ("flags", "both") else 0, arm)
    _check_flags(x, fl, arm, xd, fd)
    if mis != "flags":
        _check_heads(runs, arm, view_of(runs, 1, arm), values=[runs[n // 2].item()])


# =================================================================== search
def _S(dtype) -> int:  # splitters of search2_kernel
    return 4096 if dtype in (torch.uint32, torch.int32, torch.float32) else 2048


def _search_case(dtype, n, m):
    def make():
        g = gen(2000 + n % 9973)
        keys = search_keys(dtype, n, g)
        q = search_queries(keys, m, g)
        return keys, q, ora_search(keys, q, False), ora_search(keys, q, True)
    return cached(("search", dtype, n, m), make)


def _check_search(keys, q, lo, hi, device):
    kd, qd = to_torch(keys).to(device), to_torch(q).to(device)
    got = A.lower_bound(kd, qd)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), lo)
    assert torch.equal(A.upper_bound(kd, qd).cpu(), hi)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", SEARCH_DT, ids=str)
@pytest.mark.parametrize("case", ["0", "1", "2", "1000", "1000xgrid", "16S-1", "16S", "16S+1", "200001"])
def test_search(dev, dtype, case):
    """Full-width keys (no NaN: out of scope), every key, its two neighbours
    and the ends of the range as queries. Lengths around the two-level
    threshold n >= 16 S with query counts on either side of its m >= 64 S
    (S splitters: 4096 for 4-byte, 2048 for 8-byte keys); 600 001 queries into 1000
    keys send the one-level kernel (a grid of at most 8 * 256 CUs blocks of
    256, stream_grid / kNumCU in common.h) round its grid-stride loop."""
    S = _S(dtype)
    n = {"0": 0, "1": 1, "2": 2, "1000": 1000, "1000xgrid": 1000, "16S-1": 16 * S - 1, "16S": 16 * S,
         "16S+1": 16 * S + 1, "200001": 200_001}[case]
    if case == "1000xgrid":
        ms = [600_001]
    elif n >= 16 * S - 1:
        ms = [64 * S - 1, 64 * S]
    else:
        ms = [None]
    for m in ms:
        _check_search(*_search_case(dtype, n, m), dev)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", SEARCH_DT, ids=str)
def test_search_all_equal(dev, dtype):
    """Every splitter equal: the query equal to the key, below and above it."""
    S = _S(dtype)
    npdt = NP[dtype]
    key = {torch.uint32: 3_000_000_000, torch.int32: -7, torch.int64: -2 ** 60 + 5, torch.float32: -0.0,
           torch.float64: 1.0 + 2.0 ** -52}[dtype]
    keys = np.full(16 * S + 5, key, dtype=npdt)
    if npdt(0).dtype.kind == "f":
        three = np.array([key, np.nextafter(npdt(key), npdt(-np.inf)), np.nextafter(npdt(key), npdt(np.inf)), 0.0],
                         dtype=npdt)
    else:
        three = np.array([key, key - 1, key + 1], dtype=npdt)
    for m in (three.size, 64 * S):
        q = np.resize(three, m)
        _check_search(keys, q, ora_search(keys, q, False), ora_search(keys, q, True), dev)


# ======================================================= segment reduce
def _small_ints(dtype, n, g) -> np.ndarray:
    return torch.randint(-50, 51, (n,), generator=g, dtype=torch.int64).numpy().astype(NP[dtype])


def _edge_offsets() -> np.ndarray:
    """offsets[0] = 5; empty segments at the start, in the middle and at the
    end; lengths 1, 63, 64, 65 (the wave is 64 lanes) and 100 000."""
    lens = [0, 0, 1, 63, 64, 65, 0, 100_000, 1, 0, 2, 64, 0, 0]
    return np.concatenate([[5], 5 + np.cumsum(lens)]).astype(np.int64)


def _many_offsets() -> np.ndarray:
    """40 000 segments of 0..8 items: more than the 8 * 256 CUs * 4 waves of
    the largest grid (stream_grid and kNumCU in csrc/include/cme213/common.h;
    one wave per segment), so every wave goes round its grid-stride loop."""
    lens = torch.randint(0, 9, (40_000,), generator=gen(31)).numpy()
    return np.concatenate([[3], 3 + np.cumsum(lens)]).astype(np.int64)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", RED_DT, ids=str)
@pytest.mark.parametrize("layout", ["edges", "many"])
def test_segment_reduce(dev, dtype, layout):
    off = _edge_offsets() if layout == "edges" else _many_offsets()
    v = _small_ints(dtype, int(off[-1]) + 7, gen(32))  # items before offsets[0] and after offsets[-1] stay out
    assert_exact_sums(v, off)
    vd, od = torch.from_numpy(v).to(dev), torch.from_numpy(off).to(dev)
    for op in ("sum", "max", "min"):
        got = A.segment_reduce(vd, od, op)
        assert got.dtype == dtype and got.device == vd.device
        want = ora_segments(v, off, op)
        assert np.array_equal(to_numpy(got), want), (op, np.flatnonzero(to_numpy(got) != want)[:5])
    # one-signed data: a zero accumulator instead of the identity would show
    for op, sign in (("max", -1), ("min", 1)):
        w = (sign * (np.abs(v) + 1)).astype(v.dtype)
        got = A.segment_reduce(torch.from_numpy(w).to(dev), od, op)
        assert np.array_equal(to_numpy(got), ora_segments(w, off, op)), op
    assert torch.equal(od.cpu(), torch.from_numpy(off))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_segment_reduce_int_wrap(dev):
    """int32 sums that leave the range wrap like numpy's; int64 values beyond
    2^53 add exactly."""
    off = _edge_offsets()
    g = gen(33)
    v32 = torch.randint(2 ** 30, 2 ** 31, (int(off[-1]),), generator=g, dtype=torch.int64).numpy().astype(np.int32)
    want = ora_segments(v32, off, "sum")
    assert np.array_equal(want[2:6], [np.add.reduce(v32[a:b], dtype=np.int32) for a, b in zip(off[2:6], off[3:7])])
    assert want[7] != np.add.reduce(v32[off[7]:off[8]], dtype=np.int64)  # it did wrap
    got = A.segment_reduce(torch.from_numpy(v32).to(dev), torch.from_numpy(off).to(dev), "sum")
    assert np.array_equal(to_numpy(got), want)
    v64 = torch.randint(-2 ** 62, 2 ** 62, (int(off[-1]),), generator=g, dtype=torch.int64).numpy()
    for op in ("sum", "max", "min"):
        got = A.segment_reduce(torch.from_numpy(v64).to(dev), torch.from_numpy(off).to(dev), op)
        assert np.array_equal(to_numpy(got), ora_segments(v64, off, op)), op


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("layout", ["edges", "many"])
def test_segment_reduce_float32_rounding(dev, layout):
    """uniform(0.5, 1) float32 values (no short binary expansion): every
    segment sum within (len - 1) * 2^-24 * sum |v| of the float64 sum."""
    off = _edge_offsets() if layout == "edges" else _many_offsets()
    v = (0.5 + 0.5 * torch.rand(int(off[-1]), generator=gen(34), dtype=torch.float64)).to(torch.float32).numpy()
    ref = ora_segments(v, off, "sum", wide=np.float64)
    bound = np.maximum(np.diff(off) - 1, 0) * 2.0 ** -24 * ora_segments(np.abs(v), off, "sum", wide=np.float64)
    got = to_numpy(A.segment_reduce(torch.from_numpy(v).to(dev), torch.from_numpy(off).to(dev), "sum"))
    err = np.abs(got.astype(np.float64) - ref)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"segment {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e}"


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("kdtype", [torch.int32, torch.int64, torch.float64], ids=str)
@pytest.mark.parametrize("vdtype", RED_DT, ids=str)
def test_reduce_by_key(dev, kdtype, vdtype):
    """Runs that cross the tile boundaries of the head-flag select (one over
    T - 1 | T, one that starts exactly at 2 T); int64 values of magnitude
    2^40 reduce exactly."""
    n = N_PAT
    g = gen(35)
    ids = run_ids(n, g, 0.05)
    ids[T - 1:T + 1] = ids[T - 1]
    ids[2 * T:] += 1 - (ids[2 * T] - ids[2 * T - 1])  # a head at 2 T
    ids = torch.cummax(ids, 0).values
    keys = from_ids(ids, kdtype)
    if vdtype == torch.int64:
        v = torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64).numpy()
    else:
        v = _small_ints(vdtype, n, g)
    starts = np.flatnonzero(head_mask(bits(keys).numpy()))
    assert T not in starts and 2 * T in starts
    off = np.append(starts, n).astype(np.int64)
    assert_exact_sums(v, off)
    for op in ("sum", "max", "min"):
        k, r = A.reduce_by_key(keys.to(dev), torch.from_numpy(v).to(dev), op)
        _eq(k, bits(keys)[torch.from_numpy(starts)], "keys")
        assert r.dtype == vdtype and np.array_equal(to_numpy(r), ora_segments(v, off, op)), op


# ================================================================ arg-reduce
def _ora_arg(x: np.ndarray, is_max: bool):
    """(extremum, its first index) of the non-NaN elements; all NaN: (nan, 0)."""
    ok = np.flatnonzero(~np.isnan(x)) if x.dtype.kind == "f" else np.arange(x.size)
    if ok.size == 0:
        return math.nan, 0
    y = x[ok]
    j = int(np.argmax(y) if is_max else np.argmin(y))  # numpy: the first occurrence
    return y[j].item(), int(ok[j])


def _check_arg(x: np.ndarray, device, is_max: bool) -> None:
    f = A.max_element if is_max else A.min_element
    val, idx = f(torch.from_numpy(x).to(device))
    wv, wi = _ora_arg(x, is_max)
    assert idx == wi, (idx, wi, val, wv)
    if isinstance(wv, float) and math.isnan(wv):
        assert math.isnan(val)
    else:
        assert val == wv and type(val) is type(wv)
        if isinstance(wv, float):
            assert math.copysign(1.0, val) == math.copysign(1.0, wv)  # the first of -0.0 / 0.0 as it is


def _one_signed(dtype, n, is_max: bool, g) -> np.ndarray:
    """All negative for max, all positive for min (a zero start value of the
    accumulator would win), magnitudes in [10, 1000]; int64 beyond 2^40."""
    mag = torch.randint(10, 1001, (n,), generator=g, dtype=torch.int64)
    if dtype == torch.int64:
        mag = mag + 2 ** 40
    return ((-mag if is_max else mag).numpy()).astype(NP[dtype])


ARG_SIZES = [1, 63, 64, 65, 255, 256, 257, B - 1, B, B + 1, 4 * B - 1, 4 * B, 4 * B + 1]


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", RED_DT, ids=str)
@pytest.mark.parametrize("n", ARG_SIZES)
def test_arg_reduce_sizes_and_placement(dev, dtype, n):
    """Below B one item per lane; above it lanes stride by B through a
    4x-unrolled loop and a tail. The extremum at the last index only, at index
    0 with duplicates later, everywhere, and tied between an item of the
    unrolled loop and one of the tail (n - 1 - B and n - 1 at n = 4 B + 1)."""
    for is_max in (True, False):
        base = cached(("arg", dtype, n, is_max), lambda: _one_signed(dtype, n, is_max, gen(40 + n % 97)))
        best = base.dtype.type(-5 if is_max else 5)
        _check_arg(base, dev, is_max)
        x = base.copy()
        x[-1] = best
        _check_arg(x, dev, is_max)
        x[n // 2] = best
        x[0] = best
        _check_arg(x, dev, is_max)
        x = base.copy()
        for at in (n - 1, n - 1 - B, n - 1 - 2 * B, 1):
            if 0 <= at < n:
                x[at] = best
        _check_arg(x, dev, is_max)
        _check_arg(np.full(n, base[0], dtype=base.dtype), dev, is_max)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
@pytest.mark.parametrize("n", [3, 65, 257, B + 1, 4 * B + 1])
def test_arg_reduce_nan(dev, dtype, n):
    """NaN never wins and never hides a value: the result is that of the
    array without its NaNs, the index mapped back. NaN at index 0, 64, 256,
    at multiples of the lane stride B and at the last index, one at a time and
    all together; next to the extremum; everywhere: (nan, 0)."""
    spots = [p for p in (0, 1, 64, 256, B, 2 * B, n - 1) if p < n]
    for is_max in (True, False):
        base = cached(("argnan", dtype, n, is_max), lambda: _one_signed(dtype, n, is_max, gen(50 + n % 97)))
        for where in [[p] for p in spots] + [spots]:
            x = base.copy()
            x[where] = np.nan
            _check_arg(x, dev, is_max)
        x = base.copy()
        x[n // 2] = -5 if is_max else 5  # the extremum between two NaNs
        x[[n // 2 - 1, min(n // 2 + 1, n - 1)]] = np.nan
        if n == 3:
            x[1] = -5 if is_max else 5
        _check_arg(x, dev, is_max)
        if n <= B + 1:
            _check_arg(np.full(n, np.nan, dtype=base.dtype), dev, is_max)
            x = np.full(n, np.nan, dtype=base.dtype)
            x[-1] = 7.0  # one value behind n - 1 NaNs
            _check_arg(x, dev, is_max)
    nan = math.nan
    for lit, want in (([nan, 1.0, 2.0], (2.0, 2)), ([1.0, nan, 2.0], (2.0, 2)), ([2.0, 1.0, nan], (2.0, 0))):
        assert A.max_element(torch.tensor(lit, dtype=dtype).to(dev)) == want


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=str)
def test_arg_reduce_signed_zero(dev, dtype):
    """-0.0 == 0.0: the first index wins, whichever zero sits there."""
    npdt = NP[dtype]
    for n, at in ((4, (1, 2)), (300, (3, 70)), (300, (70, 256)), (B + 5, (B - 1, B + 4))):
        for first in (0.0, -0.0):
            for is_max in (True, False):
                x = np.full(n, -1.0 if is_max else 1.0, dtype=npdt)
                x[at[0]], x[at[1]] = first, -first
                _check_arg(x, dev, is_max)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int16, torch.float16], ids=str)
def test_unsupported_dtypes_raise_type_error(dev, dtype):
    x = torch.arange(10).to(dtype).to(dev)
    off = torch.tensor([0, 4, 10]).to(dev)
    name = str(dtype).split(".")[-1]
    for call in (lambda: A.max_element(x), lambda: A.min_element(x), lambda: A.segment_reduce(x, off),
                 lambda: A.reduce_by_key(torch.arange(10, dtype=torch.int32).to(dev), x),
                 lambda: A.lower_bound(x, x), lambda: A.upper_bound(x, x), lambda: A.inner_product(x, x),
                 lambda: A.inner_product(x, x, "eq")):
        with pytest.raises(TypeError, match=name):
            call()
    if dtype != torch.uint8:  # 2-byte elements: no select either
        with pytest.raises(TypeError, match=name):
            A.unique(x)


# ============================================================ inner product
IP_SIZES = [0, 1, 255, 256, 257, B, B + 1, 2_000_003]


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("n", IP_SIZES)
def test_inner_product_mul(dev, n):
    g = gen(60 + n % 97)
    a = torch.randn(n, generator=g)
    sign = torch.ones(n)
    sign[1::2] = -1.0
    for b in (torch.randn(n, generator=g), sign):  # the second one cancels
        prod = a.numpy().astype(np.float64) * b.numpy().astype(np.float64)
        ref, bound = float(np.sum(prod)), 2.0 * n * 2.0 ** -53 * float(np.sum(np.abs(prod)))
        got = A.inner_product(a.to(dev), b.to(dev))
        assert isinstance(got, float) and abs(got - ref) <= bound, (got, ref, bound)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_inner_product_eq(dev):
    """Counts beyond 2^24 (a float32 accumulator stops there); the compare is
    on the 32-bit words: 0.0 != -0.0, NaNs of equal bits are equal."""
    n = 2 ** 24 + 3
    a = cached("ip_eq", lambda: rand_data(torch.int32, n, gen(61)))
    ad = a.to(dev)
    got = A.inner_product(ad, ad.clone(), "eq")
    assert got == float(n)
    b = a.clone()
    b[::3] ^= -2 ** 31  # a third differ, in the top bit only
    assert A.inner_product(ad, b.to(dev), "eq") == float(n - (n + 2) // 3)
    qn, qn1, _ = nan_bits(torch.float32)
    x = from_bits(torch.tensor([0, 0x80000000, qn, qn, qn1, 0x3F800000], dtype=torch.int64), torch.float32)
    y = from_bits(torch.tensor([0x80000000, 0x80000000, qn, qn1, qn1, 0x3F800000], dtype=torch.int64), torch.float32)
    assert A.inner_product(x.to(dev), y.to(dev), "eq") == 4.0
    for n0 in (0, 1, 257):
        assert A.inner_product(ad[:n0], ad[:n0], "eq") == float(n0)


# ============================================================ counting sort
@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("num_keys", [1, 2, 3, 255, 256, 257])
@pytest.mark.parametrize("n", [0, 1, T + 1])
def test_counting_sort(dev, num_keys, n):
    """Keys only, int64 keys and float32 values against a stable sort."""
    k = torch.randint(0, num_keys, (n,), generator=gen(70 + num_keys), dtype=torch.int64).to(torch.int32)
    if n:
        k[-1] = num_keys - 1
    ref = torch.sort(k, stable=True)
    v = torch.arange(n, dtype=torch.float32) * 0.5 - 3.0
    kd = k.to(dev)
    got = A.counting_sort(kd, num_keys)
    assert got.dtype == torch.int32 and torch.equal(got.cpu(), ref.values)
    got = A.counting_sort(kd.to(torch.int64), num_keys)
    assert got.dtype == torch.int64 and torch.equal(got.cpu(), ref.values.to(torch.int64))
    for keys in (kd, kd.to(torch.int64)):
        gk, gv = A.counting_sort(keys, num_keys, v.to(dev))
        assert gk.dtype == keys.dtype and gv.dtype == torch.float32
        assert torch.equal(gk.cpu(), ref.values.to(keys.dtype)) and torch.equal(gv.cpu(), v[ref.indices])
    assert torch.equal(kd.cpu(), k)
