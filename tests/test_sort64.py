"""64-bit keys, 8-byte values, descending order and argsort of ops.sort.

Oracles: int64 keys against ``torch.sort(stable=True, descending=...)`` on
the CPU; uint64 and float64 keys against a stable ``numpy.argsort`` of the
64-bit order code (float64: ``~i`` where the sign bit is set, ``i ^ 2**63``
otherwise -- the IEEE total order), complemented for descending order. Every
comparison is exact and on bit patterns, so -0 and +0 are told apart. The
same cases run on the CPU backend (unmarked) and on the GPU."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401
from cme213x import _ext
from cme213x.ops import sort as S
from cme213x.utils import tuning

T = S.RADIX64_TILE  # keys per downsweep tile of the GPU 64-bit sort
N_PAT = 2 * T + 17

CPU = pytest.param("cpu", id="cpu")
GPU = pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")
DEVS = [CPU, GPU]
# (device, radix_ds override): the default lane-order ranks and, on the GPU,
# the ballot-match ranks (6 = match + prefetch + wide tiles)
ARMS = [pytest.param(("cpu", None), id="cpu"), pytest.param(("gpu", None), marks=pytest.mark.gpu, id="gpu"),
        pytest.param(("gpu", 6), marks=pytest.mark.gpu, id="gpu-match")]

_INT = {4: torch.int32, 8: torch.int64}
_NP_U = {4: np.uint32, 8: np.uint64}


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


@pytest.fixture
def arm(request):
    name, ds = request.param
    return (request.getfixturevalue("gpu") if name == "gpu" else torch.device("cpu")), ds


def _bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bit pattern of a CPU tensor as a signed integer tensor."""
    return t.cpu().contiguous().view(_INT[t.element_size()])


def _code(t: torch.Tensor) -> np.ndarray:
    """Unsigned order code of CPU keys (the sort's total order)."""
    w = t.element_size()
    u = _bits(t).numpy().view(_NP_U[w])
    top = _NP_U[w](1 << (8 * w - 1))
    if t.dtype in (torch.uint32, torch.uint64):
        return u
    if t.dtype in (torch.int32, torch.int64):
        return u ^ top
    return np.where(u & top != 0, ~u, u ^ top)


def _ref_perm(t: torch.Tensor, descending: bool) -> torch.Tensor:
    if t.dtype in (torch.int32, torch.int64):
        return torch.sort(t, stable=True, descending=descending).indices
    c = _code(t)
    return torch.from_numpy(np.argsort(~c if descending else c, kind="stable"))


def _check(keys: torch.Tensor, device, values: torch.Tensor | None = None, descending: bool = False, **kw):
    """Sort CPU ``keys`` (and values) on ``device`` and compare with the oracle."""
    perm = _ref_perm(keys, descending)
    kd = keys.to(device)
    k0 = _bits(kd).clone()
    if values is None:
        out = S.sort(kd, descending=descending, **kw)
        assert out.dtype == keys.dtype and out.device == kd.device
        assert torch.equal(_bits(out), _bits(keys)[perm])
    else:
        vd = values.to(device)
        out, vout = S.sort(kd, vd, descending=descending, **kw)
        assert out.dtype == keys.dtype and vout.dtype == values.dtype
        assert torch.equal(_bits(out), _bits(keys)[perm])
        assert torch.equal(_bits(vout), _bits(values)[perm])
        assert torch.equal(_bits(vd), _bits(values))  # inputs untouched
    assert torch.equal(_bits(kd), k0)


def _gen(seed=0):
    return torch.Generator().manual_seed(seed)


def _rand_i64(n, g):
    return torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)


def _rand_f64_special(n, g):
    x = torch.randn(n, generator=g, dtype=torch.float64)
    tiny = float(np.nextafter(0.0, 1.0))  # the smallest denormal
    special = torch.tensor([0.0, -0.0, float("inf"), float("-inf"), tiny, -tiny, 2 * tiny, -2 * tiny, 1.5, 1.5, -1.5],
                           dtype=torch.float64)
    idx = torch.randint(0, n, (n // 3,), generator=g)
    x[idx] = special[torch.randint(0, special.numel(), (idx.numel(),), generator=g)]
    x[torch.randint(0, n, (n // 5,), generator=g)] = x[0].item()  # duplicates of an ordinary value
    return x


def _keys(dtype, n, g):
    if dtype == torch.int64:
        return _rand_i64(n, g)
    if dtype == torch.uint64:
        return _rand_i64(n, g).view(torch.uint64)
    return _rand_f64_special(n, g)


DT64 = [torch.int64, torch.uint64, torch.float64]
DT32 = [torch.int32, torch.uint32, torch.float32]


def _pattern(name: str) -> torch.Tensor:
    g = _gen(100 + PATTERNS.index(name))
    n = N_PAT
    byte = torch.randint(0, 256, (n,), generator=g, dtype=torch.int64)
    if name == "i64_full":
        return _rand_i64(n, g)
    if name == "i64_small_mixed_sign":  # top passes: identity copies, the sign digit takes two values
        return torch.randint(-2 ** 20, 2 ** 20, (n,), generator=g, dtype=torch.int64)
    if name == "i64_equal":
        return torch.full((n,), -123456789012345, dtype=torch.int64)
    if name == "i64_top_byte":
        return (byte << 56) | 0x00123456789ABCDE
    if name == "i64_bits_32_39":  # the digit next to the boundary of the two 32-bit halves
        return (byte << 32) | 0x1200000000345678
    if name == "u64_full":
        return _rand_i64(n, g).view(torch.uint64)
    if name == "u64_above_2_63":
        return (torch.randint(0, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64) | -2 ** 63).view(torch.uint64)
    if name == "u64_equal":
        return torch.full((n,), -5, dtype=torch.int64).view(torch.uint64)
    if name == "u64_top_byte":
        return ((byte << 56) | 0x00FFFFFFFFFFFF01).view(torch.uint64)
    if name == "u64_bits_32_39":
        return ((byte << 32) | -2 ** 63 | 0x77).view(torch.uint64)
    if name == "f64_special":
        return _rand_f64_special(n, g)
    if name == "f64_equal":
        return torch.full((n,), -0.0, dtype=torch.float64)
    raise KeyError(name)


PATTERNS = ["i64_full", "i64_small_mixed_sign", "i64_equal", "i64_top_byte", "i64_bits_32_39", "u64_full",
            "u64_above_2_63", "u64_equal", "u64_top_byte", "u64_bits_32_39", "f64_special", "f64_equal"]


@pytest.mark.gpu
def test_tile_constant_matches_library(gpu):
    assert _ext._fn("hip", "cme_radix_sort64_tile")() == T


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", DT64, ids=str)
@pytest.mark.parametrize("n", [1, 2, 65, T - 1, T, T + 1, 2 * T + 17, 100003])
def test_sizes_keys_only(dev, dtype, n):
    _check(_keys(dtype, n, _gen(n)), dev)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DT64, ids=str)
@pytest.mark.parametrize("with_values", [False, True])
def test_three_tiles_per_block_carry(gpu, dtype, with_values):
    """Grid capped at two blocks, n = 5T + 3: each block walks three tiles
    (the last one partial), so the per-digit bases carry across tiles."""
    n = 5 * T + 3
    g = _gen(7)
    keys = _keys(dtype, n, g)
    vals = torch.arange(n, dtype=torch.int64) + 2 ** 40 if with_values else None
    with tuning.override(radix_maxblocks=2):
        _check(keys, gpu, vals)
        _check(keys, gpu, vals, descending=True)


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("name", PATTERNS)
def test_key_patterns(arm, name):
    device, ds = arm
    keys = _pattern(name)
    vals = torch.arange(keys.numel(), dtype=torch.int32)
    if ds is None:
        _check(keys, device)
        _check(keys, device, vals)
    else:
        with tuning.override(radix_ds=ds):
            _check(keys, device)
            _check(keys, device, vals)
            _check(keys, device, vals.to(torch.float64), descending=True)


def _payload(vdtype, n):
    i = torch.arange(n, dtype=torch.int64)
    if vdtype == torch.int32:
        return (i * 3 + 1).to(torch.int32)
    if vdtype == torch.float32:
        return i.to(torch.float32) + 0.5
    if vdtype == torch.int64:
        return i + 2 ** 40
    return i.to(torch.float64) * 0.25 - 7.0


@pytest.mark.parametrize("arm", ARMS, indirect=True)
@pytest.mark.parametrize("dtype", DT64, ids=str)
@pytest.mark.parametrize("vdtype", [torch.int32, torch.float32, torch.int64, torch.float64], ids=str)
def test_key_value_stability(arm, dtype, vdtype):
    device, ds = arm
    n = N_PAT
    small = torch.randint(0, 1000, (n,), generator=_gen(3), dtype=torch.int64)
    keys = small.to(torch.float64) if dtype == torch.float64 else small.view(dtype)
    vals = _payload(vdtype, n)
    if ds is None:
        _check(keys, device, vals)
    else:
        with tuning.override(radix_ds=ds):
            _check(keys, device, vals)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", DT64 + DT32, ids=str)
def test_descending(dev, dtype):
    n = N_PAT
    g = _gen(5)
    if dtype in DT64:
        keys = _keys(dtype, n, g)
        dup = torch.randint(-50, 50, (n,), generator=g, dtype=torch.int64)
        dup = dup.to(torch.float64) if dtype == torch.float64 else dup.view(dtype)
        vals = _payload(torch.int64, n)
    else:
        i = torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        if dtype == torch.float32:
            keys = _rand_f64_special(n, g).to(torch.float32)
        else:
            keys = i.view(dtype)
        d = torch.randint(-50, 50, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        dup = d.to(torch.float32) if dtype == torch.float32 else d.view(dtype)
        vals = _payload(torch.int32, n)
    for k in (keys, dup):  # full range, and many ties (stability of the descending order)
        _check(k, dev, descending=True)
        _check(k, dev, vals, descending=True)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("key_bits", [1, 8, 20, 33, 40, 64])
def test_key_bits(dev, key_bits):
    n = N_PAT
    hi = 2 ** 63 - 1 if key_bits == 64 else 2 ** key_bits
    keys = torch.randint(0, hi, (n,), generator=_gen(key_bits), dtype=torch.int64)
    vals = _payload(torch.int64, n)
    _check(keys, dev, key_bits=key_bits)
    _check(keys, dev, vals, key_bits=key_bits)
    _check(keys, dev, vals, key_bits=key_bits, descending=True)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("n", [2 * T + 17, 2 * T + 18])
@pytest.mark.parametrize("with_values", [False, True])
def test_misaligned_view(dev, n, with_values):
    """keys[1:1+n] of an int64 tensor is 8-byte, not 16-byte aligned."""
    g = _gen(n)
    big = _rand_i64(n + 2, g).to(dev)
    vbig = (torch.arange(n + 2, dtype=torch.int64) + 2 ** 41).to(dev)
    kd, vd = big[1:1 + n], vbig[1:1 + n]
    assert kd.data_ptr() % 16 == 8
    ref = torch.sort(kd.cpu(), stable=True)
    if with_values:
        k, v = S.sort(kd, vd)
        assert torch.equal(v.cpu(), vd.cpu()[ref.indices])
    else:
        k = S.sort(kd)
    assert torch.equal(k.cpu(), ref.values)
    assert torch.equal(S.argsort(kd).cpu(), ref.indices)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", [torch.int32, torch.int64], ids=str)
@pytest.mark.parametrize("descending", [False, True])
def test_argsort_int(dev, dtype, descending):
    for n, lo, hi in ((N_PAT, -300, 300), (T + 1, -2 ** 31, 2 ** 31 - 1), (1, 0, 5), (0, 0, 5)):
        keys = torch.randint(lo, hi, (n,), generator=_gen(n), dtype=torch.int64).to(dtype)
        got = S.argsort(keys.to(dev), descending=descending)
        assert got.dtype == torch.int64 and got.device == keys.to(dev).device
        assert torch.equal(got.cpu(), torch.sort(keys, stable=True, descending=descending).indices)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64, torch.uint64], ids=str)
@pytest.mark.parametrize("descending", [False, True])
def test_argsort_gathers_the_sorted_keys(dev, dtype, descending):
    g = _gen(9)
    if dtype == torch.uint64:
        keys = _rand_i64(N_PAT, g).view(dtype)
    else:
        keys = _rand_f64_special(N_PAT, g).to(dtype)
    kd = keys.to(dev)
    order = S.argsort(kd, descending=descending)
    assert order.dtype == torch.int64
    assert torch.equal(order.cpu(), _ref_perm(keys, descending))
    assert torch.equal(_bits(kd)[order.cpu()], _bits(S.sort(kd, descending=descending)))


@pytest.mark.gpu
def test_stream_capture_int64_key_value(gpu):
    """An int64 key + int64 value sort captured into a HIP graph: two replays
    with the input contents changed in between equal the eager results."""
    n = 3 * T + 5
    g = _gen(21)
    inputs = [torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64) for _ in range(2)]
    keys = inputs[0].to(gpu)
    vals = (torch.arange(n, dtype=torch.int64) - 2 ** 35).to(gpu)
    s = torch.cuda.Stream(gpu)
    s.wait_stream(torch.cuda.current_stream(gpu))
    with torch.cuda.stream(s):
        S.sort(keys, vals)  # warm-up outside capture (one-time lane-order check)
    torch.cuda.current_stream(gpu).wait_stream(s)
    torch.cuda.synchronize(gpu)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        k_out, v_out = S.sort(keys, vals)
    for x in reversed(inputs):
        keys.copy_(x.to(gpu))
        graph.replay()
        torch.cuda.synchronize(gpu)
        k_eager, v_eager = S.sort(keys, vals)
        ref = torch.sort(x, stable=True)
        assert torch.equal(k_out, k_eager) and torch.equal(v_out, v_eager)
        assert torch.equal(k_out.cpu(), ref.values) and torch.equal(v_out.cpu(), vals.cpu()[ref.indices])


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_errors(dev):
    k64 = torch.arange(100, dtype=torch.int64).to(dev)
    k32 = torch.arange(100, dtype=torch.int32).to(dev)
    for algo in ("merge", "onesweep"):
        with pytest.raises(TypeError, match="radix"):
            S.sort(k64, algo=algo)
    with pytest.raises(TypeError):
        S.sort(k32, k64)  # 8-byte values under 32-bit keys stay out of scope
    with pytest.raises(TypeError):
        S.sort(k64, k64.to(torch.int16))
    with pytest.raises(TypeError):
        S.sort(k64.to(torch.float64), key_bits=20)
