"""Generators, oracles and comparisons of test_algorithms_edges.py.

Every oracle is numpy on the CPU in the native integer dtype or on the bit
pattern of a float (viewed as the same-width integer); none goes through
float64 for integer keys and none calls a ``cme213x`` op.
"""
import numpy as np
import torch

T = 4096  # kTile of csrc/hip/algorithms.hip (256 threads x 16 items)
BIG = 5 * 2 ** 20 + 3  # 1281 tiles: more than one round of a persistent grid of at most 4 blocks on each of 256 CUs
TILE_SIZES = [0, 1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 17]

CPU = torch.device("cpu")
_INT = {1: torch.uint8, 4: torch.int32, 8: torch.int64}
NP = {torch.uint8: np.uint8, torch.int32: np.int32, torch.uint32: np.uint32, torch.int64: np.int64,
      torch.float32: np.float32, torch.float64: np.float64}

_cache: dict = {}


def cached(key, make):
    """Inputs and oracles of one data set are computed once: the cpu and gpu
    parametrisations of a case follow each other."""
    if key not in _cache:
        if len(_cache) > 24:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


def gen(seed: int) -> torch.Generator:
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------ conversion
def bits(t: torch.Tensor) -> torch.Tensor:
    """The raw bit pattern of a tensor, on the CPU, as an integer tensor."""
    t = t.cpu().contiguous()
    return t.view(_INT[t.element_size()])


def to_numpy(t: torch.Tensor) -> np.ndarray:
    t = t.cpu().contiguous()
    if t.dtype == torch.uint32:
        return t.view(torch.int32).numpy().view(np.uint32)
    return t.numpy()


def to_torch(a: np.ndarray) -> torch.Tensor:
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).view(torch.uint32)
    return torch.from_numpy(a)


def from_bits(b: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """int64 bit patterns -> a tensor of ``dtype`` with those (low) bits."""
    w = torch.empty(0, dtype=dtype).element_size()
    if w == 1:
        return (b & 0xFF).to(torch.uint8).view(dtype)
    if w == 4:
        b = b & 0xFFFFFFFF
        return torch.where(b >= 2 ** 31, b - 2 ** 32, b).to(torch.int32).view(dtype)
    return b.view(dtype)


def view_of(t: torch.Tensor, offset: int, dev) -> torch.Tensor:
    """A copy of ``t`` on ``dev`` that starts ``offset`` elements into a fresh
    buffer: contiguous; with offset 1 aligned to the element only."""
    base = torch.zeros(t.numel() + offset + 1, dtype=t.dtype, device=dev)
    v = base[offset:offset + t.numel()]
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() == base.data_ptr() + offset * t.element_size()
    if offset == 0:
        assert v.data_ptr() % 16 == 0
    else:
        assert v.data_ptr() % 16 != 0
    return v


# ------------------------------------------------------------------ generators
def rand_data(dtype: torch.dtype, n: int, g: torch.Generator) -> torch.Tensor:
    """Full-width data: the low and the high 32-bit word of an 8-byte element
    vary independently (full-range int64; float64 with random mantissas)."""
    if dtype == torch.uint8:
        return torch.randint(0, 256, (n,), generator=g, dtype=torch.int64).to(torch.uint8)
    if dtype in (torch.int32, torch.uint32):
        return torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32).view(dtype)
    if dtype == torch.int64:
        return torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)
    return torch.randn(n, generator=g, dtype=dtype)


def from_ids(ids: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Values that are equal exactly where the int64 run ids are equal (ids
    below 2^21; uint8: consecutive ids differ). For the 8-byte dtypes
    consecutive ids differ alternately in the high word only and in the low
    word only, so a compare that drops either word merges two runs."""
    if dtype == torch.uint8:
        return from_bits(ids % 251, dtype)
    if dtype == torch.int32:
        return from_bits(ids * 2654435761, dtype)  # odd multiplier: a bijection modulo 2^32
    if dtype == torch.float32:
        return from_bits(0x3F800000 + ids, dtype)
    hi, lo = (ids + 1) >> 1, ids >> 1
    base = 0x3FF0000000000000 if dtype == torch.float64 else -2 ** 62
    return from_bits(base + (hi << 32) + lo, dtype)


def run_ids(n: int, g: torch.Generator, p: float = 0.3) -> torch.Tensor:
    """Random runs: a new run starts with probability p."""
    if n == 0:
        return torch.zeros(0, dtype=torch.int64)
    return torch.cumsum((torch.rand(n, generator=g) < p).to(torch.int64), 0)


def nan_bits(dtype: torch.dtype) -> tuple[int, int, int]:
    """Three NaN bit patterns: the canonical quiet NaN (what ``float('nan')``
    becomes in ``dtype``), the same with payload bit 0 set, and its negative."""
    if dtype == torch.float32:
        return 0x7FC00000, 0x7FC00001, 0xFFC00000
    return 0x7FF8000000000000, 0x7FF8000000000001, -0x0008000000000000


def bitwise_specials(dtype: torch.dtype) -> torch.Tensor:
    """0, -0, -0, 0, NaN a, NaN a, NaN b, NaN b, NaN c, NaN a, 1, 1, -0, 0."""
    a, b, c = nan_bits(dtype)
    one = 0x3F800000 if dtype == torch.float32 else 0x3FF0000000000000
    neg0 = 0x80000000 if dtype == torch.float32 else -2 ** 63
    return from_bits(torch.tensor([0, neg0, neg0, 0, a, a, b, b, c, a, one, one, neg0, 0], dtype=torch.int64), dtype)


# -------------------------------------------------------------- select oracles
def head_mask(xb: np.ndarray) -> np.ndarray:
    """Element i starts a run: i == 0 or its bits differ from those of i - 1."""
    m = np.ones(xb.size, dtype=bool)
    m[1:] = xb[1:] != xb[:-1]
    return m


def flag_mask(flags: torch.Tensor) -> np.ndarray:
    """A flag is set iff it is != 0 in its own dtype (-0.0 is not set)."""
    return to_numpy(flags) != 0


def ora_values(x: torch.Tensor, m: np.ndarray) -> torch.Tensor:
    return bits(x)[torch.from_numpy(m)]


def ora_indices(m: np.ndarray) -> torch.Tensor:
    return torch.from_numpy(np.flatnonzero(m).astype(np.int64))


def ora_partition(x: torch.Tensor, m: np.ndarray) -> tuple[torch.Tensor, int]:
    xb, mt = bits(x), torch.from_numpy(m)
    return torch.cat([xb[mt], xb[~mt]]), int(m.sum())


def scalar_bits(x: torch.Tensor, value) -> int:
    """Bit pattern of ``value`` in x's dtype, as a signed integer."""
    return int(bits(torch.tensor([value], dtype=x.dtype)).to(torch.int64).item())


# -------------------------------------------------------------- search oracles
def search_keys(dtype: torch.dtype, n: int, g: torch.Generator) -> np.ndarray:
    """Sorted full-width keys in the native numpy dtype.
    uint32: more than half at or above 2^31. int64: the whole range, a quarter
    of them pairs beyond +-2^53 that differ only below bit 10 (equal after a
    trip through float64). int32: the whole range. Floats: both signs,
    duplicates, and (n >= 16) +-inf, -0.0, 0.0 and the largest finite values."""
    npdt = NP[dtype]
    if dtype == torch.uint32:
        k = torch.randint(0, 2 ** 32, (n,), generator=g, dtype=torch.int64)
        k[: n // 2 + 1] |= 2 ** 31
        a = k.numpy().astype(np.uint32)
    elif dtype == torch.int32:
        a = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).numpy().astype(np.int32)
    elif dtype == torch.int64:
        k = torch.randint(-2 ** 63, 2 ** 63 - 1, (n,), generator=g, dtype=torch.int64)
        p = n // 8
        if p:
            base = k[:p] & ~1023  # |base| > 2^53 but for a 2^-9 share of the draws; asserted below
            base = torch.where((base > 2 ** 53) | (base < -2 ** 53), base, torch.full_like(base, 2 ** 60))
            k[:p] = base | torch.randint(0, 1024, (p,), generator=g, dtype=torch.int64)
            k[p:2 * p] = base | torch.randint(0, 1024, (p,), generator=g, dtype=torch.int64)
            assert bool(((k[:p] > 2 ** 53) | (k[:p] < -2 ** 53)).all()) and bool(((k[:p] ^ k[p:2 * p]) < 1024).all())
        a = k.numpy()
    else:
        k = torch.randn(n, generator=g, dtype=torch.float64) * 1e3
        if n >= 4:
            k[: n // 4] = k[n // 4: 2 * (n // 4)]  # duplicates
        a = k.numpy().astype(npdt)
        if n >= 16:
            big = np.finfo(npdt).max
            a[-8:] = np.array([np.inf, -np.inf, -0.0, 0.0, 0.0, -0.0, big, -big], dtype=npdt)
    a = np.sort(a)
    assert a.dtype == npdt
    return a


def search_queries(keys: np.ndarray, m: int | None, g: torch.Generator) -> np.ndarray:
    """Every key, every key -1 / +1 (integers, wrapping at the ends of the
    range) or its two float neighbours, and values below the minimum and above
    the maximum; shuffled, then repeated or cut to ``m`` queries."""
    dt = keys.dtype
    if dt.kind == "f":
        lim = np.array([-np.inf, np.inf, -np.finfo(dt).max, np.finfo(dt).max, -0.0, 0.0], dtype=dt)
        with np.errstate(over="ignore"):  # the neighbours of the largest finite values are +-inf
            near = [np.nextafter(keys, dt.type(-np.inf)), np.nextafter(keys, dt.type(np.inf))]
    else:
        lim = np.array([np.iinfo(dt).min, np.iinfo(dt).max, np.iinfo(dt).min + 1, np.iinfo(dt).max - 1, 0, 1], dtype=dt)
        near = [keys - dt.type(1), keys + dt.type(1)]
    q = np.concatenate([keys, *near, lim])
    q = q[torch.randperm(q.size, generator=g).numpy()]
    return q if m is None else np.resize(q, m)


def ora_search(keys: np.ndarray, q: np.ndarray, upper: bool) -> torch.Tensor:
    assert keys.dtype == q.dtype
    return torch.from_numpy(np.searchsorted(keys, q, side="right" if upper else "left").astype(np.int64))


# ------------------------------------------------------ segment-reduce oracles
def identity(npdt, op: str):
    """The empty segment's value (csrc/cpu/algorithms_cpu.cpp identity())."""
    if op == "sum":
        return npdt(0)
    if np.dtype(npdt).kind == "f":
        return npdt(-np.inf if op == "max" else np.inf)
    return np.iinfo(npdt).min if op == "max" else np.iinfo(npdt).max


def ora_segments(v: np.ndarray, off: np.ndarray, op: str, wide=None) -> np.ndarray:
    """Per-segment sum / max / min. Sums run in ``wide`` (int64 for the
    integers: exact, and the cast back wraps like the native sum; float64 for
    floats) and are cast back to v's dtype unless ``wide`` is given."""
    lens = np.diff(off)
    assert np.all(lens >= 0) and off[0] >= 0 and off[-1] <= v.size
    ne = lens > 0
    out_dt = v.dtype if wide is None else np.dtype(wide)
    out = np.full(lens.size, identity(out_dt.type, op), dtype=out_dt)
    if ne.any():
        body = v[: off[-1]]
        if op == "sum":
            acc = wide or (np.int64 if v.dtype.kind == "i" else np.float64)
            with np.errstate(over="ignore"):
                out[ne] = np.add.reduceat(body.astype(acc), off[:-1][ne]).astype(out_dt)
        else:
            out[ne] = (np.maximum if op == "max" else np.minimum).reduceat(body, off[:-1][ne])
    return out


def assert_exact_sums(v: np.ndarray, off: np.ndarray) -> None:
    """Integer-valued data whose sum of |v| over every segment stays below
    2^24 (float32) / 2^53 (float64): every partial sum, in any order, is then
    an exactly representable integer."""
    if v.dtype.kind != "f":
        return
    w = v.astype(np.float64)
    assert np.all(w == np.rint(w))
    limit = 2.0 ** 24 if v.dtype == np.float32 else 2.0 ** 53
    assert ora_segments(np.abs(w), off, "sum").max(initial=0.0) < limit
