"""Generators, oracles and comparisons shared by the 32-bit scan tests
(test_scan32.py, test_segscan32.py) and the poison-isolation test of
test_segscan64.py.

Oracles are numpy in a wider type: int64 ``cumsum`` reduced modulo 2^32 for the
integers, float64 for float32. float32 results are compared

* bitwise ("exact tier") on integer-valued data whose every partial sum, in any
  association, is an integer below 2^24 -- asserted on the float64 oracle by
  :func:`assert_exact_tier`: the largest minus the smallest prefix (the empty
  one included) bounds every contiguous partial sum;
* otherwise ("rounding tier") under the worst-case bound of any summation
  order, ``1.01 * m * 2^-24 * sum |v_j|`` (m: the 1-based position in the scan
  or segment, + 1 with ``mul`` for the product's own rounding).

"Bitwise" leaves out the sign of a zero: the kernels shift +0 in as the identity
of their lane scans, so both sides are normalised with ``+ 0.0``.
"""
import numpy as np
import torch

U32 = 2.0 ** -24
CPU = torch.device("cpu")

_cache: dict = {}


def cached(key, make):
    """A few entries are kept: parametrisations visit the cases of one data set
    consecutively, so inputs, device copies and oracles are computed once."""
    if key not in _cache:
        if len(_cache) > 16:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ conversion
def to_torch(a: np.ndarray, dev) -> torch.Tensor:
    if a.dtype == np.uint32:
        return torch.from_numpy(a.view(np.int32)).to(dev).view(torch.uint32)
    return torch.from_numpy(a).to(dev)


def to_numpy(t: torch.Tensor) -> np.ndarray:
    if t.dtype == torch.uint32:
        return t.view(torch.int32).cpu().numpy().view(np.uint32)
    return t.cpu().numpy()


def view_of(a: np.ndarray, offset: int, dev) -> torch.Tensor:
    """A copy of ``a`` on ``dev`` that starts ``offset`` elements into a fresh
    buffer: contiguous, aligned to the element only."""
    base = torch.zeros(a.size + offset, dtype=to_torch(a[:1], CPU).dtype, device=dev)
    v = base[offset:]
    v.copy_(to_torch(a, dev))
    assert v.is_contiguous() and v.data_ptr() == base.data_ptr() + offset * a.itemsize
    return v


# ----------------------------------------------------------------- comparisons
def bits(a: np.ndarray) -> np.ndarray:
    """The bits of every element; a float zero loses its sign (see above)."""
    if a.dtype.kind == "f":
        return (a + a.dtype.type(0.0)).view(np.int32 if a.itemsize == 4 else np.int64)
    return a


def assert_bits(got, want: np.ndarray, what: str = "") -> None:
    g = to_numpy(got) if isinstance(got, torch.Tensor) else got
    assert g.dtype == want.dtype and g.shape == want.shape, (g.dtype, want.dtype, g.shape, want.shape)
    bad = np.flatnonzero(bits(g) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} elements differ, first at {bad[0]}: {g[bad[0]]!r} != {want[bad[0]]!r}"


def assert_bound(got, ref: np.ndarray, bound: np.ndarray, what: str = "") -> None:
    g = to_numpy(got) if isinstance(got, torch.Tensor) else got
    err = np.abs(g.astype(np.float64) - ref)
    worst = int(np.argmax(err - bound))
    assert np.all(err <= bound), f"{what}: element {worst}: error {err[worst]:.3e} > bound {bound[worst]:.3e}"


def excl(inc: np.ndarray) -> np.ndarray:
    return np.concatenate([np.zeros(1, dtype=inc.dtype), inc[:-1]])


# --------------------------------------------------------------- plain oracles
def int_oracle(x: np.ndarray) -> np.ndarray:
    """Inclusive sums of int32 / uint32 data, exact in int64, modulo 2^32."""
    c = np.cumsum(x.astype(np.int64), dtype=np.int64)
    assert x.size < 2 ** 31  # |c| < 2^63: the int64 sum itself is exact
    return (c & 0xFFFFFFFF).astype(np.uint32).view(x.dtype)


def assert_exact_tier(v: np.ndarray) -> np.ndarray:
    """float64 inclusive sums of integer-valued ``v``; asserts that every
    contiguous partial sum is an integer of magnitude below 2^24, i.e. exact in
    float32 whatever the association."""
    c = np.cumsum(v.astype(np.float64))
    assert np.all(c == np.rint(c))
    assert max(c.max(), 0.0) - min(c.min(), 0.0) < 2.0 ** 24
    return c


def rounding_oracle(v: np.ndarray, tile: int):
    """(float64 inclusive sums, bound) of a rounding-active plain scan, with the
    condition that makes the bound meaningful: it stays below half of the
    smallest tile sum (the last, partial tile included), so a lost or doubled
    tile cannot hide under it. Checked on the oracle alone."""
    n = v.size
    c = np.cumsum(v.astype(np.float64))
    bound = 1.01 * np.arange(1, n + 1) * U32 * np.cumsum(np.abs(v.astype(np.float64)))
    edges = np.append(np.arange(0, n, tile), n)
    tile_sums = np.diff(np.concatenate([[0.0], c])[edges])
    assert bound.max() < 0.5 * np.abs(tile_sums).min(), (bound.max(), np.abs(tile_sums).min())
    return c, bound


# ------------------------------------------------------------------- segments
def seg_info(f: np.ndarray):
    """(segment starts, segment id of every element) of uint8 head flags (any
    non-zero byte is a head; element 0 starts a segment anyway)."""
    h = f != 0
    h[0] = True
    return np.flatnonzero(h), np.cumsum(h, dtype=np.int64) - 1


def pack_bits(f: np.ndarray) -> np.ndarray:
    """int32 bitmask words of uint8 flags: bit i % 32 of word i // 32."""
    return np.packbits(np.pad(f != 0, (0, -f.size % 32)), bitorder="little").view(np.int32).copy()


def seg_exact_oracle(v: np.ndarray, f: np.ndarray, limit: float) -> np.ndarray:
    """cumsum(v) - base[seg_id] in float64 for integer-valued ``v``. Asserts
    that the sum of |v| over every segment stays below ``limit`` (2^24 for
    float32): every partial sum inside a segment is then exact in any order."""
    starts, seg = seg_info(f)
    v = v.astype(np.float64)
    assert np.all(v == np.rint(v))
    ca = np.cumsum(np.abs(v))
    assert ca[-1] < 2.0 ** 53
    assert (ca - np.concatenate([[0.0], ca])[starts][seg]).max() < limit
    c = np.cumsum(v)
    return c - np.concatenate([[0.0], c])[starts][seg]


def seg_rounding_oracle(v: np.ndarray, f: np.ndarray, u: float, extra: int = 0):
    """(per-segment running sums in a wider type, bound): one cumsum per
    segment. ``v``: float64 (products included) for float32 results, longdouble
    for float64 ones."""
    starts, seg = seg_info(f)
    assert starts.size <= 200_000
    ref = np.empty(v.size, dtype=v.dtype)
    asum = np.empty(v.size, dtype=np.float64)
    av = np.abs(v).astype(np.float64)
    for lo, hi in zip(starts, np.append(starts[1:], v.size)):
        ref[lo:hi] = np.cumsum(v[lo:hi])
        asum[lo:hi] = np.cumsum(av[lo:hi])
    m = np.arange(v.size) - starts[seg] + 1 + extra
    return ref, 1.01 * m * u * asum
