"""Generators, oracles and format interpreters of test_spmv_exact.py.

Exact tier. Matrix values and ``x`` are nonzero integers in [-8, 8] stored as
float32, the old ``y`` holds even integers in [-64, 64] and ``beta`` is one of
0, 1, -2, 0.5. With ``64 * max_row_len + 128 < 2**24`` (asserted) every partial
sum of a row, in any order, fused or not, through atomics or not, is an exactly
representable integer: the kernel result must equal an int64 numpy oracle bit
for bit. A zero is never drawn, so a dropped term always shows.

Poison. Columns are drawn from [1, ncols - 2]; ``x[0]``, ``x[ncols - 1]`` and
every other column no entry refers to are NaN, and a ``beta == 0`` run starts
from a ``y`` full of NaN: a padding read that reaches the sum, or a ``0 * y``,
fails the comparison. The oracle never touches those entries.

DIA stores explicit zeros inside the matrix (a diagonal's slots at columns no
entry refers to) and multiplies them with ``x`` like any entry: for DIA a
column counts as referenced when any in-range slot lies on it, and the poison
is NaN in the columns NO slot reaches plus a nonzero value in the data slots
whose column is out of range (which only a leaking clamped read would use).

None of the oracles or interpreters calls a ``cme213x`` op.
"""
import numpy as np
import torch

from cme213x.ops.spmv import COO, CSR, DIA, ELL, HYB, CSRAligned, CSRColBlocked

BETAS = (0.0, 1.0, -2.0, 0.5)
POISON = 1 << 40  # what an interpreter sees in a NaN column: any live term on it wrecks the row
SWEEP_ROWS = [1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 1023, 1025, 2049]

_cache: dict = {}


def cached(key, make):
    """One data set (matrix, x, oracle) is built once and shared, unchanged,
    by the tests and parametrisations that need it."""
    if key not in _cache:
        if len(_cache) > 64:
            _cache.clear()
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ generators
def nonzero_ints(rng, n: int) -> np.ndarray:
    """n integers in [-8, 8] without 0."""
    v = rng.integers(1, 9, n)
    return np.where(rng.integers(0, 2, n) == 1, v, -v).astype(np.int64)


def assert_exact(max_row_len: int) -> None:
    assert 64 * int(max_row_len) + 128 < 2 ** 24, "row too long for exact float32 sums"


def int_csr(lens, ncols: int, seed: int = 0, cols=None) -> CSR:
    """CSR with the given row lengths, integer values, columns in
    [1, ncols - 2] (all 0 when ncols < 3), unsorted inside a row."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, dtype=np.int64)
    assert_exact(lens.max(initial=0))
    nnz = int(lens.sum())
    if cols is None:
        cols = rng.integers(1, ncols - 1, nnz) if ncols >= 3 else np.zeros(nnz, dtype=np.int64)
    rp = np.concatenate([[0], np.cumsum(lens)])
    return CSR(lens.size, ncols, torch.from_numpy(rp.astype(np.int32)),
               torch.from_numpy(np.asarray(cols).astype(np.int32)),
               torch.from_numpy(nonzero_ints(rng, nnz).astype(np.float32)))


def int_x(ncols: int, used: np.ndarray, seed: int = 0) -> torch.Tensor:
    """float32 x: nonzero integers at the ``used`` columns, NaN elsewhere."""
    rng = np.random.default_rng(seed + 1000)
    x = np.full(ncols, np.nan, dtype=np.float32)
    used = np.unique(np.asarray(used, dtype=np.int64))
    x[used] = nonzero_ints(rng, used.size).astype(np.float32)
    return torch.from_numpy(x)


def x_for(a: CSR, seed: int = 0) -> torch.Tensor:
    x = int_x(a.ncols, a.col.numpy(), seed)
    if a.ncols >= 3:
        assert bool(torch.isnan(x[0])) and bool(torch.isnan(x[-1]))
    return x


def int_y0(nrows: int, seed: int = 0) -> torch.Tensor:
    """Even integers in [-64, 64]: beta * y0 is an integer for every beta of BETAS."""
    rng = np.random.default_rng(seed + 2000)
    return torch.from_numpy((2 * rng.integers(-32, 33, nrows)).astype(np.float32))


def x_int(x: torch.Tensor) -> np.ndarray:
    """x as int64 for the interpreters: NaN becomes POISON."""
    xf = x.numpy().astype(np.float64)
    nan = np.isnan(xf)
    xi = np.where(nan, 0.0, xf)
    assert np.all(xi == np.rint(xi))
    return np.where(nan, POISON, xi.astype(np.int64))


def _ints(t: torch.Tensor) -> np.ndarray:
    v = t.cpu().numpy().astype(np.float64)
    assert np.all(v == np.rint(v))
    return v.astype(np.int64)


def row_ids(rp: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


# ------------------------------------------------- int64 format interpreters
def interp_csr(a: CSR, xi: np.ndarray) -> np.ndarray:
    """The CSR oracle: y[r] = sum over [rp[r], rp[r+1]) of val * x[col]."""
    rp = a.rp.cpu().numpy().astype(np.int64)
    assert rp[0] == 0 and rp[-1] == a.col.numel() == a.val.numel() and np.all(np.diff(rp) >= 0)
    col = a.col.cpu().numpy().astype(np.int64)
    assert col.size == 0 or (col.min() >= 0 and col.max() < a.ncols)
    y = np.zeros(a.nrows, dtype=np.int64)
    np.add.at(y, row_ids(rp), _ints(a.val) * xi[col])
    return y


def interp_csr_aligned(a: CSRAligned, xi: np.ndarray) -> np.ndarray:
    """Aligned CSR as its kernel reads it: whole 4-entry pieces per row."""
    rp = a.rp.cpu().numpy().astype(np.int64)
    assert np.all(rp % 4 == 0) and rp[-1] == a.col.numel() == a.val.numel()
    col = a.col.cpu().numpy().astype(np.int64).reshape(-1, 4)
    assert col.size == 0 or (col.min() >= 0 and col.max() < a.ncols)
    piece = (_ints(a.val).reshape(-1, 4) * xi[col]).sum(1)
    y = np.zeros(a.nrows, dtype=np.int64)
    np.add.at(y, row_ids(rp // 4), piece)
    return y


def interp_colblocked(a: CSRColBlocked, xi: np.ndarray) -> np.ndarray:
    y = np.zeros(a.nrows, dtype=np.int64)
    assert a.col0[0] == 0 and len(a.col0) == len(a.blocks)
    for c0, b in zip(a.col0, a.blocks):
        assert b.nrows == a.nrows and 0 <= c0 and c0 + b.ncols <= a.ncols
        xs = xi[c0:c0 + b.ncols]
        y += interp_csr_aligned(b, xs) if isinstance(b, CSRAligned) else interp_csr(b, xs)
    assert a.col0[-1] + a.blocks[-1].ncols == a.ncols
    return y


def interp_ell(a: ELL, xi: np.ndarray) -> np.ndarray:
    """Column-major [K, nrows]; col < 0 is padding and reads nothing."""
    col = a.col.cpu().numpy().astype(np.int64).reshape(a.K, a.nrows)
    val = _ints(a.val).reshape(a.K, a.nrows)
    live = col >= 0
    assert np.all(col[live] < a.ncols)
    xs = np.zeros(col.shape, dtype=np.int64)
    xs[live] = xi[col[live]]
    return (val * xs * live).sum(0) if a.K else np.zeros(a.nrows, dtype=np.int64)


def interp_coo(a: COO, xi: np.ndarray) -> np.ndarray:
    row = a.row.cpu().numpy().astype(np.int64)
    assert np.all(np.diff(row) >= 0), "COO rows must be sorted"
    y = np.zeros(a.nrows, dtype=np.int64)
    np.add.at(y, row, _ints(a.val) * xi[a.col.cpu().numpy().astype(np.int64)])
    return y


def interp_hyb(a: HYB, xi: np.ndarray) -> np.ndarray:
    return interp_ell(a.ell, xi) + interp_coo(a.coo, xi)


def interp_dia(a: DIA, xi: np.ndarray) -> np.ndarray:
    """data[d * nrows + r] = A[r, r + off[d]]; slots whose column is out of
    range are not part of the matrix (shifted slices, no clamped reads)."""
    off = a.offsets.cpu().numpy().astype(np.int64)
    data = _ints(a.data).reshape(off.size, a.nrows)
    y = np.zeros(a.nrows, dtype=np.int64)
    for d, o in enumerate(off):
        lo, hi = max(0, -o), min(a.nrows, a.ncols - o)  # rows r with 0 <= r + o < ncols
        if lo < hi:
            y[lo:hi] += data[d, lo:hi] * xi[lo + o:hi + o]
    return y


INTERP = {CSRAligned: interp_csr_aligned, CSR: interp_csr, CSRColBlocked: interp_colblocked, ELL: interp_ell,
          COO: interp_coo, HYB: interp_hyb, DIA: interp_dia}


def interp(m, xi: np.ndarray) -> np.ndarray:
    return INTERP[type(m)](m, xi)


# ----------------------------------------------------------------- the oracle
def expected(ax: np.ndarray, beta: float, y0: torch.Tensor | None) -> torch.Tensor:
    """float32 A x + beta * y0 from the int64 product ``ax``; exact."""
    assert beta in BETAS
    y = ax.copy()
    if beta != 0.0:
        h = _ints(y0) // 2  # y0 is even
        assert np.all(2 * h == _ints(y0))
        y = y + int(round(2 * beta)) * h
    assert np.abs(y).max(initial=0) < 2 ** 24
    return torch.from_numpy(y.astype(np.float32))


def nan_y(nrows: int, dev) -> torch.Tensor:
    return torch.full((nrows,), float("nan"), dtype=torch.float32, device=dev)


def assert_same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got = got.detach().cpu()
    if torch.equal(got, want):
        return
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    bad = np.flatnonzero(~((got == want).numpy()))
    show = ", ".join(f"y[{i}] = {got[i].item()} != {want[i].item()}" for i in bad[:6])
    raise AssertionError(f"{what}: {bad.size} of {want.numel()} rows differ: {show}")


def check_exact(run, ax: np.ndarray, x: torch.Tensor, dev, what: str, betas=(0.0, 0.5), seed: int = 0) -> None:
    """``run(x_dev, y_dev, beta)`` computes y = A x + beta y in place (or
    returns the result); beta == 0 starts from NaN, the others from y0."""
    nrows = ax.size
    xd = x.to(dev)
    for beta in betas:
        y0 = None if beta == 0.0 else int_y0(nrows, seed)
        yd = nan_y(nrows, dev) if y0 is None else y0.clone().to(dev)
        out = run(xd, yd, beta)
        assert_same(yd if out is None else out, expected(ax, beta, y0), f"{what}, beta = {beta}")


def beta_pair(i: int) -> tuple:
    """beta = 0 and one nonzero beta, rotating through 1, -2, 0.5."""
    return (0.0, BETAS[1 + i % 3])


# ------------------------------------------------------------- DIA, hand-built
def int_dia(nrows: int, ncols: int, offsets, seed: int = 0, garbage: float = 7.0):
    """(DIA, x, int64 A x): every in-range slot holds a nonzero integer, every
    out-of-range slot ``garbage``; x is NaN in the columns no slot reaches."""
    rng = np.random.default_rng(seed)
    off = np.asarray(offsets, dtype=np.int64)
    assert np.unique(off).size == off.size
    assert_exact(off.size)
    r = np.arange(nrows, dtype=np.int64)
    c = r[None, :] + off[:, None]
    live = (c >= 0) & (c < ncols)
    data = np.where(live, nonzero_ints(rng, live.size).reshape(live.shape), int(garbage))
    x = int_x(ncols, c[live], seed)
    a = DIA(nrows, ncols, torch.from_numpy(off.astype(np.int32)), torch.from_numpy(data.astype(np.float32).ravel()))
    xi = x_int(x)
    ax = np.where(live, data * xi[np.clip(c, 0, max(ncols - 1, 0))], 0).sum(0)
    assert np.array_equal(ax, interp_dia(a, xi))
    return a, x, ax


def csr_of_dia(d: DIA) -> CSR:
    """The in-range slots of a DIA as CSR entries, row by row."""
    off = d.offsets.numpy().astype(np.int64)
    c = np.arange(d.nrows, dtype=np.int64)[:, None] + off[None, :]
    live = (c >= 0) & (c < d.ncols)
    rp = np.concatenate([[0], np.cumsum(live.sum(1))])
    val = d.data.numpy().reshape(off.size, d.nrows).T[live]
    return CSR(d.nrows, d.ncols, torch.from_numpy(rp.astype(np.int32)), torch.from_numpy(c[live].astype(np.int32)),
               torch.from_numpy(val.copy()))


def dia_offsets(nrows: int, ncols: int, ndiag: int, seed: int = 0) -> np.ndarray:
    """ndiag distinct offsets: the main diagonal and its neighbours and, from
    4 diagonals, one wholly out of range on each side (clamped reads only)
    and ones that lie mostly out of range (1 or 2 live slots at a corner)."""
    rng = np.random.default_rng(seed)
    edge = [-(nrows + 5), ncols + 3, 0, -(nrows - 1), ncols - 1, 1, -1, -(nrows - 2), ncols - 2]
    pick = []
    for o in ([0] if ndiag < 4 else edge) + [0, 1, -1, 2, -3]:
        if o not in pick and len(pick) < ndiag:
            pick.append(o)
    pool = [o for o in range(-(nrows - 1), ncols) if o not in pick]
    if len(pick) < ndiag:
        pick += list(rng.choice(pool, ndiag - len(pick), replace=False))
    return np.sort(np.asarray(pick, dtype=np.int64))


# ------------------------------------------------------------ the float bound
def float_reference(rows: np.ndarray, val: np.ndarray, xg: np.ndarray, nrows: int, stored: np.ndarray,
                    beta: float = 0.0, y0: np.ndarray | None = None):
    """(y64, bound): the fp64 product and the worst-case float32 error of a
    row of L stored terms (padding included), in any summation order, fused or
    not: |y - y64| <= (L + 3) * 2**-24 * (sum |v_j x_j| + |beta * y0|). The
    L + 1 products (beta * y0 among them) and the L additions each round once
    (u = 2**-24), so every term is perturbed by at most L + 2 roundings:
    (L + 2) u to first order, gamma_(L + 2) = (L + 2) u / (1 - (L + 2) u) in
    full, which stays below (L + 3) u up to L = 4000 and exceeds it by a
    factor of 1.0003 at most for the longest row used (6603 entries, ELL)."""
    t = val.astype(np.float64) * xg.astype(np.float64)
    y64 = np.zeros(nrows)
    mag = np.zeros(nrows)
    np.add.at(y64, rows, t)
    np.add.at(mag, rows, np.abs(t))
    if beta != 0.0:
        y64 += beta * y0.astype(np.float64)
        mag += np.abs(beta * y0.astype(np.float64))
    return y64, (stored.astype(np.float64) + 3) * 2.0 ** -24 * mag


def stored_terms(m) -> np.ndarray:
    """Stored terms per row of a format, padding included."""
    if isinstance(m, CSRColBlocked):
        return sum(stored_terms(b) for b in m.blocks) + len(m.blocks)  # + one addition per block
    if isinstance(m, CSR):
        return np.diff(m.rp.cpu().numpy().astype(np.int64))
    if isinstance(m, ELL):
        return np.full(m.nrows, m.K, dtype=np.int64)
    if isinstance(m, DIA):
        return np.full(m.nrows, m.offsets.numel(), dtype=np.int64)
    if isinstance(m, COO):
        return np.bincount(m.row.cpu().numpy().astype(np.int64), minlength=m.nrows)
    if isinstance(m, HYB):
        return stored_terms(m.ell) + stored_terms(m.coo) + 1
    raise TypeError(type(m))
