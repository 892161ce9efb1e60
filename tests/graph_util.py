"""Generator, oracles and error bound of test_pagerank_exact.py. Plain numpy:
apart from the ``CSRGraph`` container nothing here calls a ``cme213x`` op.

One sweep is ``out[i] = c + 0.5 * sum_{j in row i} x[e_j] * inv[e_j]`` with
``c = fl(0.5f / (float)n)``, and the prescaled kernels also emit
``y_next = out * inv``.

Exact tier. ``x`` is drawn from {1..15}/16 (never zero: a dropped or an extra
gathered term always changes the sum) and ``inv_deg`` from {1, 1/2, 1/4, 1/8}
(deliberately NOT the inverse out-degree: the kernels treat it as an arbitrary
array). Every product ``x * inv`` is then an exact multiple of 2**-7 below 1,
and as long as a row's sum stays below 2**24 units of 2**-7 (asserted by the
oracle) every partial sum, in any order and any grouping, is exactly
representable in float32. ``0.5 * sum`` is exact, so a sweep has ONE rounding,
``fl(c + 0.5 * sum)``, and ``out * inv`` (a power of two) is exact again: every
kernel, whatever its summation order, must equal the int64 oracle bit for bit.
"""
import numpy as np
import torch

from cme213x.ops.graph import CSRGraph

U = 2.0 ** -24  # float32 unit roundoff
MIXED_LENS = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 200)

_cache: dict = {}


def cached(key, make):
    """One data set (graph, x, oracle) is built once and shared, unchanged, by
    the tests and parametrisations that need it."""
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ------------------------------------------------------------------ generators
def int_graph(row_lens, n: int, seed: int = 0, allowed=None) -> CSRGraph:
    """CSR graph of ``n`` nodes with the given row lengths (zero included).
    Targets are uniform over ``allowed`` (default: all of [0, n)); on top of
    that every third non-empty row starts with a self-loop, every other row
    of two or more edges repeats its first target, and rows of three or more
    edges end in node 0 or node n - 1 alternately (each only where ``allowed``
    admits it). ``inv_deg`` is drawn from {1, 1/2, 1/4, 1/8}."""
    rng = np.random.default_rng(seed)
    lens = np.asarray(row_lens, dtype=np.int64)
    assert lens.shape == (n,) and lens.min(initial=0) >= 0
    allowed = np.arange(n, dtype=np.int64) if allowed is None else np.asarray(allowed, dtype=np.int64)
    ok = np.zeros(max(n, 1), dtype=bool)
    ok[allowed] = True
    rp = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    nnz = int(rp[-1])
    edges = allowed[rng.integers(0, allowed.size, nnz)] if nnz else np.zeros(0, dtype=np.int64)
    rows = np.flatnonzero(lens > 0)
    for k, r in enumerate(rows):
        b, e = rp[r], rp[r + 1]
        if k % 3 == 0 and ok[r]:
            edges[b] = r  # self-loop
        if e - b >= 2 and k % 2 == 0:
            edges[b + 1] = edges[b]  # duplicate target inside the row
        if e - b >= 3:
            t = 0 if k % 4 < 2 else n - 1
            if ok[t]:
                edges[e - 1] = t
    assert edges.size == 0 or (edges.min() >= 0 and edges.max() < n)
    inv = (2.0 ** -rng.integers(0, 4, n)).astype(np.float32)
    return CSRGraph(torch.from_numpy(rp.astype(np.int32)), torch.from_numpy(edges.astype(np.int32)),
                    torch.from_numpy(inv))


def int_x(n: int, seed: int = 0) -> torch.Tensor:
    """float32 x from {1..15}/16."""
    rng = np.random.default_rng(seed + 1000)
    return torch.from_numpy((rng.integers(1, 16, n) / 16.0).astype(np.float32))


def mixed_lens(n: int, seed: int = 0) -> np.ndarray:
    """``n`` row lengths cycling through MIXED_LENS in shuffled order; from
    three rows on, the first and the last row are empty."""
    rng = np.random.default_rng(seed + 2000)
    reps = -(-n // len(MIXED_LENS))
    lens = np.concatenate([rng.permutation(MIXED_LENS) for _ in range(reps)])[:n].astype(np.int64)
    if n >= 3:
        lens[0] = lens[-1] = 0
    elif lens.sum() == 0:
        lens[0] = 5
    return lens


def true_inverse(g: CSRGraph) -> CSRGraph:
    """``g`` with the reference generator's ``inv_deg = 1 / row length`` (1
    for an empty row)."""
    deg = np.diff(g.indices.numpy().astype(np.int64))
    inv = (1.0 / np.maximum(deg, 1).astype(np.float32)).astype(np.float32)
    return CSRGraph(g.indices, g.edges, torch.from_numpy(inv))


def mass_graph(n: int, seed: int = 0) -> CSRGraph:
    """A graph on which a sweep conserves ``sum(x)``: node v is gathered by
    ``k_v`` edges, ``k_v`` in {1, 2, 4, 8} (never 0), and ``inv_deg[v] = 1 / k_v``
    exactly, so ``sum(out) = 0.5 + 0.5 * sum_v k_v * x[v] / k_v``. Row lengths
    are uneven and include empty rows."""
    rng = np.random.default_rng(seed)
    k = 2 ** rng.integers(0, 4, n)
    edges = rng.permutation(np.repeat(np.arange(n, dtype=np.int64), k))
    cuts = np.sort(rng.integers(0, edges.size + 1, n - 1))
    rp = np.concatenate([[0], cuts, [edges.size]]).astype(np.int64)
    assert np.array_equal(np.bincount(edges, minlength=n), k)
    return CSRGraph(torch.from_numpy(rp.astype(np.int32)), torch.from_numpy(edges.astype(np.int32)),
                    torch.from_numpy((1.0 / k).astype(np.float32)))


# ----------------------------------------------------------------- the oracles
def _arrays(g: CSRGraph):
    rp = g.indices.cpu().numpy().astype(np.int64)
    edges = g.edges.cpu().numpy().astype(np.int64)
    inv = g.inv_deg.cpu().numpy()
    n = inv.size
    assert rp.shape == (n + 1,) and rp[0] == 0 and rp[-1] == edges.size and np.all(np.diff(rp) >= 0)
    assert edges.size == 0 or (edges.min() >= 0 and edges.max() < n)
    return rp, edges, inv, n


def row_ids(rp: np.ndarray) -> np.ndarray:
    return np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))


def longest_row(g: CSRGraph) -> int:
    return int(np.diff(g.indices.cpu().numpy().astype(np.int64)).max(initial=0))


def exact_sweep(g: CSRGraph, x: torch.Tensor):
    """(out, y_next) of one sweep as float32 tensors, exactly: row sums in
    int64 units of 2**-7, then the sweep's single float32 rounding."""
    rp, edges, inv, n = _arrays(g)
    xu = x.numpy().astype(np.float64) * 16
    iu = inv.astype(np.float64) * 8
    assert x.dtype == torch.float32 and x.shape == (n,)
    assert np.all(xu == np.rint(xu)) and np.all((xu >= 1) & (xu <= 15)), "x must come from {1..15}/16"
    assert np.all(np.isin(iu, (1, 2, 4, 8))), "inv_deg must come from {1, 1/2, 1/4, 1/8}"
    yu = xu.astype(np.int64) * iu.astype(np.int64)  # units of 2**-7, at most 120
    s = np.zeros(n, dtype=np.int64)
    np.add.at(s, row_ids(rp), yu[edges])
    # exactness precondition: (max row sum) * 2**7 < 2**24, so that every
    # partial sum of every row, in any order, is a float32
    assert s.max(initial=0) < 2 ** 24, "row sum too large for exact float32 sums"
    half_sum = s.astype(np.float32) * np.float32(2.0 ** -8)  # 0.5 * sum: exact
    assert np.array_equal(half_sum.astype(np.float64) * 256, s)
    if n == 0:
        return torch.zeros(0), torch.zeros(0)
    c = np.float32(0.5) / np.float32(n)
    out = (c + half_sum).astype(np.float32)  # the one rounding
    assert out.dtype == np.float32
    y = out * inv
    assert np.array_equal(y.astype(np.float64), out.astype(np.float64) * inv.astype(np.float64))  # exact
    return torch.from_numpy(out), torch.from_numpy(y)


def sweeps64(g: CSRGraph, x0: torch.Tensor, sweeps: int) -> np.ndarray:
    """float64 reference of ``sweeps`` sweeps from the float32 ``x0`` (with the
    real-valued constant 0.5 / n)."""
    rp, edges, inv, n = _arrays(g)
    rows = row_ids(rp)
    inv = inv.astype(np.float64)
    x = x0.cpu().numpy().astype(np.float64)
    for _ in range(sweeps):
        y = x * inv
        s = np.zeros(n)
        np.add.at(s, rows, y[edges])
        x = 0.5 / n + 0.5 * s
    return x


def sweep_bound(g: CSRGraph, sweeps: int) -> float:
    """Relative error bound of the float32 result of ``sweeps`` sweeps against
    :func:`sweeps64`, elementwise: ``sweeps * (L + 3) * 2**-24``, L the
    longest row.

    Derivation. Every quantity is positive, so relative errors never amplify:
    a sum of positive terms with relative errors <= e has a relative error
    <= e. One sweep, from inputs with relative error e, computes for a row of
    l <= L terms
      * the products ``x * inv`` (prescale kernel, or per edge in the
        reference kernel and on the CPU): one rounding each;
      * their sum, in ANY order or grouping (lane groups, column blocks,
        additions of 0 are exact): at most l - 1 <= L - 1 roundings on the
        path of one term;
      * ``0.5 * sum``: exact in binary floating point, but charged one
        rounding all the same;
      * ``c = fl(0.5f / n)``: one rounding, on the constant's path only;
      * the final addition: one rounding.
    Charging the prescale product, the ``0.5 * sum`` term and the final add
    (the + 3) on top of L for the sum, the sweep's output has relative error
    <= e + (L + 3) u to first order, u = 2**-24, and after s sweeps
    s (L + 3) u. That is rigorous, not only first order: a term's path really
    holds at most m = max(L + 1, 2) factors (1 + d) per sweep (the sum has
    L - 1, ``0.5 * sum`` none), so the exact bound is
    (1 + u)**(s m) - 1 <= k / (1 - k) with k = s m u, and the two spare
    roundings per sweep cover the difference (asserted below) as well as the
    float64 reference's own rounding, about s (L + 3) 2**-53."""
    L = longest_row(g)
    b = sweeps * (L + 3) * U
    k = sweeps * max(L + 1, 2) * U
    assert k / (1 - k) + sweeps * (L + 3) * 2.0 ** -52 < b
    return b


def assert_within(got, ref64: np.ndarray, bound: float, what: str) -> float:
    """|got - ref64| <= bound * ref64 elementwise; returns the worst ratio."""
    got = got.detach().cpu().numpy().astype(np.float64) if isinstance(got, torch.Tensor) else got.astype(np.float64)
    assert got.shape == ref64.shape, f"{what}: shape {got.shape} != {ref64.shape}"
    assert np.all(ref64 > 0)
    rel = np.abs(got - ref64) / ref64
    worst = float(rel.max(initial=0.0))
    i = int(rel.argmax()) if rel.size else -1
    assert worst <= bound, f"{what}: relative error {worst:.3e} > bound {bound:.3e} at node {i}"
    return worst


def assert_same(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    if torch.equal(got, want):
        return
    bad = np.flatnonzero(~((got == want).numpy()))
    show = ", ".join(f"[{i}] = {got[i].item()!r} != {want[i].item()!r}" for i in bad[:6])
    raise AssertionError(f"{what}: {bad.size} of {want.numel()} nodes differ: {show}")


# -------------------------------------------------------- block_columns oracle
def blocked_oracle(g: CSRGraph, blocks: int):
    """(rp, edges) of the column-blocked copy by a numpy stable sort of the
    (block, row) keys."""
    rp, edges, _, n = _arrays(g)
    bs = -(-n // blocks)
    key = (edges // bs) * n + row_ids(rp)
    order = np.argsort(key, kind="stable")
    counts = np.bincount(key, minlength=blocks * n)
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), edges[order]
