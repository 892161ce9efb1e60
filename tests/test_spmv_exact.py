"""SpMV, exactly: every kernel instantiation of csrc/hip/spmv.hip and every
host-side format conversion against an int64 numpy oracle, bit for bit, on
integer-valued data with NaN wherever only a padding read or a ``0 * y`` would
look (generators, interpreters and the derived float bound: spmv_util.py).

Unmarked tests run the pure-numpy format interpreters and the CPU backend;
``gpu`` tests run the HIP kernels. Unless a test says otherwise it runs
beta = 0 on a NaN-filled y and one nonzero beta out of {1, -2, 0.5}.
"""
import contextlib

import numpy as np
import pytest
import spmv_util as U
import torch

from cme213x import _ext
from cme213x.ops.spmv import (CSR, DIA, CSRAligned, hyb_k, laplacian, prepare, random_csr, spmv, to_coo,
                               to_csr_aligned, to_csr_colblocked, to_dia, to_ell, to_hyb)

CPU = torch.device("cpu")
HIP_INVALID_VALUE = 1  # hipErrorInvalidValue


# ------------------------------------------------------------------ data sets
def case(key, make_lens, ncols, seed=0, cols=None):
    """(CSR on the host, x, int64 A x), cached by key."""
    def make():
        a = U.int_csr(make_lens(np.random.default_rng(seed + 77)), ncols, seed, cols)
        x = U.x_for(a, seed)
        return a, x, U.interp_csr(a, U.x_int(x))
    return U.cached(key, make)


def sweep_case(nrows):
    return case(("sweep", nrows), lambda rng: rng.integers(0, 10, nrows), 97, seed=nrows)


def spread(rng, total, nrows):
    """``nrows`` row lengths that add up to ``total``, uneven."""
    lens = np.full(nrows, total // nrows, dtype=np.int64)
    lens[:total % nrows] += 1
    for _ in range(nrows // 2):  # move entries between random pairs of rows
        i, j = rng.integers(0, nrows, 2)
        k = int(rng.integers(0, lens[i] + 1))
        lens[i] -= k
        lens[j] += k
    assert lens.sum() == total and lens.min() >= 0
    return lens


def single(total, nrows, at):
    lens = np.zeros(nrows, dtype=np.int64)
    lens[at] = total
    return lens


def run_spmv(m, kernel="auto"):
    return lambda xd, yd, beta: spmv(m, xd, yd, kernel=kernel, beta=beta)


def knobs(**kw):
    from cme213x.utils import tuning

    return tuning.override(**kw) if kw else contextlib.nullcontext()


def to_format(a: CSR, fmt: str):
    return {"csr_aligned": to_csr_aligned, "ell": lambda m: to_ell(m)[0], "coo": to_coo, "hyb": to_hyb,
            "dia": to_dia, "csr_cb": lambda m: to_csr_colblocked(m, block_bytes=64),
            "csr_cb_u": lambda m: to_csr_colblocked(m, block_bytes=64, aligned=False)}.get(fmt, lambda m: m)(a)


CSR_KERNELS = ["scalar", "vector", "stream", "short", "wave"]


def dia_x(d: DIA, seed=0):
    """x for a DIA from ``to_dia``: finite on every column an in-range slot
    lies on (DIA multiplies its explicit zeros), NaN elsewhere."""
    off = d.offsets.numpy().astype(np.int64)
    c = np.arange(d.nrows, dtype=np.int64)[None, :] + off[:, None]
    return U.int_x(d.ncols, c[(c >= 0) & (c < d.ncols)], seed)


# ================================================================= CPU: formats
LONG = ("long", lambda rng: np.concatenate([rng.integers(0, 40, 5001), [9000, 4097]])[rng.permutation(5003)], 7000)
MIXED = ("mixed", lambda rng: rng.integers(0, 10, 300), 97)
EMPTYISH = ("emptyish", lambda rng: rng.integers(0, 3, 515) * rng.integers(0, 2, 515), 40)


@pytest.mark.parametrize("which,fmt", [(w, f) for w in (LONG, MIXED, EMPTYISH)
                                       for f in ("csr_aligned", "ell", "coo", "hyb", "hyb_k3", "dia", "csr_cb", "csr_cb_u")
                                       if (w, f) != (LONG, "ell")],  # 9000 x 5003 slots
                         ids=lambda v: v if isinstance(v, str) else v[0])
def test_interpreters_match_csr_oracle(which, fmt):
    """Every conversion keeps the matrix: its arrays, read by a numpy
    interpreter of the format, give the CSR oracle's int64 product."""
    a, x, ax = case(*which)
    if fmt == "dia":
        if which is LONG:  # ~12000 diagonals: not a DIA matrix
            with pytest.raises(ValueError):
                to_dia(a)
            return
        m = to_dia(a)
        x = dia_x(m)
        ax = U.interp_csr(a, U.x_int(x))
    elif fmt == "hyb_k3":
        m = to_hyb(a, K=3)
        assert m.ell.K == 3 and m.coo.nnz == int(np.maximum(np.diff(a.rp.numpy()) - 3, 0).sum())
    elif fmt.startswith("csr_cb"):
        m = to_csr_colblocked(a, block_bytes=4096 if which is LONG else 64, aligned=fmt == "csr_cb")
        assert len(m.blocks) == -(-4 * a.ncols // (4096 if which is LONG else 64))
    else:
        m = to_format(a, fmt)
    assert np.array_equal(U.interp(m, U.x_int(x)), ax)
    if fmt == "hyb" and which is LONG:
        assert m.ell.K == hyb_k(a) > 0 and m.coo.nnz > 0
    if fmt == "csr_aligned":  # padding: value 0 on a column of the same row
        assert m.nnz - a.nnz == int(((-np.diff(a.rp.numpy())) % 4).sum())
    if fmt == "ell":
        assert m.K == int(np.diff(a.rp.numpy()).max()) and int((m.col >= 0).sum()) == a.nnz


def test_to_dia_rectangular_65_diagonals():
    """to_dia on 1000 x 1300 with 65 occupied diagonals (the kernel's
    global-memory offset path) and on a tall matrix."""
    for nrows, ncols in ((1000, 1300), (700, 520)):
        d0, _, _ = U.int_dia(nrows, ncols, np.arange(-32, 33) * 3, seed=5, garbage=0.0)
        a = U.csr_of_dia(d0)
        d = to_dia(a)
        assert d.offsets.numel() == 65 and torch.equal(d.offsets, d0.offsets) and torch.equal(d.data, d0.data)
        x = dia_x(d)
        assert np.array_equal(U.interp_dia(d, U.x_int(x)), U.interp_csr(a, U.x_int(x)))


def test_zero_row_conversions():
    """A matrix without rows converts to every format (ELL / HYB with K = 0)."""
    a = CSR(0, 5, torch.zeros(1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    assert hyb_k(a) == 0
    ell, rest = to_ell(a)
    assert ell.K == 0 and ell.col.numel() == 0 and rest.nnz == 0
    assert to_hyb(a).ell.K == 0 and to_coo(a).nnz == 0 and to_dia(a).offsets.numel() == 0
    assert to_csr_aligned(a).nnz == 0 and len(to_csr_colblocked(a, block_bytes=8).blocks) == 3
    for fmt in ("csr_aligned", "ell", "coo", "hyb", "dia", "csr_cb"):
        assert U.interp(to_format(a, fmt), np.zeros(5, dtype=np.int64)).size == 0
    assert to_hyb(sweep_case(300)[0]).ell.K == 0  # below 4096 rows HYB is all COO


# ============================================================ CPU backend, exact
@pytest.mark.parametrize("nrows", U.SWEEP_ROWS)
def test_cpu_backend_sweep(nrows):
    a, x, ax = sweep_case(nrows)
    U.check_exact(run_spmv(a), ax, x, CPU, f"cpu, {nrows} rows", U.BETAS, seed=nrows)


def test_cpu_backend_long_rows_and_aligned():
    a, x, ax = case(*LONG)
    U.check_exact(run_spmv(a), ax, x, CPU, "cpu, long rows", U.BETAS)
    U.check_exact(run_spmv(to_csr_aligned(a)), ax, x, CPU, "cpu, aligned CSR", (0.0, -2.0))


# ================================================================== degenerate
def degenerate(kind):
    if kind == "no_rows":
        a = CSR(0, 5, torch.zeros(1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    elif kind == "all_empty":
        a = U.int_csr(np.zeros(300, dtype=np.int64), 40)
    else:  # one column: every entry on column 0, x[0] a real value
        a = U.int_csr(np.random.default_rng(3).integers(0, 4, 300), 1)
    x = U.x_for(a)
    return a, x, U.interp_csr(a, U.x_int(x))


@pytest.mark.parametrize("kind", ["no_rows", "all_empty", "one_col"])
def test_degenerate_cpu(kind):
    a, x, ax = degenerate(kind)
    U.check_exact(run_spmv(a), ax, x, CPU, kind, U.BETAS)
    assert spmv(a, x).shape == (a.nrows,)
    if kind == "all_empty":
        assert bool(torch.isnan(x).all()) and not ax.any()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["no_rows", "all_empty", "one_col"])
def test_degenerate_gpu(gpu, kind):
    """No rows (no launch: a zero-size grid is an error), only empty rows
    (y = beta * y0; 0 over a NaN y when beta is 0; K = 0 ELL, 0 diagonals),
    a single column; every kernel and format."""
    a, x, ax = degenerate(kind)
    dev = a.to(gpu)
    for i, kernel in enumerate(CSR_KERNELS + ["auto"]):
        U.check_exact(run_spmv(dev, kernel), ax, x, gpu, f"{kind}, {kernel}", U.beta_pair(i))
    for i, fmt in enumerate(["csr_aligned", "ell", "coo", "hyb", "dia", "csr_cb", "csr_cb_u"]):
        m = to_format(a, fmt)
        assert np.array_equal(U.interp(m, U.x_int(x)), ax)
        U.check_exact(run_spmv(m.to(gpu)), ax, x, gpu, f"{kind}, {fmt}", U.beta_pair(i))
    assert spmv(dev, x.to(gpu)).shape == (a.nrows,)


# ============================================= every instantiation, via the C ABI
GROUPS = [1, 2, 4, 8, 16, 32, 64]


def group_case(G):
    return case(("group", G), lambda rng: np.resize([0, 1, G - 1, G, G + 1, 4 * G - 1, 4 * G + 1, 300, 0, 2],
                                                    257)[rng.permutation(257)], 331, seed=G)


def call_csr(name, m, group, stream):
    nnz = (m.nnz,) if name == "cme_spmv_csr_aligned" else ()

    def run(xd, yd, beta):
        return _ext._fn("hip", name)(m.nrows, *nnz, m.rp.data_ptr(), m.col.data_ptr(), m.val.data_ptr(),
                                     xd.data_ptr(), yd.data_ptr(), group, float(beta), stream)
    return run


@pytest.mark.gpu
@pytest.mark.parametrize("G", GROUPS)
@pytest.mark.parametrize("entry", ["csr", "aligned_plain", "aligned_nt"])
def test_every_group_instantiation(gpu, entry, G):
    """cme_spmv_csr (csr_scalar_kernel, csr_vector_kernel<2..64>) and
    cme_spmv_csr_aligned (csr_vec4_kernel<1..64, NT and plain>; 32 and 64 are
    out of spmv()'s reach) on 257 rows -- 257 * G is no multiple of 256, so the
    last group straddles the grid's end -- of 0, 1, G - 1, G, G + 1, 4G +- 1
    and 300 entries."""
    a, x, ax = group_case(G)
    m = (a if entry == "csr" else to_csr_aligned(a)).to(gpu)
    name = "cme_spmv_csr" if entry == "csr" else "cme_spmv_csr_aligned"
    run = call_csr(name, m, G, _ext.stream_ptr(gpu))

    def checked(xd, yd, beta):
        assert run(xd, yd, beta) == 0

    with knobs(spmv_nt=int(entry == "aligned_nt")) if entry != "csr" else contextlib.nullcontext():
        U.check_exact(checked, ax, x, gpu, f"{name}, group {G}", U.beta_pair(G.bit_length()), seed=G)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["cme_spmv_csr", "cme_spmv_csr_aligned"])
@pytest.mark.parametrize("group", [3, 128, 0])
def test_unknown_group_is_refused(gpu, entry, group):
    a, x, _ = group_case(4)
    m = (a if entry == "cme_spmv_csr" else to_csr_aligned(a)).to(gpu)
    y = torch.full((a.nrows,), 5.0, device=gpu)
    assert call_csr(entry, m, group, _ext.stream_ptr(gpu))(x.to(gpu), y, 0.0) == HIP_INVALID_VALUE
    torch.cuda.synchronize()
    assert bool((y == 5.0).all())


# ================================================================ row-count sweep
@pytest.mark.gpu
@pytest.mark.parametrize("nrows", U.SWEEP_ROWS)
@pytest.mark.parametrize("what", CSR_KERNELS + ["csr_aligned", "ell", "coo"])
def test_row_count_sweep(gpu, what, nrows):
    """Row counts round a wave (64), a block (256, 512, 1024) and two blocks."""
    a, x, ax = sweep_case(nrows)
    kernel = what if what in CSR_KERNELS else "auto"
    U.check_exact(run_spmv(to_format(a, what).to(gpu), kernel), ax, x, gpu, f"{what}, {nrows} rows",
                  U.beta_pair(nrows), seed=nrows)


@pytest.mark.gpu
@pytest.mark.parametrize("rpt", [1, 2, 4])
@pytest.mark.parametrize("d", [-1, 0, 1])
def test_short_block_edges(gpu, rpt, d):
    """csr_short_kernel<1 / 2 / 4> at 256 * rpt - 1, 256 * rpt, 256 * rpt + 1 rows."""
    a, x, ax = sweep_case(256 * rpt + d)
    with knobs(spmv_short_rpt=rpt):
        U.check_exact(run_spmv(a.to(gpu), "short"), ax, x, gpu, f"short, rpt {rpt}", U.beta_pair(rpt + d))


@pytest.mark.gpu
@pytest.mark.parametrize("rpt", [1, 2, 4])
def test_short_row_lengths(gpu, rpt):
    """Rows round the 8-entry batch of CSR-short (0, 1, 7, 8, 9, 16, 17, 100)."""
    a, x, ax = case("shortlens", lambda rng: np.resize([0, 1, 7, 8, 9, 16, 17, 100], 601)[rng.permutation(601)], 203)
    with knobs(spmv_short_rpt=rpt):
        U.check_exact(run_spmv(a.to(gpu), "short"), ax, x, gpu, f"short rows, rpt {rpt}", U.beta_pair(rpt))


@pytest.mark.gpu
@pytest.mark.parametrize("R", [64, 128, 256, 512, 1024])
def test_stream_rows_per_block(gpu, R):
    """csr_stream_kernel<R>, R forced, at R - 1, R, R + 1 and 2R + 3 rows."""
    for i, nrows in enumerate((R - 1, R, R + 1, 2 * R + 3)):
        a, x, ax = sweep_case(nrows)
        with knobs(spmv_stream_rows=R):
            U.check_exact(run_spmv(a.to(gpu), "stream"), ax, x, gpu, f"stream<{R}>, {nrows} rows", U.beta_pair(i))


# ===================================================== CSR-stream range alignment
STREAM_T = [0, 1, 3, 4, 5, 3071, 3072, 3073, 4095, 4096, 4097]


def three_block_case(unit, pre, t, layout):
    """Three blocks of ``unit`` rows: 4k + pre entries, then exactly t (spread
    over the rows or in one row), then a random partial block."""
    def lens(rng):
        first = spread(rng, 4 * 50 + pre, unit)
        mid = spread(rng, t, unit) if layout == "spread" else single(t, unit, 6)
        return np.concatenate([first, mid, rng.integers(0, 10, unit // 2 + 5)])
    return case(("three", unit, pre, t, layout), lens, 97, seed=pre + 4 * t)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["spread", "single"])
@pytest.mark.parametrize("t", STREAM_T)
def test_stream_range_alignment(gpu, t, layout):
    """csr_stream_kernel<64>: block 1's nonzero range starts at base % 4 ==
    pre and holds exactly t entries -- head / body / tail split (a0, a1) at
    every residue, the 3 x 256-piece loop bound (3072) and the 4096-product cap
    (4097 takes the wave-per-row path)."""
    for pre in range(4):
        a, x, ax = three_block_case(64, pre, t, layout)
        assert int(a.rp[64]) % 4 == pre and int(a.rp[128] - a.rp[64]) == t
        with knobs(spmv_stream_rows=64):
            U.check_exact(run_spmv(a.to(gpu), "stream"), ax, x, gpu, f"stream, pre {pre}, t {t}, {layout}",
                          U.beta_pair(pre + t))


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["spread", "single"])
@pytest.mark.parametrize("t", [255, 256, 257, 1023, 1024, 1025])
def test_wave_range_sizes(gpu, t, layout):
    """csr_wave_kernel: a wave's 64 rows hold t entries (the 4 x 64 unrolled
    loop, the 1024-product cap); the last wave is partial."""
    a, x, ax = three_block_case(64, t % 4, t, layout)
    U.check_exact(run_spmv(a.to(gpu), "wave"), ax, x, gpu, f"wave, t {t}, {layout}", U.beta_pair(t))


# ================================================================== ELL and HYB
@pytest.mark.gpu
@pytest.mark.parametrize("K", [4, 5, 6, 7])
def test_ell_natural_width(gpu, K):
    """ELL at K % 4 = 0..3: the 4-wide loop and its masked remainder, with
    NaN at x[0], which every padding slot reads."""
    a, x, ax = case(("ellK", K), lambda rng: np.concatenate([rng.integers(0, K + 1, 299), [K]]), 97, seed=K)
    ell, rest = to_ell(a)
    assert ell.K == K and rest.nnz == 0 and int((ell.col < 0).sum()) > 0
    U.check_exact(run_spmv(ell.to(gpu)), ax, x, gpu, f"ell, K {K}", U.beta_pair(K))


@pytest.mark.gpu
@pytest.mark.parametrize("K", [0, 1, 3, 4, 5, 9, 11])
def test_hyb_forced_width(gpu, K):
    """HYB with K = 0 (all COO: what hyb_k gives below 4096 rows), inside,
    at (9) and past (11) the longest row."""
    a, x, ax = sweep_case(300)
    assert int(np.diff(a.rp.numpy()).max()) == 9
    h = to_hyb(a, K=K)
    assert h.ell.K == K and (h.coo.nnz == 0) == (K >= 9)
    assert np.array_equal(U.interp_hyb(h, U.x_int(x)), ax)
    U.check_exact(run_spmv(h.to(gpu)), ax, x, gpu, f"hyb, K {K}", U.beta_pair(K))


# ========================================================================= COO
def coo_lens(kind, rng):
    if isinstance(kind, int):  # nnz entries over about nnz / 3 rows
        return np.bincount(rng.integers(0, max(1, kind // 3), kind), minlength=max(1, kind // 3))
    return {"lane_ends": np.array([16, 16, 16, 16, 192, 3, 70, 1, 0, 40, 63, 1, 64]),  # ends at lanes 15 / 31 / 47 / 63, entry 255
            "long_row": np.concatenate([rng.integers(0, 5, 40), [2000], rng.integers(0, 5, 40)]),
            "all_ones": np.ones(700, dtype=np.int64),
            "empty_runs": np.concatenate([np.zeros(100, dtype=np.int64), [3, 1], np.zeros(300, dtype=np.int64),
                                          rng.integers(0, 4, 50), np.zeros(70, dtype=np.int64)])}[kind]


@pytest.mark.gpu
@pytest.mark.parametrize("kind", [1, 63, 64, 65, 255, 256, 257, 1023, 1025, "lane_ends", "long_row", "all_ones",
                                  "empty_runs"])
def test_coo(gpu, kind):
    """coo_kernel: entry counts round a round (64), a wave (256) and a block
    (1024); segments that end on a DPP row / bank / wave boundary; one row
    across waves and workgroups; through beta (scale kernel first) and through
    the accumulate flag (no scaling: y += A x)."""
    a, x, ax = case(("coo", kind), lambda rng: coo_lens(kind, rng), 97, seed=len(str(kind)))
    m = to_coo(a).to(gpu)
    U.check_exact(run_spmv(m), ax, x, gpu, f"coo, {kind}", (0.0, 1.0, -2.0, 0.5))

    def accumulate(xd, yd, beta):
        _ext.call_hip("cme_spmv_coo", m.nrows, m.nnz, m.row.data_ptr(), m.col.data_ptr(), m.val.data_ptr(),
                      xd.data_ptr(), yd.data_ptr(), 1.0, 1, _ext.stream_ptr(gpu))
    U.check_exact(accumulate, ax, x, gpu, f"coo accumulate, {kind}", (1.0,))


# ========================================================================= DIA
DIA_SHAPES = [(1, 90), (255, 292), (255, 226), (256, 293), (256, 227), (257, 294), (257, 228), (1028, 1065),
              (1028, 999)]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", DIA_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ndiag", [1, 3, 4, 5, 63, 64, 65, 68])
def test_dia(gpu, ndiag, shape):
    """dia_kernel, wide and tall: the 4-diagonal loop and its remainder,
    offsets from LDS (up to 64) and from global memory (beyond), diagonals
    wholly or mostly out of range whose slots hold a nonzero value that only a
    leaking clamped read would multiply in."""
    nrows, ncols = shape
    a, x, ax = U.cached(("dia", ndiag, shape),
                        lambda: U.int_dia(nrows, ncols, U.dia_offsets(nrows, ncols, ndiag, seed=ndiag), seed=nrows))
    U.check_exact(run_spmv(a.to(gpu)), ax, x, gpu, f"dia, {ndiag} diagonals, {shape}", U.beta_pair(ndiag))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 2])
def test_dia_clamped_reads_find_nan(gpu, mode):
    """No in-range slot lies on column 0 or ncols - 1 (x is NaN there); the
    out-of-range diagonals clamp onto exactly those two."""
    nrows, ncols = 256, 300
    a, x, ax = U.int_dia(nrows, ncols, [-(nrows + 5), -300, 1, 2, 5, 17, ncols + 3, 400], seed=9)
    assert bool(torch.isnan(x[0])) and bool(torch.isnan(x[-1]))
    with knobs(spmv_dia1=mode):
        U.check_exact(run_spmv(a.to(gpu)), ax, x, gpu, f"dia NaN corners, mode {mode}", (0.0, -2.0))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(4, 4), (4, 90), (1024, 1024), (1028, 1028), (1028, 999), (1032, 1032),
                                   (1032, 1100)], ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("ndiag", [5, 65])
def test_dia_four_row_kernel(gpu, ndiag, shape):
    """dia4_kernel forced (spmv_dia1 = 2) at one lane, one block and just
    beyond; the knob's value 1 (one row per lane) gives the same."""
    nrows, ncols = shape
    if ndiag == 65 and nrows == 4:  # a 4 x 4 matrix has 7 diagonals
        ncols = 90
    a, x, ax = U.cached(("dia4", ndiag, nrows, ncols),
                        lambda: U.int_dia(nrows, ncols, U.dia_offsets(nrows, ncols, ndiag, seed=1), seed=nrows + ndiag))
    with knobs(spmv_dia1=2):
        U.check_exact(run_spmv(a.to(gpu)), ax, x, gpu, f"dia4, {ndiag} diagonals, {nrows}x{ncols}",
                      U.beta_pair(ndiag + nrows // 4))


@pytest.mark.gpu
def test_dia_four_row_kernel_unaligned_y_falls_back(gpu):
    """dia4_kernel stores 16 bytes at y + r0: a y that starts 4 bytes off takes the one-row kernel."""
    a, x, ax = U.int_dia(1024, 1024, [-3, 0, 1, 40], seed=2)
    buf = torch.full((1025,), float("nan"), device=gpu)
    with knobs(spmv_dia1=2):
        spmv(a.to(gpu), x.to(gpu), buf[1:])
    U.assert_same(buf[1:], U.expected(ax, 0.0, None), "dia4 on an offset y")


@pytest.mark.gpu
def test_dia_four_row_kernel_by_rule(gpu):
    """4M rows: the launcher's own switch to dia4_kernel. Built on the device
    (48 MB of diagonals); oracle: shifted int64 slices."""
    n, off = 4 << 20, [-1024, 0, 3]
    g = torch.Generator(device=gpu).manual_seed(11)

    def ints(k):
        v = torch.randint(1, 9, (k,), generator=g, device=gpu, dtype=torch.int32)
        return torch.where(torch.randint(0, 2, (k,), generator=g, device=gpu, dtype=torch.int32) == 1, v, -v)

    data, xi = ints(3 * n), ints(n)
    r = torch.arange(n, device=gpu)
    for d, o in enumerate(off):  # out-of-range slots: a value no sum may contain
        data[d * n:(d + 1) * n][(r + o < 0) | (r + o >= n)] = 7
    a = DIA(n, n, torch.tensor(off, dtype=torch.int32, device=gpu), data.float())
    dh, xh = data.cpu().numpy().astype(np.int64).reshape(3, n), xi.cpu().numpy().astype(np.int64)
    ax = np.zeros(n, dtype=np.int64)
    for d, o in enumerate(off):
        lo, hi = max(0, -o), min(n, n - o)
        ax[lo:hi] += dh[d, lo:hi] * xh[lo + o:hi + o]
    x = xi.float()
    y = spmv(a, x, U.nan_y(n, gpu))
    assert torch.equal(y.cpu(), U.expected(ax, 0.0, None))
    y0 = U.int_y0(n, 1)
    assert torch.equal(spmv(a, x, y0.to(gpu), beta=0.5).cpu(), U.expected(ax, 0.5, y0))


# ========================================================== column-blocked CSR
@pytest.mark.gpu
@pytest.mark.parametrize("aligned", [True, False])
def test_column_blocks(gpu, aligned):
    """Seven blocks of 14 columns (the last 13 wide), two of them without
    entries; x enters as offset slices; beta is applied by the first block only."""
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 10, 515)
    pool = np.array([c for c in range(1, 96) if c // 14 not in (2, 5)])
    a, x, ax = case(("cb",), lambda _r: lens, 97, cols=pool[rng.integers(0, pool.size, int(lens.sum()))])
    m = to_csr_colblocked(a, block_bytes=64, aligned=aligned)
    assert len(m.blocks) == 7 and m.blocks[-1].ncols == 13 and m.blocks[2].nnz == 0 and m.blocks[5].nnz == 0
    assert all(isinstance(b, CSRAligned) == aligned for b in m.blocks)
    U.check_exact(run_spmv(m.to(gpu)), ax, x, gpu, f"column blocks, aligned {aligned}", U.BETAS)


# ============================================================= prepare(a, "auto")
def auto_case(want):
    rng = np.random.default_rng(8)
    if want == "dia":
        d, x, ax = U.int_dia(600, 600, [-20, -1, 0, 1, 20], seed=4, garbage=0.0)
        return U.csr_of_dia(d), x, ax
    if want == "csr_cb":  # the 2000 x 2^20 shape of test_colblocked_format_choice_and_blocks
        a = U.int_csr(rng.integers(2, 23, 2000), 1 << 20, seed=5)
    else:
        lens = {"ell": lambda: rng.integers(6, 9, 300), "csr_aligned": lambda: rng.integers(0, 31, 300),
                "hyb": lambda: np.concatenate([rng.integers(0, 10, 299), [200]])}[want]()
        a = U.int_csr(lens, 331, seed=6)
    x = U.x_for(a)
    return a, x, U.interp_csr(a, U.x_int(x))


@pytest.mark.gpu
@pytest.mark.parametrize("want", ["dia", "ell", "hyb", "csr_aligned", "csr_cb"])
def test_prepare_auto(gpu, want):
    a, x, ax = U.cached(("auto", want), lambda: auto_case(want))
    name, m = prepare(a, "auto", gpu)
    assert name == want
    U.check_exact(run_spmv(m), ax, x, gpu, f"prepare auto -> {want}", (0.0, 1.0))


# ================================================================== offset views
def offset_view(t, dev):
    buf = torch.zeros(t.numel() + 1, dtype=t.dtype, device=dev)
    buf[1:].copy_(t)
    v = buf[1:]
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ["short", "medium"])
def test_offset_views(gpu, rows):
    """rp, col and val four bytes off a 16-byte boundary: no 16-byte load may
    be formed on them. CSR-stream refuses such arrays and spmv() takes
    CSR-vector for "stream" and for "auto" (a mean of 20 entries per row)."""
    a, x, ax = case(("views", rows), lambda rng: rng.integers(0, 10, 300) if rows == "short" else
                    rng.integers(10, 31, 300), 97)
    v = CSR(a.nrows, a.ncols, offset_view(a.rp, gpu), offset_view(a.col, gpu), offset_view(a.val, gpu))
    y = torch.full((a.nrows,), 5.0, device=gpu)
    rc = _ext._fn("hip", "cme_spmv_csr_stream")(v.nrows, v.rp.data_ptr(), v.col.data_ptr(), v.val.data_ptr(),
                                                x.to(gpu).data_ptr(), y.data_ptr(), 64, 0.0, _ext.stream_ptr(gpu))
    torch.cuda.synchronize()
    assert rc == HIP_INVALID_VALUE and bool((y == 5.0).all())
    for i, kernel in enumerate(["auto", "stream", "short", "wave", "scalar", "vector"]):
        U.check_exact(run_spmv(v, kernel), ax, x, gpu, f"offset views, {kernel}", U.beta_pair(i))


# ========================================================== argument validation
def operands(dev):
    a, x, ax = sweep_case(65)
    return a.to(dev), x.to(dev), ax


def validation(dev, other):
    a, x, ax = operands(dev)
    n, m = a.nrows, a.ncols
    wide = torch.zeros(2 * m, device=dev)
    wide[::2] = x
    U.assert_same(spmv(a, wide[::2]), U.expected(ax, 0.0, None), "non-contiguous x")
    y = U.nan_y(n, dev)
    bad_x = [(TypeError, x.double()), (TypeError, torch.ones(m, dtype=torch.int32, device=dev)), (ValueError, x[:-1]), (ValueError, x[None, :]),
             (ValueError, torch.cat([x, x[:1]]))]
    bad_y = [(TypeError, y.double()), (ValueError, y[:-1].clone()), (ValueError, torch.cat([y, y])),
             (ValueError, U.nan_y(2 * n, dev)[::2]), (ValueError, y[:, None])]
    if other is not None:
        bad_x.append((ValueError, x.to(other)))
        bad_y.append((ValueError, y.to(other)))
    for err, xb in bad_x:
        with pytest.raises(err):
            spmv(a, xb)
        with pytest.raises(err):
            spmv(a, xb, y)
    for err, yb in bad_y:
        keep = yb.clone()
        with pytest.raises(err):
            spmv(a, x, yb)
        assert torch.equal(torch.nan_to_num(yb), torch.nan_to_num(keep))  # raised before any launch
    assert bool(torch.isnan(y).all())


def test_argument_validation_cpu():
    validation(CPU, None)


@pytest.mark.gpu
def test_argument_validation_gpu(gpu):
    validation(gpu, CPU)
    a, x, _ = operands(CPU)
    with pytest.raises(ValueError):
        spmv(a, x.to(gpu))  # host matrix, device x
    for fmt in ("csr_aligned", "ell", "coo", "hyb", "dia", "csr_cb"):
        m = to_format(a, fmt).to(gpu)
        with pytest.raises(ValueError):
            spmv(m, x.to(gpu)[:-1])
        with pytest.raises(TypeError):
            spmv(m, x.to(gpu), torch.zeros(a.nrows, dtype=torch.float64, device=gpu))


# =================================================================== float data
FLOAT_FORMATS = ["csr_scalar", "csr_vector", "csr_stream", "csr_short", "csr_wave", "csr_auto", "csr_aligned", "ell",
                 "dia", "coo", "hyb", "csr_cb"]


def float_case(mat):
    """The matrices of test_spmv.py::test_spmv_gpu with randn x and y0."""
    def make():
        a = {"5pt": lambda: laplacian("5pt", 100), "27pt": lambda: laplacian("27pt", 20),
             "random": lambda: random_csr(20000, 15000, 12, seed=2),
             "skew": lambda: random_csr(20000, 20000, 20, seed=3, skew=True)}[mat]()
        g = torch.Generator().manual_seed(12)
        return a, torch.randn(a.ncols, generator=g), torch.randn(a.nrows, generator=g)
    return U.cached(("float", mat), make)


@pytest.mark.gpu
@pytest.mark.parametrize("mat,fmt", [(m, f) for m in ("5pt", "27pt", "random", "skew") for f in FLOAT_FORMATS
                                     if f != "dia" or m in ("5pt", "27pt")])
def test_float_within_derived_bound(gpu, mat, fmt):
    """randn data: |y - y64| <= (L + 3) 2^-24 (sum |v x| + |beta y0|) per row,
    L the row's stored terms in this format; two runs agree bitwise wherever
    no atomics are involved."""
    a, x, y0 = float_case(mat)
    kernel = fmt[4:] if fmt[4:] in CSR_KERNELS else "auto"
    m = (to_csr_colblocked(a, block_bytes=4096) if fmt == "csr_cb" else to_format(a, fmt))
    L = U.stored_terms(m)
    m = m.to(gpu)
    rows = U.row_ids(a.rp.numpy().astype(np.int64))
    xd = x.to(gpu)
    for beta in (0.0, 0.5):
        y64, bound = U.float_reference(rows, a.val.numpy(), x.numpy()[a.col.numpy()], a.nrows, L, beta, y0.numpy())
        y = spmv(m, xd, U.nan_y(a.nrows, gpu) if beta == 0.0 else y0.to(gpu), kernel=kernel, beta=beta)
        again = spmv(m, xd, U.nan_y(a.nrows, gpu) if beta == 0.0 else y0.to(gpu), kernel=kernel, beta=beta)
        err = np.abs(y.cpu().numpy().astype(np.float64) - y64)
        worst = int(np.argmax(err - bound))
        print(f"{mat} {fmt} beta {beta}: max err {err.max():.3e}, at the worst row err {err[worst]:.3e} "
              f"bound {bound[worst]:.3e}")
        assert np.all(err <= bound), f"row {worst}: |y - y64| = {err[worst]} > {bound[worst]}"
        if fmt not in ("coo", "hyb"):
            assert torch.equal(y, again)


# ================================================================ graph capture
@pytest.mark.gpu
@pytest.mark.parametrize("fmt", ["csr", "csr_aligned", "ell", "dia", "coo", "hyb", "csr_cb", "csr_cb_u"])
def test_graph_replay_equals_eager(gpu, fmt):
    """One capture and replay per format (HYB: two kernels, three with the
    scale; column blocks: sliced x views): the replay equals the eager run."""
    a, x, ax = sweep_case(513)
    if fmt == "dia":
        m, x, ax = U.int_dia(513, 550, U.dia_offsets(513, 550, 9, seed=2), seed=3)
    elif fmt == "hyb":
        m = to_hyb(a, K=4)
    else:
        m = to_format(a, fmt)
    m, xd = m.to(gpu), x.to(gpu)
    y0 = U.int_y0(513, 4)
    eager = spmv(m, xd, y0.to(gpu), beta=-2.0)
    U.assert_same(eager, U.expected(ax, -2.0, y0), f"{fmt}, eager")
    y = y0.to(gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        spmv(m, xd, y, beta=-2.0)
    y.copy_(y0)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, eager)
