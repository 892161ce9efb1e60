"""Transpose, exactly: every case of cme_transpose_f32, every arm of
cme_transpose_tune, tile_reps_kernel and the two diagnostic kernels of
csrc/hip/transpose.hip against numpy, bit for bit.

Data. ``x[r, c] = r * cols + c`` as float32 with fewer than 2**24 elements:
every value is distinct and exact, so a wrong element cannot equal the right
one by chance. The expected result is ``numpy.ascontiguousarray(x.T)``. Every
output starts from -1 (no element is negative), so an element that no thread
wrote shows as well.

Unmarked tests run the CPU backend and the argument checks; ``gpu`` tests run
the HIP kernels.
"""
import numpy as np
import pytest
import torch

from cme213x import _ext
from cme213x.ops.transpose import DIAGNOSTICS, VARIANTS, diagnostic, transpose, transpose_reps

_ext.proto(_ext.HIP_PROTOS, "cme_transpose_tune", "ppiiiiip")  # as benchmarks/tune_transpose.py declares it

CPU = torch.device("cpu")
INVALID = r"HIP error 1 \("  # hipErrorInvalidValue, raised by _ext.check

# partial tiles in each direction, square partial grids (diagonal, xcd), both
# production instantiations of vec (square: 64x64 diagonal; otherwise 64x128)
# and the fallback of vec (a dimension that is no multiple of 4)
SHAPES = [(1, 1), (1, 300), (300, 1), (4, 4), (63, 65), (64, 64), (65, 63), (100, 100), (128, 192), (130, 70),
          (257, 129), (260, 132), (516, 1028)]
EMPTY = [(0, 5), (5, 0), (0, 0)]
CPU_VARIANTS = ["copy", "naive", "lds_pad"]

_cache: dict = {}


def data(shape, dev=CPU):
    """(x, expected transpose) on ``dev``, built once per shape and device."""
    key = (tuple(shape), str(dev))
    if key not in _cache:
        rows, cols = shape
        assert rows * cols < 2 ** 24
        a = np.arange(rows * cols, dtype=np.float32).reshape(rows, cols)
        _cache[key] = (torch.from_numpy(a).to(dev), torch.from_numpy(np.ascontiguousarray(a.T)).to(dev))
    return _cache[key]


def fresh(shape, dev):
    return torch.full(tuple(shape), -1.0, dtype=torch.float32, device=dev)


def check_variant(shape, variant, dev):
    x, want = data(shape, dev)
    if variant == "copy":
        want = x
    out = fresh(want.shape, dev)
    got = transpose(x, variant, out)
    assert got is out
    assert torch.equal(got, want), f"{variant} {shape}: {int((got != want).sum())} wrong elements"
    got = transpose(x, variant)
    assert got.shape == want.shape and got.is_contiguous() and torch.equal(got, want)
    if variant == "copy":
        assert got.data_ptr() != x.data_ptr()


# ======================================================================== CPU
@pytest.mark.parametrize("shape", SHAPES, ids=str)
@pytest.mark.parametrize("variant", CPU_VARIANTS)
def test_variants_cpu(shape, variant):
    check_variant(shape, variant, CPU)


def check_empty(dev, variants):
    for shape in EMPTY:
        x = torch.empty(shape, dtype=torch.float32, device=dev)
        for v in variants:
            want = shape if v == "copy" else shape[::-1]
            got = transpose(x, v)
            assert tuple(got.shape) == want and got.dtype == torch.float32 and got.device == x.device
            out = torch.empty(want, dtype=torch.float32, device=dev)
            assert transpose(x, v, out) is out


def test_empty_cpu():
    check_empty(CPU, VARIANTS)


def check_views(dev, variants):
    """Non-contiguous inputs are made contiguous; 4-byte-offset inputs and
    outputs (which vec / vec_xcd must hand to the scalar tile kernel)."""
    for shape in [(128, 192), (64, 64), (130, 70)]:
        rows, cols = shape
        x, want = data(shape, dev)
        for v in variants:
            assert torch.equal(transpose(want.t(), v), want), (v, shape, "x.t() as input")
            assert torch.equal(transpose(x[:, ::2], v), want[::2].contiguous()), (v, shape, "x[:, ::2] as input")
            shifted = torch.cat([fresh((1,), dev), x.reshape(-1)])[1:].view(rows, cols)
            assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
            assert torch.equal(transpose(shifted, v), want), (v, shape, "offset input")
            buf = fresh((rows * cols + 2,), dev)
            out = buf[1:-1].view(cols, rows)
            assert out.data_ptr() % 16 == 4
            assert transpose(x, v, out) is out
            assert torch.equal(out, want) and buf[0] == -1 and buf[-1] == -1, (v, shape, "offset out")


def test_views_cpu():
    check_views(CPU, ["naive", "lds_pad"])


def check_out_rejections(dev):
    """A wrong ``out`` raises before any launch (it would be written out of
    bounds, or through the wrong strides)."""
    x, want = data((130, 70), dev)
    other = torch.device("meta") if dev.type == "cpu" else CPU
    for v in ("vec", "naive", "lds_pad", "copy"):
        good = (130, 70) if v == "copy" else (70, 130)
        bad = [torch.empty(good[::-1], device=dev), torch.empty((good[0], good[1] - 1), device=dev),
               torch.empty(good[0] * good[1], device=dev), torch.empty(good, device=dev, dtype=torch.float64),
               torch.empty(good, device=dev, dtype=torch.int32), torch.empty(good, device=other),
               torch.empty(good[::-1], device=dev).t(), torch.empty((good[0], 2 * good[1]), device=dev)[:, ::2]]
        for out in bad:
            with pytest.raises(ValueError):
                transpose(x, v, out)
    with pytest.raises(ValueError):
        transpose(x, "no_such_variant")
    for bad_x in (x.double(), x.to(torch.int32), x[0], x.view(2, 65, 70)):
        with pytest.raises(TypeError):
            transpose(bad_x)


def test_out_rejections_cpu():
    check_out_rejections(CPU)


def test_gpu_only_entry_points_reject_cpu_tensors():
    x, _ = data((64, 64))
    with pytest.raises(ValueError):
        diagnostic(x, "coarse")
    with pytest.raises(ValueError):
        transpose_reps(x, 1)


# ============================================================== GPU: variants
# The gpu tests loop over their cases inside one test each (every case runs
# before the test fails and the message names all that differ): the suite
# already holds thousands of gpu test ids, and these add six.
@pytest.mark.gpu
def test_variants_gpu(gpu):
    """Every variant of VARIANTS at every shape of SHAPES."""
    wrong = []
    for shape in SHAPES:
        for variant in VARIANTS:
            try:
                check_variant(shape, variant, gpu)
            except AssertionError as e:
                wrong.append(str(e))
    assert not wrong, f"{len(wrong)} of {len(SHAPES) * len(VARIANTS)} differ:\n" + "\n".join(wrong[:40])
    empty_gpu(gpu)


def empty_gpu(gpu):
    check_empty(gpu, VARIANTS)
    x = torch.empty((0, 0), dtype=torch.float32, device=gpu)
    assert diagnostic(x, "coarse").shape == (0, 0) and diagnostic(x, "fine").shape == (0, 0)
    for shape in EMPTY:
        x = torch.empty(shape, dtype=torch.float32, device=gpu)
        assert transpose_reps(x, 3).shape == shape[::-1]
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_views_and_out_gpu(gpu):
    check_views(gpu, ["vec", "vec_xcd", "lds_pad", "naive_1d"])
    check_out_rejections(gpu)


# ================================================================= GPU: tall
def tall(dev, rows=4194368, cols=4):
    """(x, x.T) with x[r, c] = (r % 4096) * 4 + c: 65537 tile rows of 64."""
    key = ("tall", str(dev))
    if key not in _cache:
        r = torch.arange(rows, device=dev, dtype=torch.int32)
        x = ((r % 4096) * 4).view(rows, 1) + torch.arange(cols, device=dev, dtype=torch.int32).view(1, cols)
        x = x.to(torch.float32).contiguous()
        _cache[key] = (x, x.t().contiguous())
    return _cache[key]


@pytest.mark.gpu
def test_tall_gpu(gpu):
    """cdiv(rows, 64) = 65537 blocks along gridDim.y (4194368 x 4) and along
    gridDim.x (its transpose)."""
    x, xt = tall(gpu)
    wrong = []
    for src, want in ((x, xt), (xt, x)):
        for variant in ("vec", "lds_pad", "naive", "naive_1d"):
            out = fresh(want.shape, gpu)
            assert transpose(src, variant, out) is out
            if not torch.equal(out, want):
                wrong.append((variant, tuple(src.shape)))
    _cache.pop(("tall", str(gpu)))  # 128 MB: not kept for the rest of the session
    assert not wrong, f"wrong: {wrong}"


# ========================================================== GPU: tuning arms
TILES = [(64, 64), (128, 64), (256, 64), (64, 128), (128, 128), (256, 128)]
REMAPS = [0, 1, 2, 4, 6, 8, 9, 12, 13, 20, 22]
# (332, 204): partial tiles in both directions; the second tile of a K = 2
# arm's last block is partly out of range for 64- and 256-row tiles and
# wholly for 128-row tiles (3 tile rows). (512, 256): an exact fit. Two
# squares: (320, 320) gives 5x5 and 3x3 grids (and 5 tile rows of 64: a K = 2
# second tile wholly out of range), (256, 256) gives 4x4 and 2x2 grids, where
# a diagonal remap with the wrong stride is no permutation of the blocks.
TUNE_SHAPES = [(332, 204), (512, 256), (320, 320), (256, 256)]


def tune(x, out, tr, tc, remap):
    rows, cols = x.shape
    _ext.call_hip("cme_transpose_tune", x.data_ptr(), out.data_ptr(), rows, cols, tr, tc, remap,
                  _ext.stream_ptr(x.device))


def lds_fits(tr, tc, remap):
    k = 2 if remap & 8 else 1
    return k * tc * (tr + 1) * 4 <= 160 * 1024


def test_tune_arm_table():
    """66 arms; the only ones that cannot exist are the two-tile arms of the
    256 x 128 tile (2 x 128 x 257 floats = 257 KB of LDS)."""
    arms = [(t, r) for t in TILES for r in REMAPS]
    assert len(arms) == 66
    assert [(t, r) for t, r in arms if not lds_fits(*t, r)] == [((256, 128), r) for r in (8, 9, 12, 13)]


def tune_arms_gpu(gpu, shape, wrong):
    x, want = data(shape, gpu)
    for tr, tc in TILES:
        for remap in REMAPS:
            out = fresh(want.shape, gpu)
            if not lds_fits(tr, tc, remap):
                with pytest.raises(RuntimeError, match=INVALID):
                    tune(x, out, tr, tc, remap)
                assert bool((out == -1).all())
                continue
            tune(x, out, tr, tc, remap)
            if not torch.equal(out, want):
                wrong.append(f"{shape}, tile {tr}x{tc}, remap {remap}: {int((out != want).sum())} wrong elements")


@pytest.mark.gpu
def test_tune_arms_gpu(gpu):
    """All 66 arms at every shape of TUNE_SHAPES."""
    wrong = []
    for shape in TUNE_SHAPES:
        tune_arms_gpu(gpu, shape, wrong)
    assert not wrong, f"{len(wrong)} differ:\n" + "\n".join(wrong[:40])


def tune_rejections_gpu(gpu):
    """Shapes that are no multiple of 4 (16-byte accesses), unknown remap
    codes and unknown tiles are rejected by the entry and nothing is written."""
    for shape, tr, tc, remap in [((330, 204), 64, 64, 0), ((332, 202), 64, 64, 0), ((63, 65), 64, 128, 20),
                                 ((332, 204), 64, 64, 3), ((332, 204), 64, 64, 5), ((332, 204), 128, 64, 16),
                                 ((332, 204), 32, 64, 0), ((332, 204), 64, 256, 0), ((332, 204), 64, 64, -1)]:
        x, want = data(shape, gpu)
        out = fresh(want.shape, gpu)
        with pytest.raises(RuntimeError, match=INVALID):
            tune(x, out, tr, tc, remap)
        assert bool((out == -1).all())


# ============================================== GPU: diagnostics and reps
def diagnostics_gpu(gpu, n):
    x, _ = data((n, n), gpu)
    T = 64
    xt = x.view(n // T, T, n // T, T)  # [tile_r, r, tile_c, c]
    # coarse: tile (I, J) lands at tile (J, I) with its elements untransposed
    coarse = xt.permute(2, 1, 0, 3).reshape(n, n)
    # fine: tile (I, J) stays, its elements are transposed
    fine = xt.permute(0, 3, 2, 1).reshape(n, n)
    for kind, want in (("coarse", coarse), ("fine", fine)):
        out = fresh((n, n), gpu)
        assert diagnostic(x, kind, out) is out
        assert torch.equal(out, want), kind
        assert torch.equal(diagnostic(x, kind), want), kind


def diagnostic_rejections_gpu(gpu):
    for kind in DIAGNOSTICS:
        for n in (1, 63, 65, 100, 130):
            x, _ = data((n, n), gpu)
            with pytest.raises(ValueError):
                diagnostic(x, kind)
            out = fresh((n, n), gpu)  # the entry point itself rejects it as well
            with pytest.raises(RuntimeError, match=INVALID):
                _ext.call_hip("cme_transpose_f32", x.data_ptr(), out.data_ptr(), n, n, DIAGNOSTICS[kind],
                              _ext.stream_ptr(gpu))
            assert bool((out == -1).all())
        x, _ = data((128, 128), gpu)
        for bad in (x.double(), x.to(torch.int32), x.t(), x[:, :64], x[0], data((128, 192), gpu)[0]):
            with pytest.raises(ValueError):
                diagnostic(bad, kind)
        for out in (torch.empty((128, 64), device=gpu), torch.empty((128, 128), device=gpu, dtype=torch.float64),
                    torch.empty((128, 128)), torch.empty((128, 128), device=gpu).t()):
            with pytest.raises(ValueError):
                diagnostic(x, kind, out)
    with pytest.raises(ValueError):
        diagnostic(x, "medium")


def transpose_reps_gpu(gpu, shape):
    x, want = data(shape, gpu)
    for reps in (1, 2, 5):
        out = fresh(want.shape, gpu)
        assert transpose_reps(x, reps, out) is out
        assert torch.equal(out, want), reps
        assert torch.equal(transpose_reps(x, reps), want), reps
    assert torch.equal(transpose_reps(want.t(), 2), want)  # non-contiguous input is made contiguous
    assert torch.equal(transpose_reps(x[:, ::2], 1), want[::2].contiguous())


def transpose_reps_rejections_gpu(gpu):
    x, want = data((130, 70), gpu)
    for reps in (0, -1, 1.5, None):
        with pytest.raises(ValueError):
            transpose_reps(x, reps)
    out = fresh(want.shape, gpu)  # the entry point rejects reps < 1 too and writes nothing
    with pytest.raises(RuntimeError, match=INVALID):
        _ext.call_hip("cme_transpose_reps_f32", x.data_ptr(), out.data_ptr(), 130, 70, 0, _ext.stream_ptr(gpu))
    assert bool((out == -1).all())
    for bad in (x.double(), x.to(torch.int32), x[0]):
        with pytest.raises(ValueError):
            transpose_reps(bad, 1)
    for out in (torch.empty((130, 70), device=gpu), torch.empty((70, 130), device=gpu, dtype=torch.float64),
                torch.empty((70, 130)), torch.empty((130, 70), device=gpu).t(), torch.empty(70 * 130, device=gpu)):
        with pytest.raises(ValueError):
            transpose_reps(x, 1, out)


@pytest.mark.gpu
def test_diagnostics_and_reps_gpu(gpu):
    """grain_kernel<0|1> at n = 64, 128, 320; tile_reps_kernel with reps = 1,
    2, 5 at a partial-tile and an exact shape."""
    for n in (64, 128, 320):
        diagnostics_gpu(gpu, n)
    for shape in ((130, 70), (256, 256)):
        transpose_reps_gpu(gpu, shape)


@pytest.mark.gpu
def test_rejections_gpu(gpu):
    """What the tuning entry, the diagnostics and transpose_reps refuse."""
    tune_rejections_gpu(gpu)
    diagnostic_rejections_gpu(gpu)
    transpose_reps_rejections_gpu(gpu)
