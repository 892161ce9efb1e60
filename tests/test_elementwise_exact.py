"""The hw1 streaming kernels (csrc/hip/elementwise.hip), exactly: the shift
cipher at every width for every (byte, shift) pair, at the sizes around one
lane's load, on misaligned views of either operand and in the unrolled
non-temporal loop; copy_ and mul_ on aligned and misaligned operands.

The cipher and mul_ bodies run on the CPU backend (unmarked) and on the HIP
kernels (``gpu``); copy_ exists on the GPU only. The argument checks sit in
the wrappers and run on the CPU.
"""
import numpy as np
import pytest
import torch
from text_util import dev, seeded, view_at  # noqa: F401

from cme213x.ops.elementwise import copy_, mul_, shift_cipher

WIDTHS = ["char", "uint", "uint2", "uint4"]
GUARD = 0xA5


def guarded(n: int, off: int, dev, dtype=torch.uint8):
    """(whole buffer, the n-element view ``off`` elements into it); the
    elements around the view hold GUARD and must still hold it afterwards."""
    buf = torch.full((off + n + 16,), GUARD, dtype=dtype, device=dev)
    return buf, buf[off:off + n]


def guards_intact(buf: torch.Tensor, n: int, off: int) -> bool:
    b = buf.cpu()
    return bool((b[:off] == GUARD).all() and (b[off + n:] == GUARD).all())


# ============================================================== shift_cipher
@pytest.mark.parametrize("width", WIDTHS)
def test_shift_every_byte_every_shift(dev, width):
    """All 256 byte values (and a 3-byte tail) under all 256 shifts, -1 and
    259: a packed add that let a carry cross into the next byte would show for
    some pair. One row of a device matrix per shift, compared once."""
    a = np.concatenate([np.arange(256), [255, 0, 128]]).astype(np.uint8)
    shifts = list(range(256)) + [-1, 259]
    x = view_at(a, 0, dev)
    rows = torch.zeros(len(shifts), 272, dtype=torch.uint8, device=dev)  # 272: every row starts 16-byte aligned
    for k, s in enumerate(shifts):
        out = rows[k, :a.size]
        assert out.data_ptr() % 16 == 0
        assert shift_cipher(x, s, out=out, width=width) is out
    want = ((a.astype(np.int64)[None, :] + np.asarray(shifts)[:, None]) % 256).astype(np.uint8)
    got = rows.cpu().numpy()
    assert np.array_equal(got[:, :a.size], want)
    assert not got[:, a.size:].any()


@pytest.mark.parametrize("width", WIDTHS)
def test_shift_small_sizes_and_offset_views(dev, width):
    for n in (0, 1, 3, 4, 7, 8, 15, 16, 17, 1027):
        a = seeded("shift", n).integers(0, 256, n, dtype=np.uint8)
        want = torch.from_numpy(((a.astype(np.int64) + 77) % 256).astype(np.uint8))
        # (offset of the input, offset of out): aligned, then each one off by 1 and by 3 bytes
        for xo, oo in ((0, 0), (1, 0), (3, 0), (0, 1), (0, 3), (1, 3)):
            x = view_at(a, xo, dev)
            buf, out = guarded(n, oo, dev)
            shift_cipher(x, 77, out=out, width=width)
            assert torch.equal(out.cpu(), want), (n, xo, oo)
            assert guards_intact(buf, n, oo), (n, xo, oo)
            assert torch.equal(x.cpu(), torch.from_numpy(a)), "input changed"
        assert torch.equal(shift_cipher(view_at(a, 0, dev), 77, width=width).cpu(), want)


@pytest.mark.parametrize("width", WIDTHS)
def test_shift_block_sizes(dev, width):
    a = seeded("block").integers(0, 256, 5003, dtype=np.uint8)
    want = torch.from_numpy(((a.astype(np.int64) + 200) % 256).astype(np.uint8))
    x = view_at(a, 0, dev)
    for block in (64, 256, 0, 1, 192):  # 0: the default
        assert torch.equal(shift_cipher(x, 200, width=width, block=block).cpu(), want), block


def test_shift_arguments():
    x = torch.zeros(100, dtype=torch.uint8)
    for block in (257, 1024, -1, -256):  # the kernels are compiled for at most 256 threads
        with pytest.raises(ValueError):
            shift_cipher(x, 1, block=block)
    with pytest.raises(ValueError):
        shift_cipher(x, 1, width="uint8")
    with pytest.raises(ValueError):
        shift_cipher(x, 1, out=torch.zeros(99, dtype=torch.uint8))
    with pytest.raises(ValueError):
        shift_cipher(x, 1, out=torch.zeros(200, dtype=torch.uint8)[::2])
    with pytest.raises(TypeError):
        shift_cipher(torch.zeros(200, dtype=torch.uint8)[::2], 1)


def test_shift_unrolled_nontemporal_loop(dev):
    """The size at which ``shift_u128_kernel<4>`` enters its unrolled
    non-temporal loop. The grid is capped at 1024 blocks of 256 lanes, a
    stride of 262 144 16-byte vectors, and a lane enters the loop only while
    ``i + 3 * stride < m``: m = 4 * 262 144 + 1000 vectors gives every lane one
    unrolled trip, lanes 0..999 one more vector in the remainder loop, and the
    5 bytes after the last vector go to the byte kernel (about 16.8 MB)."""
    n = 16 * (4 * 262_144 + 1000) + 5
    a = seeded("big").integers(0, 256, n, dtype=np.uint8)
    x = view_at(a, 0, dev)
    buf, out = guarded(n, 0, dev)
    shift_cipher(x, 131, out=out, width="uint4")
    assert np.array_equal(out.cpu().numpy(), a + np.uint8(131))  # uint8 addition wraps
    assert guards_intact(buf, n, 0)


# ====================================================================== mul_
def mul_data(n: int, seed=0):
    rng = seeded("mul", n, seed)
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    tiny = np.float32(1e-45)
    # denormal operands and results, signed zeros, infinities (never inf * 0)
    sa = [3 * tiny, -5 * tiny, 1e-30, 0.0, -0.0, 0.0, np.inf, -np.inf, np.inf, 1e30, 3.0e38, 1.5]
    sb = [2.0, 0.5, 1e-10, -1.0, 2.0, -0.0, 2.0, 3.0, -np.inf, 1e30, -2.0, 7 * tiny]
    k = min(n, len(sa))
    at = rng.permutation(n)[:k]
    a[at] = np.asarray(sa, dtype=np.float32)[:k]
    b[at] = np.asarray(sb, dtype=np.float32)[:k]
    with np.errstate(over="ignore"):
        want = a * b  # one float32 rounding per element
    assert not np.isnan(want).any()
    return a, b, want


def bitwise_equal(got: torch.Tensor, want: np.ndarray) -> bool:
    return np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))


# 2 100 003: past the 2048 blocks x 256 lanes x 4 floats of one trip of the grid
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027, 2_100_003])
def test_mul(dev, n):
    a, b, want = mul_data(n)
    assert bitwise_equal(torch.from_numpy(a) * torch.from_numpy(b), want)  # torch's product is the same one
    offsets = [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (1, 1), (3, 2)]
    for ao, bo in offsets if n < 100_000 else offsets[:1] + offsets[3:5]:
        buf = torch.full((ao + n + 16,), float(GUARD), dtype=torch.float32, device=dev)
        x = buf[ao:ao + n]
        x.copy_(torch.from_numpy(a))
        y = view_at(b, bo, dev)
        assert mul_(x, y) is x
        assert bitwise_equal(x, want), (n, ao, bo)
        assert guards_intact(buf, n, ao), (n, ao, bo)
        assert bitwise_equal(y, b), "b changed"


def test_mul_and_copy_need_contiguous_operands():
    a = torch.ones(8, 8)
    with pytest.raises(ValueError):
        mul_(a[:, ::2], torch.ones(8, 4))
    with pytest.raises(ValueError):
        mul_(torch.ones(8, 4), a[:, ::2])
    with pytest.raises(ValueError):
        mul_(a.t(), torch.ones(8, 8))
    with pytest.raises(ValueError):
        copy_(a[:, ::2], torch.ones(8, 4))
    with pytest.raises(ValueError):
        copy_(torch.ones(8, 4), a[:, ::2])
    assert a.eq(1).all()


# ===================================================================== copy_
@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027])
def test_copy_floats(gpu, n):
    a = seeded("copy", n).standard_normal(n).astype(np.float32)
    for so, do in [(0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (0, 2), (0, 3), (2, 1)]:
        src = view_at(a, so, gpu)
        buf, dst = guarded(n, do, gpu, torch.float32)
        assert copy_(dst, src) is dst
        assert bitwise_equal(dst, a), (n, so, do)
        assert guards_intact(buf, n, do), (n, so, do)
        assert bitwise_equal(src, a)


@pytest.mark.gpu
# one 16-byte lane less a byte, exactly, and plus a byte; 4099: one block of lanes and a 3-byte tail
@pytest.mark.parametrize("n", [15, 16, 17, 4099])
def test_copy_bytes(gpu, n):
    a = seeded("copyb", n).integers(0, 256, n, dtype=np.uint8)
    for so, do in [(0, 0), (1, 0), (0, 3), (5, 9)]:
        src = view_at(a, so, gpu)
        buf, dst = guarded(n, do, gpu)
        copy_(dst, src)
        assert torch.equal(dst.cpu(), torch.from_numpy(a)), (n, so, do)
        assert guards_intact(buf, n, do), (n, so, do)
