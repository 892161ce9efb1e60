"""Matrix transpose ladder (Lecture06/07, Ruetsch & Micikevicius
``my-refs/MatrixTranspose.pdf``): copy / naive / LDS tile / +1 pad / XOR
swizzle / diagonal reorder / XCD remap / 16-B vectorised. CPU: OpenMP blocked.

Effective bandwidth convention (the paper's): 2 x bytes / time.
"""
from __future__ import annotations

import torch

from .. import _ext

_ext.proto(_ext.HIP_PROTOS, "cme_transpose_f32", "ppiiip")
_ext.proto(_ext.HIP_PROTOS, "cme_transpose_reps_f32", "ppiiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_transpose_f32", "ppiii")

VARIANTS = {"copy": 0, "naive": 1, "lds": 2, "lds_pad": 3, "lds_swizzle": 4, "diagonal": 5, "xcd": 6, "vec": 7,
            "vec_xcd": 8, "naive_1d": 9}
# the paper's diagnostic kernels (square matrices; NOT transposes):
# "coarse" moves tiles without transposing their elements, "fine" transposes
# elements inside tiles that stay in place
DIAGNOSTICS = {"coarse": 10, "fine": 11}
_TILE = 64  # kT of csrc/hip/transpose.hip


def _check_out(out: torch.Tensor, shape: tuple, x: torch.Tensor) -> None:
    """The kernels write ``shape`` contiguous float32 elements through out's
    pointer: anything else is written out of bounds or through the wrong strides."""
    if not isinstance(out, torch.Tensor) or out.dtype != torch.float32:
        raise ValueError("out must be a float32 tensor")
    if tuple(out.shape) != tuple(shape):
        raise ValueError(f"out must have shape {tuple(shape)}, got {tuple(out.shape)}")
    if out.device != x.device:
        raise ValueError(f"out is on {out.device}, the input on {x.device}")
    if not out.is_contiguous():
        raise ValueError("out must be contiguous")


def transpose(x: torch.Tensor, variant: str = "vec", out: torch.Tensor | None = None) -> torch.Tensor:
    """Transpose a 2-D float32 tensor (``variant="copy"`` returns a same-shape
    copy -- the bandwidth upper bound). A non-contiguous ``x`` is made
    contiguous first; ``out``, when given, is a contiguous float32 tensor of
    the result's shape on x's device and is returned."""
    if x.dim() != 2 or x.dtype != torch.float32:
        raise TypeError("transpose expects a 2-D float32 tensor")
    if variant not in VARIANTS:
        raise ValueError(f"unknown variant {variant!r} (one of {', '.join(VARIANTS)})")
    x = x.contiguous()
    rows, cols = x.shape
    shape = (rows, cols) if variant == "copy" else (cols, rows)
    if out is None:
        out = torch.empty(shape, dtype=x.dtype, device=x.device)
    else:
        _check_out(out, shape, x)
    if x.is_cuda:
        _ext.call_hip("cme_transpose_f32", x.data_ptr(), out.data_ptr(), rows, cols, VARIANTS[variant],
                      _ext.stream_ptr(x.device))
    else:
        if variant == "copy":
            out.copy_(x)
        else:
            _ext.call_cpu("cme_cpu_transpose_f32", x.data_ptr(), out.data_ptr(), rows, cols,
                          0 if variant == "naive" else 1)
    return out


def diagnostic(x: torch.Tensor, kind: str, out: torch.Tensor | None = None) -> torch.Tensor:
    """The paper's coarse-/fine-grained diagnostic kernels (square, GPU):
    ``coarse`` = tiles moved to their transposed position, elements kept in
    tile order; ``fine`` = elements transposed inside tiles kept in place.
    Whole 64 x 64 tiles only: a partial tile has no transposed position with
    the same shape."""
    if x.dim() != 2 or x.shape[0] != x.shape[1] or not x.is_cuda:
        raise ValueError("diagnostics take a square cuda matrix")
    if kind not in DIAGNOSTICS:
        raise ValueError(f"unknown diagnostic {kind!r} (one of {', '.join(DIAGNOSTICS)})")
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("diagnostics take a contiguous float32 matrix")
    if x.shape[0] % _TILE:
        raise ValueError(f"diagnostics take whole {_TILE} x {_TILE} tiles: n = {x.shape[0]} is no multiple of {_TILE}")
    if out is None:
        out = torch.empty_like(x)
    else:
        _check_out(out, x.shape, x)
    _ext.call_hip("cme_transpose_f32", x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], DIAGNOSTICS[kind],
                  _ext.stream_ptr(x.device))
    return out


def transpose_reps(x: torch.Tensor, reps: int, out: torch.Tensor | None = None) -> torch.Tensor:
    """lds_pad transpose performed ``reps`` (>= 1) times inside ONE kernel
    launch -- the paper's second timing methodology (launch overhead
    excluded). A non-contiguous ``x`` is made contiguous first."""
    if not x.is_cuda:
        raise ValueError("GPU only")
    if x.dim() != 2 or x.dtype != torch.float32:
        raise ValueError("transpose_reps expects a 2-D float32 tensor")
    if isinstance(reps, bool) or not isinstance(reps, int) or reps < 1:
        raise ValueError(f"reps must be a positive integer, got {reps!r}")
    x = x.contiguous()
    rows, cols = x.shape
    if out is None:
        out = torch.empty((cols, rows), dtype=x.dtype, device=x.device)
    else:
        _check_out(out, (cols, rows), x)
    _ext.call_hip("cme_transpose_reps_f32", x.data_ptr(), out.data_ptr(), rows, cols, reps,
                  _ext.stream_ptr(x.device))
    return out
