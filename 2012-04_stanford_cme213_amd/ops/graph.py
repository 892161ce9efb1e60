"""CSR graph propagation (PageRank, hw1 p2).

``propagate(g, x)`` is one sweep ``out[i] = 0.5/N + 0.5*sum_j x[e_j]*inv[e_j]``
(``hw/hw1/programming/pagerank.cu:70-83``) and also returns the prescaled
vector ``out*inv`` the next sweep gathers from; ``iterate`` runs the 20-sweep
ping-pong of ``device_graph_iterate`` (``:86-143``) with the prescaled-gather
kernels and no host synchronisation between sweeps.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _ext
from .algorithms import bincount
from .scan import scan

_ext.proto(_ext.HIP_PROTOS, "cme_pr_prescale", "pppip")
_ext.proto(_ext.HIP_PROTOS, "cme_pr_propagate_ref", "pppppip")
_ext.proto(_ext.HIP_PROTOS, "cme_pr_propagate", "ppppppiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_pr_propagate", "pppppi")
_ext.proto(_ext.HIP_PROTOS, "cme_pr_propagate_blocked", "pppppppiiip")


@dataclass
class CSRGraph:
    indices: torch.Tensor  # int32 (n+1,) row offsets (uint32 semantics)
    edges: torch.Tensor  # int32 (nnz,) targets
    inv_deg: torch.Tensor  # float32 (n,)

    @property
    def n(self) -> int:
        return self.inv_deg.numel()

    def to(self, device) -> "CSRGraph":
        return CSRGraph(self.indices.to(device), self.edges.to(device), self.inv_deg.to(device))


def make_graph(n: int = 1 << 21, avg_edges: int = 8, seed: int = 0) -> CSRGraph:
    """The reference generator (``pagerank.cu:185-204``): node i has
    ``(i % (2*avg-1)) + 1`` out-edges to uniformly random targets."""
    rng = np.random.default_rng(seed)
    deg = (np.arange(n, dtype=np.int64) % (2 * avg_edges - 1)) + 1
    idx = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(deg, out=idx[1:])
    if idx[-1] >= n * avg_edges:
        raise ValueError("more edges than we have space for")
    edges = rng.integers(0, n, size=int(idx[-1]), dtype=np.int64)
    inv = (1.0 / deg.astype(np.float32)).astype(np.float32)
    return CSRGraph(torch.from_numpy(idx.astype(np.int32)), torch.from_numpy(edges.astype(np.int32)),
                    torch.from_numpy(inv))


@dataclass
class BlockedGraph:
    """Edges re-sorted by (block of the gathered node, row): ``blocks`` column
    blocks of ``ceil(n / blocks)`` nodes, row offsets ``rp`` of length
    ``blocks*n + 1`` (row i of block b: ``[rp[b*n+i], rp[b*n+i+1])``); within
    a (block, row) the edges keep their CSR order."""
    rp: torch.Tensor
    edges: torch.Tensor
    inv_deg: torch.Tensor
    blocks: int

    @property
    def n(self) -> int:
        return self.inv_deg.numel()


GROUPS = (1, 2, 4, 8, 16)  # lanes per row of cme_pr_propagate
BLOCKED_GROUPS = (1, 2, 4, 8)  # ... of cme_pr_propagate_blocked


def _check_group(g, group: int) -> None:
    ok = BLOCKED_GROUPS if isinstance(g, BlockedGraph) else GROUPS
    if group not in ok:
        kind = "a column-blocked graph" if isinstance(g, BlockedGraph) else "a CSR graph"
        raise ValueError(f"group must be one of {ok} for {kind}, got {group!r}")


def _check_vector(g, x: torch.Tensor, what: str) -> None:
    """``x`` is a contiguous float32 vector of g.n entries on g's device (the
    kernels index it with the graph's node numbers and nothing else checks)."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float32:
        raise TypeError(f"{what} must be a float32 tensor")
    if x.dim() != 1 or x.numel() != g.n:
        raise ValueError(f"{what} must have shape ({g.n},), got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"{what} must be contiguous")
    if x.device != g.inv_deg.device:
        raise ValueError(f"{what} is on {x.device}, the graph on {g.inv_deg.device}")


def _edge_order(key: torch.Tensor) -> torch.Tensor:
    """Stable sorting permutation of the int64 (block, row) keys: the edges of
    one (block, row) keep their CSR order. Still ``torch.sort``:
    ``ops.sort.argsort`` gives the same permutation and measured faster on
    this shape (2^21 nodes: 2.30 against 2.72 ms for the whole preprocessing,
    ``benchmarks/bench_sort.py --block-columns``), but one row of the 64-bit
    sort's table (int64 keys with int64 values at 48M) does not beat
    ``torch.sort`` yet, and until every row does this caller stays where it
    was (profiles/sort64_r7.md)."""
    return torch.sort(key, stable=True).indices


def _row_pointers(counts: torch.Tensor, out: torch.Tensor) -> torch.Tensor:
    """Inclusive sum of the int64 (block, row) edge counts into ``out`` (an
    8-byte aligned view). This library's int64 scan: identical to the
    ``torch.cumsum`` it replaced and not slower over the whole preprocessing
    (2^21 nodes: 2.722 against 2.729 ms, five runs of each form spreading
    0.003-0.006 ms; ``benchmarks/bench_sort.py --block-columns``
    swaps this function, profiles/scan64_r8.md)."""
    return scan(counts, out=out)


def _edge_counts(key: torch.Tensor, nbins: int) -> torch.Tensor:
    """int64 number of edges per (block, row) key, ``nbins = blocks * n``
    entries: this library's ``bincount(key, nbins=)``, identical to the
    ``torch.bincount(key, minlength=nbins)`` it replaced (every key is in
    range) and not slower over the whole preprocessing (2^21 nodes: 2.598
    against 2.700 ms, five interleaved runs of each form spreading 0.015-0.020
    ms; ``benchmarks/bench_bincount.py --block-columns`` swaps this function,
    profiles/bincount.md)."""
    return bincount(key, nbins=nbins)


def block_columns(g: CSRGraph, blocks: int = 4) -> BlockedGraph:
    """Column-blocked copy of ``g`` (one-time preprocessing with tensor ops,
    on g's device): a sweep then gathers from one 1/blocks slice of the vector
    at a time (:func:`iterate` with ``blocks``)."""
    if isinstance(blocks, bool) or not isinstance(blocks, int) or blocks < 1:
        raise ValueError(f"blocks must be a positive integer, got {blocks!r}")
    n = g.n
    dev = g.edges.device
    if n == 0:
        return BlockedGraph(torch.zeros(1, dtype=torch.int32, device=dev), g.edges, g.inv_deg, blocks)
    deg = (g.indices[1:] - g.indices[:-1]).to(torch.int64)
    row = torch.repeat_interleave(torch.arange(n, device=dev), deg)
    bs = (n + blocks - 1) // blocks
    blk = g.edges.to(torch.int64) // bs
    key = blk * n + row
    order = _edge_order(key)
    edges = g.edges[order].contiguous()
    counts = _edge_counts(key, blocks * n)
    rp = torch.zeros(blocks * n + 1, dtype=torch.int64, device=dev)
    _row_pointers(counts, rp[1:])
    return BlockedGraph(rp.to(torch.int32), edges, g.inv_deg, blocks)


def propagate_ref(g: CSRGraph, x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """One sweep with the reference's two-gathers-per-edge arithmetic."""
    _check_vector(g, x, "x")
    if out is None:
        out = torch.empty_like(x)
    else:
        _check_vector(g, out, "out")
    if x.is_cuda:
        _ext.call_hip("cme_pr_propagate_ref", g.indices.data_ptr(), g.edges.data_ptr(), x.data_ptr(),
                      out.data_ptr(), g.inv_deg.data_ptr(), g.n, _ext.stream_ptr(x.device))
    else:
        _ext.call_cpu("cme_cpu_pr_propagate", g.indices.data_ptr(), g.edges.data_ptr(), x.data_ptr(),
                      out.data_ptr(), g.inv_deg.data_ptr(), g.n)
    return out


def propagate(g, x: torch.Tensor, group: int = 1, blocks: int | None = None):
    """One sweep from an unscaled ``x``: returns ``(out, y_next)`` with
    ``y_next = out * inv_deg``, the prescaled vector the next sweep gathers.
    GPU: one prescale launch and one sweep of the prescaled-gather kernels
    (``group`` lanes per row); with a :class:`BlockedGraph`, or ``blocks``
    given (``block_columns(g, blocks)`` first), the column-blocked sweep.
    CPU: the reference arithmetic (``group`` only validated)."""
    if blocks is not None:
        if isinstance(g, BlockedGraph):
            if blocks != g.blocks:
                raise ValueError(f"blocks = {blocks!r}, but the graph has {g.blocks} column blocks")
        else:
            g = block_columns(g, blocks)
    _check_group(g, group)
    _check_vector(g, x, "x")
    blocked = isinstance(g, BlockedGraph)
    if not x.is_cuda:
        if blocked:
            raise ValueError("column-blocked sweeps run on the GPU")
        out = propagate_ref(g, x)
        return out, out * g.inv_deg
    s = _ext.stream_ptr(x.device)
    n = g.n
    y, out, y_next = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    _ext.call_hip("cme_pr_prescale", x.data_ptr(), g.inv_deg.data_ptr(), y.data_ptr(), n, s)
    if blocked:
        acc = torch.empty_like(x)
        _ext.call_hip("cme_pr_propagate_blocked", g.rp.data_ptr(), g.edges.data_ptr(), y.data_ptr(), acc.data_ptr(),
                      out.data_ptr(), y_next.data_ptr(), g.inv_deg.data_ptr(), n, g.blocks, group, s)
    else:
        _ext.call_hip("cme_pr_propagate", g.indices.data_ptr(), g.edges.data_ptr(), y.data_ptr(), out.data_ptr(),
                      y_next.data_ptr(), g.inv_deg.data_ptr(), n, group, s)
    return out, y_next


def _check_iters(iters: int) -> None:
    if isinstance(iters, bool) or not isinstance(iters, int) or iters < 0:
        raise ValueError(f"iters must be a non-negative integer, got {iters!r}")
    if iters % 2:
        raise ValueError("iters must be even (A/B ping-pong, as in the reference)")


def iterate(g, x0: torch.Tensor, iters: int = 20, group: int = 1) -> torch.Tensor:
    """``iters`` sweeps (even, like the reference); returns the final vector.
    group = lanes per row on the GPU (1 keeps the CPU summation order).
    ``g`` may be a :class:`BlockedGraph` (GPU): column-blocked sweeps, each
    row summed block by block (same terms, different association order).
    ``iters == 0`` returns a copy of ``x0``; ``x0`` is a contiguous float32
    vector of ``g.n`` entries on the graph's device."""
    _check_iters(iters)
    _check_group(g, group)
    _check_vector(g, x0, "x0")
    if isinstance(g, BlockedGraph):
        return _iterate_blocked(g, x0, iters, group)
    if iters == 0:
        return x0.clone()
    if not x0.is_cuda:
        a, b = x0.clone(), torch.empty_like(x0)
        for _ in range(iters // 2):
            propagate_ref(g, a, b)
            propagate_ref(g, b, a)
        return a
    s = _ext.stream_ptr(x0.device)
    n = g.n
    out = torch.empty_like(x0)
    ya, yb = torch.empty_like(x0), torch.empty_like(x0)
    _ext.call_hip("cme_pr_prescale", x0.data_ptr(), g.inv_deg.data_ptr(), ya.data_ptr(), n, s)
    for it in range(iters):
        yi, yo = (ya, yb) if it % 2 == 0 else (yb, ya)
        _ext.call_hip("cme_pr_propagate", g.indices.data_ptr(), g.edges.data_ptr(), yi.data_ptr(), out.data_ptr(),
                      yo.data_ptr(), g.inv_deg.data_ptr(), n, group, s)
    return out


def _iterate_blocked(g: BlockedGraph, x0: torch.Tensor, iters: int, group: int) -> torch.Tensor:
    if not x0.is_cuda:
        raise ValueError("column-blocked sweeps run on the GPU")
    if iters == 0:
        return x0.clone()
    s = _ext.stream_ptr(x0.device)
    n = g.n
    out = torch.empty_like(x0)
    acc = torch.empty_like(x0)
    ya, yb = torch.empty_like(x0), torch.empty_like(x0)
    _ext.call_hip("cme_pr_prescale", x0.data_ptr(), g.inv_deg.data_ptr(), ya.data_ptr(), n, s)
    for it in range(iters):
        yi, yo = (ya, yb) if it % 2 == 0 else (yb, ya)
        _ext.call_hip("cme_pr_propagate_blocked", g.rp.data_ptr(), g.edges.data_ptr(), yi.data_ptr(), acc.data_ptr(),
                      out.data_ptr(), yo.data_ptr(), g.inv_deg.data_ptr(), n, g.blocks, group, s)
    return out


def bytes_model(g: CSRGraph, iters: int = 20) -> int:
    """The student's traffic model (``hw/hw1/programming/analysis/pagerank.cu:
    47-62``): 2 uint per node + (2 float + 2 uint) per edge + 1 float per node,
    per sweep -- used to quote GB/s comparably with BASELINE.md #5."""
    n, nnz = g.n, g.edges.numel()
    return iters * (n * 8 + nnz * 16 + n * 4)
