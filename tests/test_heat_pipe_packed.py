"""The packed-pair row update of the wide-lane pipelined fast pass (heat_pipe.h
arithmetic code 6, launched by cme_heat_pipe_fast_f32 for 2-4 steps per pass):
explicit float pairs for the centre row, the DPP halo moves written into pair
elements, one shuffle per odd-aligned pair, and a role-0 input window the
loads land in directly (12 slots, unrolled over 6 phases; roles 1.. keep the
10-slot window and its 5-phase unroll).

Every check is torch.equal against the CPU fast oracle (heat_step(..., "fast")
applied ns times) on seeded random data. The cases walk what the new code
paths depend on: steps per pass, the strip start relative to the 8-column lane
grid, partial / exact / spilling strips, the number of phases per chunk modulo
both unroll periods, row clamping at the grid's first and last rows, and the
unmasked (interior) and masked (edge) instantiations."""
import pytest
import torch

from cme213x.models.heat2d import HeatGrid
from cme213x.ops.stencil import heat_step, heat_stepn
from cme213x.utils.params import SimParams

NX, NY = 1140, 200
RB, B = 2, 4  # rows per phase, stencil border (order 8)


def _strip(ns):
    """Output columns of one strip: 64 lanes of 8 columns less the whole lanes
    covering the ns*B columns lost per side (heat_region.h PipeOut)."""
    return (64 - 2 * ((ns * B + 7) // 8)) * 8


def _phases(h, ns):
    """Phases a chunk of h rows runs: rows y0 - 2(ns-1)B .. y1 in blocks of RB."""
    return (h + 2 * (ns - 1) * B + RB - 1) // RB


def _chunk_heights(H, chunk):
    c = ((chunk + RB - 1) // RB) * RB
    return [min(c, H - y) for y in range(0, H, c)]


_cache = {}


def _grids(gpu):
    """The random field on both devices and, per ns, the CPU field after
    ns - 1 fast steps over the interior (computed once, never modified)."""
    if "g" not in _cache:
        p = SimParams(nx=NX, ny=NY, order=8)
        c = HeatGrid(p, torch.float32)
        gen = torch.Generator().manual_seed(7)
        c.buf[0].copy_(torch.rand(c.buf[0].shape, generator=gen, dtype=torch.float32) * 10.0)
        _cache["g"] = (c, c.buf[0].to(gpu))
        src = c.buf[0].clone()
        for ns in (2, 3, 4):
            tmp = src.clone()
            heat_step(src, tmp, c.interior, 8, c.xcfl, c.ycfl, "fast")
            src = tmp
            _cache[ns] = src
    return _cache["g"]


def _check(gpu, ns, regions, chunk):
    c, dev0 = _grids(gpu)
    want = c.buf[0].clone()
    for reg in regions:
        heat_step(_cache[ns], want, reg, 8, c.xcfl, c.ycfl, "fast")
    out = dev0.clone()
    heat_stepn(dev0, out, regions, c.interior, 8, c.xcfl, c.ycfl, ns, chunk=chunk, fma="fast", kernel="pipe")
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), want)


# (yb, ye, chunk): chunk 0 = the launcher's rule (2-row chunks on regions this small)
ROWS = [(4, 204, 2), (4, 204, 4), (4, 204, 6), (4, 204, 8), (4, 204, 10), (4, 204, 12),  # first and last rows
        (4, 6, 0), (4, 7, 0), (201, 204, 0), (202, 204, 0),  # 2 and 3 rows at either end of the grid
        (4, 7, 4), (201, 204, 4), (100, 105, 6),  # one 3-row / 5-row chunk
        (50, 87, 10), (33, 48, 16), (90, 101, 12), (60, 129, 14)]  # odd heights


def test_rows_cover_both_unroll_periods():
    """The chunk heights above give phase counts in every residue class of
    the 5-phase (roles 1..) and the 6-phase (role 0) unroll, for each ns."""
    for ns in (2, 3, 4):
        n = {_phases(h, ns) for yb, ye, ch in ROWS for h in _chunk_heights(ye - yb, ch or RB)}
        assert {v % 5 for v in n} == set(range(5)) and {v % 6 for v in n} == set(range(6)), (ns, sorted(n))
    hs = {h for yb, ye, ch in ROWS for h in _chunk_heights(ye - yb, ch or RB)}
    assert {2, 3} <= hs and any(h % 2 for h in hs if h > 3)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("x0", [4, 9, 12, 130])
@pytest.mark.parametrize("width", ["100", "strip", "strip+1", "2strip+9"])
def test_gpu_packed_strips_bitwise(gpu, ns, x0, width):
    """Strip geometry: the region's first column on / off the 8-column lane
    grid, at the grid edge (4) and well inside (130: whole strips there run
    the unmasked instantiation); partial, exact and spilling strips."""
    s = _strip(ns)
    w = {"100": 100, "strip": s, "strip+1": s + 1, "2strip+9": 2 * s + 9}[width]
    assert x0 + w <= B + NX
    _check(gpu, ns, [(x0, x0 + w, 30, 67)], 10)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("yb,ye,chunk", ROWS)
def test_gpu_packed_rows_bitwise(gpu, ns, yb, ye, chunk):
    """Chunk heights over every residue of both unroll periods, over the full
    width (left and right grid edges: masked), with chunks that start at the
    first and end at the last interior row (input rows clamped to the grid)."""
    _check(gpu, ns, [(B, B + NX, yb, ye)], chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("chunk", [0, 18])
def test_gpu_packed_inside_bitwise(gpu, ns, chunk):
    """A region of whole strips far from every grid edge: every task runs the
    unmasked instantiation."""
    s = _strip(ns)
    _check(gpu, ns, [(136, 136 + 2 * s, 40, 150)], chunk)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [2, 3, 4])
@pytest.mark.parametrize("edge", ["left", "right", "top", "bottom"])
def test_gpu_packed_edges_bitwise(gpu, ns, edge):
    """A region touching exactly one grid edge (masked instantiation)."""
    reg = {"left": (4, 300, 60, 120), "right": (700, B + NX, 60, 120), "top": (200, 800, 4, 50),
           "bottom": (200, 800, 150, B + NY)}[edge]
    _check(gpu, ns, [reg], 12)


@pytest.mark.gpu
@pytest.mark.parametrize("ns", [2, 3, 4])
def test_gpu_packed_three_regions_bitwise(gpu, ns):
    """Interior + two border strips in one launch (the distributed schedule)."""
    xb, xe, yb, ye = B, B + NX, B, B + NY
    _check(gpu, ns, [(xb, xe, yb + 20, ye - 20), (xb, xe, yb, yb + 20), (xb, xe, ye - 20, ye)], 0)
