"""Dispatcher op and in-project callers of the 64-bit scan:
``torch.ops.cme213x.scan`` passes ``torch.library.opcheck`` with int64 and
float64 input, ``dist_scan`` works on int64 / float64 shards, and
``graph.block_columns`` still gives the row pointers ``torch.cumsum`` gave."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.ops import graph as G
from cme213x.ops.scan import scan
from dist_util import run_ranks

ops = torch.ops.cme213x

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
_TESTS = ["test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"]


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _inputs(dev):
    g = torch.Generator().manual_seed(0)
    return {
        "i64": torch.randint(-2 ** 40, 2 ** 40, (4097,), generator=g, dtype=torch.int64).to(dev),
        "f64": torch.randint(0, 2 ** 20, (4097,), generator=g, dtype=torch.int64).double().to(dev),
    }


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("name", ["i64", "f64"])
def test_opcheck_scan64(dev, name, exclusive):
    torch.library.opcheck(ops.scan.default, (_inputs(dev)[name], exclusive), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_op_matches_eager_and_cumsum(dev):
    for x in _inputs(dev).values():
        for excl in (False, True):
            got = ops.scan(x, excl)
            assert got.dtype == x.dtype
            assert torch.equal(got, scan(x, exclusive=excl))
            ref = torch.cumsum(x.cpu(), 0) - (x.cpu() if excl else 0)
            assert torch.equal(got.cpu(), ref)


def _dist_scan64_rank(rank, world, seed):
    import cme213x  # noqa: F401
    from cme213x.parallel.comm import TorchComm
    from cme213x.parallel.dist_scan import dist_scan

    rng = np.random.default_rng(seed)
    n = 10_007
    xi = rng.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    xf = rng.integers(0, 2 ** 20, n).astype(np.float64)
    cuts = sorted(rng.choice(np.arange(1, n), world - 1, replace=False).tolist())  # uneven shards
    bounds = [0] + cuts + [n]
    lo, hi = bounds[rank], bounds[rank + 1]
    c = TorchComm()
    out = [dist_scan(torch.from_numpy(x[lo:hi].copy()), c, exclusive=e).numpy()
           for x in (xi, xf) for e in (False, True)]
    return lo, hi, out


def test_dist_scan_int64_float64_gloo():
    world = 3
    rng = np.random.default_rng(7)
    n = 10_007
    xi = rng.integers(-2 ** 40, 2 ** 40, n, dtype=np.int64)
    xf = rng.integers(0, 2 ** 20, n).astype(np.float64)
    refs = [np.cumsum(xi), np.cumsum(xi) - xi, np.cumsum(xf), np.cumsum(xf) - xf]
    seen = 0
    for lo, hi, out in run_ranks(_dist_scan64_rank, world, (7,)):
        assert hi > lo
        seen += hi - lo
        for got, ref in zip(out, refs):
            assert got.dtype == ref.dtype
            np.testing.assert_array_equal(got, ref[lo:hi])
    assert seen == n


@pytest.mark.gpu
def test_dist_scan_int64_loopback_gpu(gpu):
    from cme213x.parallel.comm import LoopbackComm
    from cme213x.parallel.dist_scan import dist_scan

    x = torch.randint(-2 ** 40, 2 ** 40, (70_001,), generator=torch.Generator().manual_seed(1), dtype=torch.int64)
    for excl in (False, True):
        y = dist_scan(x.to(gpu), LoopbackComm(), exclusive=excl)
        assert torch.equal(y.cpu(), torch.cumsum(x, 0) - (x if excl else 0))


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_block_columns_row_pointers_unchanged(dev):
    """2^12-node graph: the BlockedGraph arrays equal the ones computed with
    torch.sort and torch.cumsum, and the library's int64 scan of the counts
    gives the same row pointers."""
    g = torch.Generator().manual_seed(5)
    n, blocks = 1 << 12, 4
    deg = torch.randint(0, 12, (n,), generator=g)
    indices = torch.zeros(n + 1, dtype=torch.int32)
    indices[1:] = torch.cumsum(deg, 0).to(torch.int32)
    edges = torch.randint(0, n, (int(indices[-1]),), generator=g, dtype=torch.int32)
    inv = 1.0 / torch.clamp(deg, min=1).to(torch.float32)
    got = G.block_columns(G.CSRGraph(indices.to(dev), edges.to(dev), inv.to(dev)), blocks)
    row = torch.repeat_interleave(torch.arange(n), deg)
    key = (edges.to(torch.int64) // ((n + blocks - 1) // blocks)) * n + row
    counts = torch.bincount(key, minlength=blocks * n)
    rp = torch.zeros(blocks * n + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(counts, 0)
    assert got.blocks == blocks and got.rp.dtype == torch.int32
    assert torch.equal(got.rp.cpu(), rp.to(torch.int32))
    assert torch.equal(got.edges.cpu(), edges[torch.sort(key, stable=True).indices])
    assert torch.equal(got.inv_deg.cpu(), inv)
    ours = torch.zeros(blocks * n + 1, dtype=torch.int64, device=dev)
    scan(counts.to(dev), out=ours[1:])  # an 8-byte aligned out= view, as the call would use
    assert torch.equal(ours.cpu(), rp)
