"""Dispatcher ops of the reductions along a dimension:
``torch.ops.cme213x.reduce_dim`` / ``max_dim`` / ``min_dim`` pass
``torch.library.opcheck`` on CPU and GPU, trace through ``torch.compile``
without a graph break, and a chunked ``reduce(..., dim=)`` replays from a HIP
graph."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.ops.library import OPS
from cme213x.ops.scan import reduce

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
    shape = (5, 131, 12)
    ramp = torch.arange(131, dtype=torch.int64).view(1, -1, 1)
    return {
        "f32": (ramp + torch.randint(-50, 51, shape, generator=g)).float().to(dev),
        "i64": (7 * (ramp + torch.randint(-50, 51, shape, generator=g)) - 2 ** 53).to(dev),
    }


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("keepdim", [False, True])
@pytest.mark.parametrize("op,dim", [("sum", 1), ("sum", -1), ("max", 0), ("min", 2)])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_opcheck_reduce_dim(dev, name, op, dim, keepdim):
    torch.library.opcheck(ops.reduce_dim.default, (_inputs(dev)[name], dim, op, keepdim), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("keepdim", [False, True])
@pytest.mark.parametrize("dim", [0, 1, -1])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_opcheck_max_dim_min_dim(dev, name, dim, keepdim):
    x = _inputs(dev)[name]
    torch.library.opcheck(ops.max_dim.default, (x, dim, keepdim), test_utils=_TESTS)
    torch.library.opcheck(ops.min_dim.default, (x, dim, keepdim), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_ops_match_eager_and_torch(dev):
    assert all(OPS[k] is not None for k in ("reduce_dim", "max_dim", "min_dim"))
    for x in _inputs(dev).values():
        for dim in (0, 1, 2, -2):
            for keep in (False, True):
                got = ops.reduce_dim(x, dim, "sum", keep)
                assert got.dtype == x.dtype and torch.equal(got, reduce(x, "sum", dim=dim, keepdim=keep))
                assert torch.equal(got.cpu(), x.cpu().sum(dim, keepdim=keep))  # integer-valued: exact in float32 too
                assert torch.equal(ops.reduce_dim(x, dim, "max", keep).cpu(), x.cpu().amax(dim, keepdim=keep))
                for f, t in ((ops.max_dim, torch.max), (ops.min_dim, torch.min)):
                    v, i = f(x, dim, keep)
                    tv, ti = t(x.cpu(), dim, keepdim=keep)
                    assert i.dtype == torch.int64 and torch.equal(i.cpu(), ti) and torch.equal(v.cpu(), tv)
    with pytest.raises(ValueError, match="op"):
        ops.reduce_dim(x, 0, "prod", False)
    with pytest.raises(IndexError):
        ops.max_dim(x, 3, False)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_compile_fullgraph(dev):
    """A normalised cdf's last column is one: scan, reduce and max_dim in one
    traced function, no graph break."""

    def f(p):
        total = ops.reduce_dim(p, -1, "sum", True)
        top, where = ops.max_dim(p, -1, False)
        return ops.scan_dim(p, -1, "sum", False) / total, top, where

    p = (_inputs(dev)["f32"].abs() + 1.0)
    cdf, top, where = torch.compile(f, fullgraph=True, backend="aot_eager")(p)
    e_cdf, e_top, e_where = f(p)
    assert torch.equal(cdf, e_cdf) and torch.equal(top, e_top) and torch.equal(where, e_where)
    assert torch.equal(where.cpu(), p.cpu().argmax(-1)) and torch.equal(cdf[..., -1].cpu(), torch.ones(5, 131))


@pytest.mark.gpu
def test_graph_capture_of_a_chunked_reduce(gpu):
    """One capture of a chunked sum and a chunked indexed max, run once eagerly
    first (the partials are sized outside the capture), replayed on changed
    inputs and compared bitwise with the eager call; then a larger eager call,
    which retires the buffer the graph still holds, and one more replay."""
    from cme213x.utils import tuning

    shape = (3, 301, 64)
    rng = np.random.default_rng(7)
    x = torch.zeros(shape, dtype=torch.float32, device=gpu)
    with tuning.override(scan_dim_chunks=5):
        reduce(x, "sum", dim=1)
        reduce(x, "max", dim=1, return_indices=True)
        torch.cuda.synchronize(gpu)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            s = reduce(x, "sum", dim=1)
            v, i = reduce(x, "max", dim=1, return_indices=True)

        def replay_and_compare(seed):
            a = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32))
            x.copy_(a)
            graph.replay()
            torch.cuda.synchronize(gpu)
            es = reduce(x, "sum", dim=1)
            ev, ei = reduce(x, "max", dim=1, return_indices=True)
            assert torch.equal(s.view(torch.int32), es.view(torch.int32))
            assert torch.equal(v.view(torch.int32), ev.view(torch.int32)) and torch.equal(i, ei)
            tv, ti = torch.max(a, 1)
            assert torch.equal(i.cpu(), ti) and torch.equal(v.cpu(), tv)

        replay_and_compare(1)
        big = torch.ones((64, 4099, 64), dtype=torch.float32, device=gpu)
        assert (reduce(big, "sum", dim=1) == 4099).all()
        assert (reduce(big, "min", dim=1, return_indices=True).indices == 0).all()
        replay_and_compare(2)
