"""Dispatcher op of the fixed-length count: ``torch.ops.cme213x.bincount_fixed``
passes ``torch.library.opcheck`` on CPU and GPU, equals the eager
``bincount(x, nbins=)`` and ``numpy.bincount`` of the in-range elements, and
traces through ``torch.compile`` without a graph break."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.ops.algorithms import bincount
from cme213x.ops.library import OPS

ops = torch.ops.cme213x

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
_TESTS = ["test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"]


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _inputs(dev):
    """Values from -3 to 69: some fall outside every bin count used below."""
    g = torch.Generator().manual_seed(0)
    x = torch.randint(-3, 70, (3001,), generator=g)
    return {"u8": x.clamp(min=0).to(torch.uint8).to(dev), "i32": x.to(torch.int32).to(dev), "i64": x.to(dev)}


def _opcheck(dev):
    for x in _inputs(dev).values():
        for nbins in (0, 1, 64, 300):
            torch.library.opcheck(ops.bincount_fixed.default, (x, nbins), test_utils=_TESTS)


def _matches_eager_and_numpy(dev):
    assert OPS["bincount_fixed"] is not None
    for x in _inputs(dev).values():
        a = x.cpu().numpy().astype(np.int64)
        for nbins in (0, 1, 64, 300):
            r = ops.bincount_fixed(x, nbins)
            assert r.dtype == torch.int64 and tuple(r.shape) == (nbins,) and r.device == x.device
            assert torch.equal(r, bincount(x, nbins=nbins))
            want = np.bincount(a[(a >= 0) & (a < nbins)], minlength=nbins)
            assert np.array_equal(r.cpu().numpy(), want)
        r = ops.bincount_fixed(x[1:][::2], 64)  # a view the op makes contiguous
        assert torch.equal(r, bincount(x[1:][::2].contiguous(), nbins=64))


def _compiles_without_graph_break(dev):
    x = _inputs(dev)["i64"]

    def f(t):
        return ops.bincount_fixed(t + 1, 64) * 2

    r = torch.compile(f, fullgraph=True, backend="aot_eager")(x)
    assert torch.equal(r, bincount(x + 1, nbins=64) * 2)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_bincount_fixed_op(dev):
    """One test per backend (each part takes milliseconds on the GPU)."""
    _opcheck(dev)
    _matches_eager_and_numpy(dev)
    _compiles_without_graph_break(dev)
