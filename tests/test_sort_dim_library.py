"""Dispatcher op of the sort along a dimension: ``torch.ops.cme213x.sort_dim``
passes ``torch.library.opcheck`` on CPU and GPU, equals the eager
``sort(x, dim=)`` and, on data without NaN and ``-0.0``,
``torch.sort(stable=True)``, and traces through ``torch.compile`` without a
graph break."""
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.ops.library import OPS
from cme213x.ops.sort import sort

ops = torch.ops.cme213x

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
_TESTS = ["test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"]


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _inputs(dev):
    """Heavy ties (draws from 101 values over 131-element lines): stability shows."""
    g = torch.Generator().manual_seed(0)
    shape = (5, 131, 12)
    return {
        "f32": (torch.randint(-50, 51, shape, generator=g).float() + 0.5).to(dev),
        "i64": (7 * torch.randint(-50, 51, shape, generator=g) - 2 ** 53).to(dev),
    }


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("dim", [0, 1, -1])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_opcheck_sort_dim(dev, name, dim, descending):
    torch.library.opcheck(ops.sort_dim.default, (_inputs(dev)[name], dim, descending), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_op_matches_eager_and_torch(dev):
    assert OPS["sort_dim"] is not None
    for x in _inputs(dev).values():
        for dim in (0, 1, 2, -2):
            for descending in (False, True):
                v, i = ops.sort_dim(x, dim, descending)
                e = sort(x, dim=dim, descending=descending)
                assert torch.equal(v, e.values) and torch.equal(i, e.indices)
                tv, ti = torch.sort(x.cpu(), dim=dim, stable=True, descending=descending)
                assert torch.equal(v.cpu(), tv) and torch.equal(i.cpu(), ti)
        v, i = ops.sort_dim(x, 1)  # the schema's default
        assert torch.equal(i, sort(x, dim=1).indices)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_compiles_without_graph_break(dev):
    x = _inputs(dev)["f32"]

    def f(t):
        v, i = ops.sort_dim(t, 1, True)
        return v * 2, i + 1

    v, i = torch.compile(f, fullgraph=True, backend="aot_eager")(x)
    e = sort(x, dim=1, descending=True)
    assert torch.equal(v, e.values * 2) and torch.equal(i, e.indices + 1)
