"""Dispatcher op of the scans along a dimension: ``torch.ops.cme213x.scan_dim``
passes ``torch.library.opcheck`` on CPU and GPU for float32 and int64, in the
row and the column form, and equals the eager call and torch."""
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.ops.library import OPS
from cme213x.ops.scan import scan

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
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("op,dim", [("sum", 1), ("sum", -1), ("max", 0), ("min", 2)])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_opcheck_scan_dim(dev, name, op, dim, exclusive):
    torch.library.opcheck(ops.scan_dim.default, (_inputs(dev)[name], dim, op, exclusive), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_op_matches_eager_and_torch(dev):
    assert OPS["scan_dim"] is not None
    for x in _inputs(dev).values():
        for dim in (0, 1, 2, -2):
            got = ops.scan_dim(x, dim, "sum", False)
            assert got.dtype == x.dtype and got.shape == x.shape and got.data_ptr() != x.data_ptr()
            assert torch.equal(got, scan(x, dim=dim))
            assert torch.equal(got.cpu(), torch.cumsum(x.cpu(), dim))  # integer-valued: exact in float32 too
            for op, f in (("max", torch.cummax), ("min", torch.cummin)):
                assert torch.equal(ops.scan_dim(x, dim, op, False).cpu(), f(x.cpu(), dim).values)
            ex = ops.scan_dim(x, dim, "sum", True).cpu()
            assert torch.equal(ex, got.cpu() - x.cpu())
    with pytest.raises(ValueError, match="op"):
        ops.scan_dim(x, 0, "prod", False)
    with pytest.raises(IndexError):
        ops.scan_dim(x, 3, "sum", False)
