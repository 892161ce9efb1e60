"""Dispatcher ops of the running max / min with indices:
``torch.ops.cme213x.cummax`` / ``cummin`` pass ``torch.library.opcheck`` on CPU
and GPU for float32 and int64, in the row and the column form, equal the eager
call and ``torch.cummax`` / ``torch.cummin`` on CPU tensors, and trace under
``torch.compile(fullgraph=True)`` with both outputs in use."""
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.ops.library import OPS
from cme213x.ops.scan import cummax, cummin

ops = torch.ops.cme213x

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
_TESTS = ["test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"]


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _inputs(dev):
    """Values in {0..3}: ties everywhere, so the index moves while the value
    stands still (int64 beyond 2^53)."""
    g = torch.Generator().manual_seed(0)
    shape = (5, 131, 12)
    return {
        "f32": torch.randint(0, 4, shape, generator=g).float().to(dev),
        "i64": (torch.randint(0, 4, shape, generator=g) - 2 ** 53 - 2).to(dev),
    }


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("dim", [0, 1, -1])
@pytest.mark.parametrize("op", ["cummax", "cummin"])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_opcheck_cumarg(dev, name, op, dim):
    torch.library.opcheck(getattr(ops, op).default, (_inputs(dev)[name], dim), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_ops_match_eager_and_torch(dev):
    assert OPS["cummax"] is not None and OPS["cummin"] is not None
    for x in _inputs(dev).values():
        for dim in (0, 1, 2, -2):
            for op, eager, ref in ((ops.cummax, cummax, torch.cummax), (ops.cummin, cummin, torch.cummin)):
                v, i = op(x, dim)
                assert v.dtype == x.dtype and i.dtype == torch.int64 and v.shape == i.shape == x.shape
                assert v.data_ptr() != x.data_ptr()
                e = eager(x, dim=dim, return_indices=True)
                assert torch.equal(v, e.values) and torch.equal(i, e.indices)
                want = ref(x.cpu(), dim)
                assert torch.equal(v.cpu(), want.values) and torch.equal(i.cpu(), want.indices)
    with pytest.raises(IndexError):
        ops.cummax(x, 3)
    with pytest.raises(TypeError):
        ops.cummin(x.half(), 0)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_compile_uses_both_outputs(dev):
    """No graph break: the fake kernels give both outputs' shape and dtype."""

    def peak_and_where(x):
        v, i = torch.ops.cme213x.cummax(x, 1)
        w, j = torch.ops.cme213x.cummin(x, 1)
        return v - w, i - j, torch.gather(x, 1, i)

    x = _inputs(dev)["f32"]
    got = torch.compile(peak_and_where, fullgraph=True, backend="aot_eager")(x)
    hi, lo = torch.cummax(x.cpu(), 1), torch.cummin(x.cpu(), 1)
    assert torch.equal(got[0].cpu(), hi.values - lo.values)
    assert got[1].dtype == torch.int64 and torch.equal(got[1].cpu(), hi.indices - lo.indices)
    assert torch.equal(got[2].cpu(), hi.values)  # x at the winner's index is the running value
