"""Dispatcher op and model of the 64-bit segmented scan:
``torch.ops.cme213x.segmented_scan`` passes ``torch.library.opcheck`` with
int64 and float64 input, and ``SpmvScanSolver(dtype=torch.float64)`` steps as
it runs."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.models.spmv_scan import SpmvScanSolver, generate
from cme213x.ops.scan import segmented_scan

ops = torch.ops.cme213x

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
_TESTS = ["test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"]
U = 2.0 ** -53


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _inputs(dev):
    g = torch.Generator().manual_seed(0)
    n = 4097
    heads = (torch.rand(n, generator=g) < 0.01).to(torch.uint8)
    words = torch.from_numpy(np.packbits(np.pad(heads.numpy(), (0, -n % 32)), bitorder="little").view(np.int32).copy())
    return {
        "i64": torch.randint(-2 ** 40, 2 ** 40, (n,), generator=g, dtype=torch.int64).to(dev),
        "f64": torch.randint(0, 2 ** 20, (n,), generator=g, dtype=torch.int64).double().to(dev),
    }, {"u8": heads.to(dev), "bits": words.to(dev)}


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("flags", ["u8", "bits"])
@pytest.mark.parametrize("name", ["i64", "f64"])
def test_opcheck_segmented_scan64(dev, name, flags):
    xs, fs = _inputs(dev)
    torch.library.opcheck(ops.segmented_scan.default, (xs[name], fs[flags]), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_op_matches_eager_and_oracle(dev):
    xs, fs = _inputs(dev)
    h = fs["u8"].cpu().long()
    h[0] = 1
    seg = torch.cumsum(h, 0) - 1
    for x in xs.values():
        c = torch.cumsum(x.cpu(), 0)
        ref = c - (c - x.cpu())[torch.nonzero(h).flatten()][seg]  # integers below 2^53: exact in float64 too
        for f in fs.values():
            got = ops.segmented_scan(x, f)
            assert got.dtype == x.dtype
            assert torch.equal(got, segmented_scan(x, f))
            assert torch.equal(got.cpu(), ref)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_solver_float64_step_matches_run(dev):
    """step() (segmented_scan with mul, in place) and run(1) (spmv_scan_run)
    compute the same sums, each within the worst-case bound of any summation
    order, (m + 1) terms with the product's rounding, of a longdouble oracle."""
    prob = generate(37035, 3128, 1000, 6, seed=1, dtype=np.float64)
    a, b = SpmvScanSolver(prob, dev, dtype=torch.float64), SpmvScanSolver(prob, dev, dtype=torch.float64)
    assert a.a.dtype == a.xx.dtype == torch.float64
    a.step()
    b.run(1)
    v = prob.a.astype(np.longdouble) * prob.x[prob.k].astype(np.longdouble)
    s = prob.s.astype(np.int64)
    ref = np.empty(prob.n, dtype=np.longdouble)
    asum = np.empty(prob.n)
    for lo, hi in zip(s[:-1], s[1:]):
        ref[lo:hi] = np.cumsum(v[lo:hi])
        asum[lo:hi] = np.cumsum(np.abs(v[lo:hi]).astype(np.float64))
    m = np.arange(prob.n) - np.repeat(s[:-1], np.diff(s)) + 1
    bound = 1.01 * (m + 1) * U * asum
    for sol in (a, b):
        err = np.abs(sol.a.cpu().numpy().astype(np.longdouble) - ref)
        assert np.all(err <= bound), float((err - bound).max())
    a.reset()
    assert torch.equal(a.a.cpu(), torch.from_numpy(prob.a))
    if dev.type == "cuda":
        from cme213x.ops.scan import lookback_timed_out

        assert not lookback_timed_out(dev)


def test_solver_float64_rejects_float32_only_algorithms():
    prob = generate(1000, 50, 100, 2)
    for algo in ("wave", "serial"):
        with pytest.raises(ValueError, match="float32 only"):
            SpmvScanSolver(prob, "cpu", algo=algo, dtype=torch.float64)
    with pytest.raises(ValueError, match="dtype"):
        SpmvScanSolver(prob, "cpu", dtype=torch.float16)
