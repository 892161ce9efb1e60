"""Dispatcher op and distributed caller of the max / min scans:
``torch.ops.cme213x.scan_op`` passes ``torch.library.opcheck`` on CPU and GPU
for float32 and int64, and ``dist_scan(op="max" / "min")`` of unevenly sharded
float64 and int64 vectors on 3 gloo ranks -- an empty shard and a NaN in the
middle rank included -- equals the single-vector oracle bit for bit."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
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
    n = 16384 + 4097  # two look-back tiles of float32, three of int64
    ramp = torch.arange(n, dtype=torch.int64)
    return {
        "f32": (ramp + torch.randint(-50, 51, (n,), generator=g)).float().to(dev),
        "i64": (7 * (ramp + torch.randint(-50, 51, (n,), generator=g)) - 2 ** 53).to(dev),
    }


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("exclusive", [False, True])
@pytest.mark.parametrize("op", ["max", "min", "sum"])
@pytest.mark.parametrize("name", ["f32", "i64"])
def test_opcheck_scan_op(dev, name, op, exclusive):
    torch.library.opcheck(ops.scan_op.default, (_inputs(dev)[name], op, exclusive), test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_op_matches_eager_and_torch(dev):
    for x in _inputs(dev).values():
        for op, f in (("max", torch.cummax), ("min", torch.cummin)):
            got = ops.scan_op(x, op, False)
            assert got.dtype == x.dtype and got.data_ptr() != x.data_ptr()
            assert torch.equal(got, scan(x, op=op))
            assert torch.equal(got.cpu(), f(x.cpu(), 0).values)
            ex = ops.scan_op(x, op, True).cpu()
            assert torch.equal(ex[1:], got.cpu()[:-1])
        assert torch.equal(ops.scan_op(x, "sum", False), ops.scan(x, False))
    with pytest.raises(ValueError, match="op"):
        ops.scan_op(x, "prod", False)


def _bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.int64)


N = 10_007


def _vectors(op: str):
    """(float64, int64) data of a "max" scan, mirrored for "min": noisy ramps
    with both zeros in different shards and the default NaN in the middle rank."""
    rng = np.random.default_rng(7)
    sign = 1 if op == "max" else -1
    i = np.arange(N, dtype=np.int64)
    xf = sign * (i - 4_500 + rng.uniform(-50, 50, N)).astype(np.float64)
    xf[[2_999, 3_003]] = [0.0, -0.0]  # on either side of the first shard edge; the ramp is near -1500 there
    xf[5_000] = np.nan
    xi = sign * (7 * (i + rng.integers(-50, 51, N)) - 2 ** 53)
    return xf, xi


def _shards(world: int):
    """Rank bounds of 3 ranks: uneven, and (second layout) with rank 1 empty."""
    return [[0, 3_001, 7_500, N], [0, 3_001, 3_001, N]]


def _dist_rank(rank, world):
    import cme213x  # noqa: F401
    from cme213x.parallel.comm import TorchComm
    from cme213x.parallel.dist_scan import dist_scan

    c = TorchComm()
    out = []
    for bounds in _shards(world):
        lo, hi = bounds[rank], bounds[rank + 1]
        for op in ("max", "min"):
            for x in _vectors(op):
                for e in (False, True):
                    shard = torch.from_numpy(x[lo:hi].copy())
                    out.append((lo, hi, dist_scan(shard, c, exclusive=e, op=op).numpy()))
    return out


def test_dist_scan_max_min_gloo():
    world = 3
    refs = []
    for _ in _shards(world):
        for op in ("max", "min"):
            for x in _vectors(op):
                inc = (torch.cummax if op == "max" else torch.cummin)(torch.from_numpy(x), 0).values.numpy()
                if x.dtype == np.float64:
                    ident = -np.inf if op == "max" else np.inf
                else:
                    ident = np.iinfo(np.int64).min if op == "max" else np.iinfo(np.int64).max
                refs += [inc, np.concatenate([np.array([ident], dtype=x.dtype), inc[:-1]])]
    assert np.isnan(refs[0][5_000:]).all() and not np.isnan(refs[0][:5_000]).any()
    empty = 0
    for out in run_ranks(_dist_rank, world):
        assert len(out) == len(refs)
        for (lo, hi, got), ref in zip(out, refs):
            empty += hi == lo
            assert got.dtype == ref.dtype and got.shape == (hi - lo,)
            bad = np.flatnonzero(_bits(got) != _bits(ref[lo:hi]))
            assert bad.size == 0, (lo, hi, bad[:3], got[bad[:3]], ref[lo:hi][bad[:3]])
    assert empty == len(refs) // 2  # rank 1 of the second layout


@pytest.mark.gpu
def test_dist_scan_max_loopback_gpu(gpu):
    from cme213x.parallel.comm import LoopbackComm
    from cme213x.parallel.dist_scan import dist_scan

    for op, f in (("max", torch.cummax), ("min", torch.cummin)):
        for x in _vectors(op):
            t = torch.from_numpy(x)
            y = dist_scan(t.to(gpu), LoopbackComm(), op=op).cpu().numpy()
            assert np.array_equal(_bits(y), _bits(f(t, 0).values.numpy()))
