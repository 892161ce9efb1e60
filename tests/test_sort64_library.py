"""Dispatcher ops and in-project callers of the 64-bit / descending sorts:
``torch.ops.cme213x.argsort`` and ``sort`` / ``sort_by_key`` with int64 keys
pass ``torch.library.opcheck``; ``graph.block_columns`` gives the same
blocked graph with ``argsort`` of its int64 keys as with ``torch.sort``, and
``vigenere.solve_cipher`` (descending sort_by_key of the digraph counts)
returns the ranking its numpy predecessor returned."""
import numpy as np
import pytest
import torch

import cme213x  # noqa: F401  (registers the ops)
from cme213x.models.vigenere import create_cipher, solve_cipher
from cme213x.ops import graph as G
from cme213x.ops import sort as S
from cme213x.ops.text import digraph_histogram

ops = torch.ops.cme213x

DEVS = [pytest.param("cpu", id="cpu"), pytest.param("gpu", marks=pytest.mark.gpu, id="gpu")]
_TESTS = ["test_schema", "test_autograd_registration", "test_faketensor", "test_aot_dispatch_dynamic"]


@pytest.fixture
def dev(request):
    if request.param == "gpu":
        return request.getfixturevalue("gpu")
    return torch.device("cpu")


def _cases(dev):
    g = torch.Generator().manual_seed(0)
    k64 = torch.randint(-10 ** 12, 10 ** 12, (4097,), generator=g, dtype=torch.int64).to(dev)
    k32 = torch.randint(-1000, 1000, (4097,), generator=g, dtype=torch.int32).to(dev)
    f64 = torch.randn(4097, generator=g, dtype=torch.float64).to(dev)
    return {
        "argsort_i64": (ops.argsort.default, (k64,)),
        "argsort_i64_desc": (ops.argsort.default, (k64, True)),
        "argsort_i32": (ops.argsort.default, (k32,)),
        "argsort_f64": (ops.argsort.default, (f64,)),
        "sort_i64": (ops.sort.default, (k64,)),
        "sort_f64": (ops.sort.default, (f64,)),
        "sort_by_key_i64_i64": (ops.sort_by_key.default, (k64, torch.arange(4097, dtype=torch.int64).to(dev))),
        "sort_by_key_i64_f32": (ops.sort_by_key.default, (k64, torch.arange(4097, dtype=torch.float32).to(dev))),
    }


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("name", list(_cases("cpu")))
def test_opcheck(dev, name):
    op, args = _cases(dev)[name]
    torch.library.opcheck(op, args, test_utils=_TESTS)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_ops_match_eager(dev):
    from cme213x.ops.library import OPS

    assert "argsort" in OPS
    c = _cases(dev)
    k64, k32 = c["argsort_i64"][1][0], c["argsort_i32"][1][0]
    for x in (k64, k32):
        for d in (False, True):
            got = ops.argsort(x, d)
            assert got.dtype == torch.int64
            assert torch.equal(got, S.argsort(x, descending=d))
            assert torch.equal(got.cpu(), torch.sort(x.cpu(), stable=True, descending=d).indices)
    assert torch.equal(ops.argsort(k64), ops.argsort(k64, False))
    assert torch.equal(ops.sort(k64).cpu(), torch.sort(k64.cpu()).values)
    k, v = ops.sort_by_key(*c["sort_by_key_i64_i64"][1])
    ref = torch.sort(k64.cpu(), stable=True)
    assert torch.equal(k.cpu(), ref.values) and torch.equal(v.cpu(), ref.indices)


@pytest.mark.parametrize("dev", DEVS, indirect=True)
@pytest.mark.parametrize("blocks", [1, 4, 7])
def test_block_columns_equals_library_sort(dev, blocks):
    g = torch.Generator().manual_seed(blocks)
    n = 1500
    deg = torch.randint(0, 12, (n,), generator=g)
    indices = torch.zeros(n + 1, dtype=torch.int32)
    indices[1:] = torch.cumsum(deg, 0).to(torch.int32)
    nnz = int(indices[-1])
    edges = torch.randint(0, n, (nnz,), generator=g, dtype=torch.int32)
    inv = 1.0 / torch.clamp(deg, min=1).to(torch.float32)
    csr = G.CSRGraph(indices.to(dev), edges.to(dev), inv.to(dev))
    got = G.block_columns(csr, blocks)
    # ... and with this library's argsort as the edge order (a drop-in: the same stable permutation)
    shipped = G._edge_order
    G._edge_order = S.argsort
    try:
        ours = G.block_columns(csr, blocks)
    finally:
        G._edge_order = shipped
    assert torch.equal(ours.rp, got.rp) and torch.equal(ours.edges, got.edges)
    # the same preprocessing with torch.sort
    row = torch.repeat_interleave(torch.arange(n), deg)
    bs = (n + blocks - 1) // blocks
    key = (edges.to(torch.int64) // bs) * n + row
    order = torch.sort(key, stable=True).indices
    rp = torch.zeros(blocks * n + 1, dtype=torch.int64)
    rp[1:] = torch.cumsum(torch.bincount(key, minlength=blocks * n), 0)
    assert got.blocks == blocks and got.rp.dtype == torch.int32
    assert torch.equal(got.rp.cpu(), rp.to(torch.int32))
    assert torch.equal(got.edges.cpu(), edges[order])


@pytest.mark.parametrize("dev", DEVS, indirect=True)
def test_solve_cipher_top_digraphs(dev):
    rng = np.random.default_rng(0)
    en = np.array([8.17, 1.49, 2.78, 4.25, 12.70, 2.23, 2.02, 6.09, 6.97, 0.15, 0.77, 4.03, 2.41, 6.75, 7.51, 1.93,
                   0.10, 5.99, 6.33, 9.06, 2.76, 0.98, 2.36, 0.15, 1.97, 0.07])
    book = rng.choice(np.arange(97, 123, dtype=np.uint8), 60000, p=en / en.sum())
    cipher, key = create_cipher(book, 17, device=dev, out_path=None)
    r = solve_cipher(cipher, device=dev, out_path=None, verbose=False)
    assert r["key_length"] == 17
    dg = digraph_histogram(torch.from_numpy(cipher).to(dev)).cpu().numpy().ravel()
    order = np.argsort(-dg, kind="stable")[:20]
    npairs = cipher.size // 2
    want = [(chr(97 + i // 26) + chr(97 + i % 26), dg[i] / npairs) for i in order]
    assert r["top_digraphs"] == want  # ties resolved by the lower digraph id (stable descending order)
