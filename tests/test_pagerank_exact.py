"""PageRank propagation, exactly: every kernel of csrc/hip/graph.hip and the
CPU backend against an int64 numpy oracle, bit for bit, on data whose row sums
do not depend on the summation order (generator, oracles and the derived
multi-sweep bound: graph_util.py).

Unmarked tests run the oracles' self-checks and the CPU backend; ``gpu`` tests
run the HIP kernels. Single sweeps (``propagate`` / ``propagate_ref``) are
compared bitwise, ``out`` and ``y_next``; the only tolerance in this file is
``graph_util.sweep_bound`` for several sweeps against a float64 reference.
"""
import graph_util as G
import numpy as np
import pytest
import torch

from cme213x.ops.graph import (BlockedGraph, CSRGraph, block_columns, iterate, make_graph, propagate,
                               propagate_ref)

CPU = torch.device("cpu")
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000]
GROUPS = [1, 2, 4, 8, 16]
BLOCKS = [1, 2, 3, 5, 8]
BLOCKED_GROUPS = [1, 2, 4, 8]


# ------------------------------------------------------------------ data sets
def single(total, n, at):
    lens = np.zeros(n, dtype=np.int64)
    lens[at] = total
    return lens


def _make(name):
    kind, n = name
    if kind == "mixed":
        return G.int_graph(G.mixed_lens(n, seed=n), n, seed=n)
    if kind == "mixed19":  # each length of MIXED_LENS once, shuffled, between two empty rows
        lens = np.concatenate([[0], np.random.default_rng(19).permutation(G.MIXED_LENS), [0]])
        return G.int_graph(lens, n, seed=19)
    if kind == "one_row":
        return G.int_graph(single(5000, n, 137), n, seed=1)
    if kind == "no_edges":
        return G.int_graph(np.zeros(n, dtype=np.int64), n, seed=2)
    if kind == "to_node0":
        return G.int_graph(G.mixed_lens(n, seed=3), n, seed=3, allowed=[0])
    if kind == "low_cols":  # only the first 120 nodes are gathered: the upper column blocks are empty
        return G.int_graph(G.mixed_lens(n, seed=4), n, seed=4, allowed=np.arange(120))
    if kind == "high_cols":  # only the last 120: the FIRST column block(s) are empty
        return G.int_graph(G.mixed_lens(n, seed=5), n, seed=5, allowed=np.arange(n - 120, n))
    raise KeyError(name)


CASES = [("mixed", n) for n in SIZES] + [("mixed19", 21), ("one_row", 257), ("no_edges", 300), ("to_node0", 257),
                                         ("low_cols", 1000), ("high_cols", 1000)]
CASE_IDS = [f"{k}-{n}" for k, n in CASES]


def case(name):
    """(graph, x, exact out, exact y_next) on the host, built once."""
    def make():
        g = _make(name)
        x = G.int_x(g.n, seed=g.n)
        out, y = G.exact_sweep(g, x)
        return g, x, out, y
    return G.cached(("case", name), make)


def on_gpu(name, dev):
    def make():
        g, x, _, _ = case(name)
        return g.to(dev), x.to(dev)
    return G.cached(("gpu", name), make)


def multi_graph(which):
    def make():
        if which == "make_graph":
            return make_graph(1000, 8, seed=7)
        return G.true_inverse(case(("mixed", 1000))[0])
    return G.cached(("multi", which), make)


def multi_ref(which, iters):
    """(float64 reference, relative bound) of ``iters`` sweeps from x0 = 1/n."""
    def make():
        g = multi_graph(which)
        return G.sweeps64(g, uniform(g.n), iters), G.sweep_bound(g, iters)
    return G.cached(("multi_ref", which, iters), make)


def uniform(n):
    return torch.full((n,), 1.0 / n, dtype=torch.float32)


# ============================================================ CPU: the oracles
def test_cases_cover_what_they_claim():
    g = case(("mixed", 1000))[0]
    deg = np.diff(g.indices.numpy())
    assert set(deg.tolist()) == set(G.MIXED_LENS) and deg[0] == 0 and deg[-1] == 0
    e, rows = g.edges.numpy(), G.row_ids(g.indices.numpy().astype(np.int64))
    assert (e == rows).any() and (e == 0).any() and (e == 999).any()  # self-loops, both end nodes
    b = g.indices.numpy()
    assert any(len(set(e[b[r]:b[r + 1]].tolist())) < b[r + 1] - b[r] for r in range(1000))  # duplicates in a row
    assert set(np.unique(g.inv_deg.numpy()).tolist()) == {1.0, 0.5, 0.25, 0.125}
    g19 = case(("mixed19", 21))[0]
    d19 = np.diff(g19.indices.numpy())
    assert sorted(d19[1:-1].tolist()) == sorted(G.MIXED_LENS) and d19[0] == 0 and d19[-1] == 0
    assert np.diff(case(("one_row", 257))[0].indices.numpy()).max() == 5000 == case(("one_row", 257))[0].edges.numel()
    assert case(("no_edges", 300))[0].edges.numel() == 0
    assert int(case(("to_node0", 257))[0].edges.max()) == 0
    assert int(case(("low_cols", 1000))[0].edges.max()) < 120 and int(case(("high_cols", 1000))[0].edges.min()) >= 880


def test_no_edges_gives_the_constant():
    _, _, out, _ = case(("no_edges", 300))
    assert torch.equal(out, torch.full((300,), np.float32(0.5) / np.float32(300)))


def test_oracle_rejects_inexact_data():
    """The exactness precondition is checked inside the oracle."""
    g, x, _, _ = case(("mixed", 64))
    with pytest.raises(AssertionError):
        G.exact_sweep(g, x * 0.3)
    with pytest.raises(AssertionError):
        G.exact_sweep(G.true_inverse(g), x)  # 1/3, 1/5, ...
    m = 1 << 18  # one row of 2**18 terms of 120 units each: 1.875 * 2**24
    long = CSRGraph(torch.tensor([0, m, m, m], dtype=torch.int32), torch.ones(m, dtype=torch.int32), torch.ones(3))
    with pytest.raises(AssertionError, match="row sum too large"):
        G.exact_sweep(long, torch.full((3,), 15 / 16))


@pytest.mark.parametrize("name", CASES, ids=CASE_IDS)
def test_oracle_agrees_with_float64_reference(name):
    """The two independent references against each other: the int64 oracle's
    single sweep lies within the one-sweep bound of the float64 reference."""
    g, x, out, y = case(name)
    ref = G.sweeps64(g, x, 1)
    G.assert_within(out, ref, G.sweep_bound(g, 1), f"{name}: int64 oracle vs float64")
    assert np.array_equal(y.numpy().astype(np.float64), out.numpy().astype(np.float64) * g.inv_deg.numpy())


def test_float64_reference_by_hand():
    """3 nodes, worked by hand: row 0 gathers {1, 2}, row 1 nothing, row 2 {0, 0}."""
    g = CSRGraph(torch.tensor([0, 2, 2, 4], dtype=torch.int32), torch.tensor([1, 2, 0, 0], dtype=torch.int32),
                 torch.tensor([0.5, 0.25, 1.0]))
    x = torch.tensor([0.5, 0.25, 0.75])
    want = np.array([1 / 6 + 0.5 * (0.25 * 0.25 + 0.75), 1 / 6, 1 / 6 + 0.5 * (0.25 + 0.25)])
    assert np.allclose(G.sweeps64(g, x, 1), want, rtol=1e-15, atol=0)
    out, y = G.exact_sweep(g, x)
    c = np.float32(0.5) / np.float32(3)
    assert out.tolist() == [float(np.float32(c + np.float32(0.40625))), float(c), float(np.float32(c + np.float32(0.25)))]
    assert y.tolist() == [out[0].item() * 0.5, out[1].item() * 0.25, out[2].item()]


# ============================================================ CPU: the backend
@pytest.mark.parametrize("name", CASES, ids=CASE_IDS)
def test_cpu_single_sweep_exact(name):
    g, x, out, y = case(name)
    G.assert_same(propagate_ref(g, x), out, f"{name}: propagate_ref")
    o, yn = propagate(g, x)
    G.assert_same(o, out, f"{name}: propagate out")
    G.assert_same(yn, y, f"{name}: propagate y_next")


@pytest.mark.parametrize("which", ["make_graph", "mixed_true"])
@pytest.mark.parametrize("iters", [2, 4, 20])
def test_cpu_multi_sweep_within_bound(which, iters):
    g = multi_graph(which)
    ref, bound = multi_ref(which, iters)
    G.assert_within(iterate(g, uniform(g.n), iters), ref, bound, f"{which}, {iters} sweeps, cpu")


def test_mass_reference_and_cpu():
    """sum(x) = 1 is conserved per sweep on a graph with inv = 1 / (times
    gathered): by the float64 reference to 1e-12, by the backend within the
    sum of the per-node bounds (n terms; their total is bound * sum(ref))."""
    n = 1024
    g = G.mass_graph(n, seed=11)
    x0 = uniform(n)  # 2**-10: sums to exactly 1
    for s in (1, 2, 4, 20):
        ref = G.sweeps64(g, x0, s)
        assert abs(ref.sum() - 1.0) <= 1e-12
    ref, bound = G.sweeps64(g, x0, 20), G.sweep_bound(g, 20)
    out = iterate(g, x0, 20)
    G.assert_within(out, ref, bound, "mass graph, 20 sweeps, cpu")
    assert abs(out.double().sum().item() - 1.0) <= bound * ref.sum() + 1e-12


# ========================================================= CPU: block_columns
def check_blocked(g: CSRGraph, bg: BlockedGraph, blocks: int):
    n = g.n
    rp_want, edges_want = G.blocked_oracle(g, blocks)
    rp = bg.rp.cpu().numpy().astype(np.int64)
    edges = bg.edges.cpu().numpy().astype(np.int64)
    assert bg.blocks == blocks and bg.n == n and rp.shape == (blocks * n + 1,)
    assert rp[0] == 0 and np.all(np.diff(rp) >= 0) and rp[-1] == g.edges.numel()
    bs = -(-n // blocks)
    blk = np.repeat(np.arange(blocks * n) // n, np.diff(rp))  # block of every stored edge
    assert np.all((edges >= blk * bs) & (edges < (blk + 1) * bs))
    # CSR order kept within a (block, row), everything else too: the stable sort
    assert np.array_equal(rp, rp_want) and np.array_equal(edges, edges_want)


BLOCK_CASES = [(("mixed", 1000), 3), (("mixed", 1000), 7), (("mixed", 257), 5), (("mixed", 257), 8), (("mixed", 2), 5),
               (("mixed", 1), 3), (("mixed", 63), 64), (("mixed", 63), 200), (("no_edges", 300), 1),
               (("no_edges", 300), 7), (("low_cols", 1000), 8), (("high_cols", 1000), 2), (("mixed19", 21), 1)]


@pytest.mark.parametrize("name,blocks", BLOCK_CASES, ids=[f"{k}-{n}-b{b}" for (k, n), b in BLOCK_CASES])
def test_block_columns_cpu(name, blocks):
    g = case(name)[0]
    check_blocked(g, block_columns(g, blocks), blocks)


def test_block_columns_without_nodes():
    g = CSRGraph(torch.zeros(1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0))
    bg = block_columns(g, 4)
    assert bg.n == 0 and bg.blocks == 4 and bg.rp.tolist() == [0] and bg.edges.numel() == 0


# ================================================================== CPU: edges
def empty_graph(dev=CPU):
    return CSRGraph(torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev),
                    torch.zeros(0, device=dev))


def check_no_nodes(dev):
    g = empty_graph(dev)
    x = torch.zeros(0, device=dev)
    assert propagate_ref(g, x).shape == (0,)
    for group in GROUPS:
        out, y = propagate(g, x, group)
        assert out.shape == (0,) and y.shape == (0,) and out.device == x.device
        assert iterate(g, x, 2, group).shape == (0,)
    if dev.type == "cuda":
        for blocks in (1, 3):
            for group in BLOCKED_GROUPS:
                out, y = propagate(g, x, group, blocks=blocks)
                assert out.shape == (0,) and y.shape == (0,)
                assert iterate(block_columns(g, blocks), x, 4, group).shape == (0,)
        torch.cuda.synchronize()


def check_zero_iters(g, x0, groups):
    for group in groups:
        out = iterate(g, x0, 0, group)
        assert out is not x0 and out.data_ptr() != x0.data_ptr() and torch.equal(out, x0)


def check_rejections(g, x0, bg=None):
    """Everything here raises in Python, before any launch."""
    n = g.n
    for bad in (1, 3, 19, -2):
        with pytest.raises(ValueError):
            iterate(g, x0, bad)
    for bad in (0, 3, 5, 32, -1):
        with pytest.raises(ValueError):
            iterate(g, x0, 2, bad)
        with pytest.raises(ValueError):
            propagate(g, x0, bad)
    for bad in (0, -1, 2.5):
        with pytest.raises(ValueError):
            block_columns(g, bad)
    if bg is not None:
        with pytest.raises(ValueError):
            iterate(bg, x0, 2, 16)
        with pytest.raises(ValueError):
            propagate(bg, x0, 16)
        with pytest.raises(ValueError):
            iterate(bg, x0, 3, 2)
        with pytest.raises(ValueError):
            propagate(bg, x0, 1, blocks=bg.blocks + 1)
    wrong = [x0.double(), x0.to(torch.int32)]
    for x in wrong:
        for f in (lambda: iterate(g, x, 2), lambda: propagate(g, x), lambda: propagate_ref(g, x)):
            with pytest.raises(TypeError):
                f()
    two = torch.cat([x0, x0])
    other = torch.empty(n, device="meta") if x0.device.type == "cpu" else x0.cpu()
    for x in (x0[:-1], two, x0.view(1, n), two[::2], other):
        for f in (lambda: iterate(g, x, 2), lambda: propagate(g, x), lambda: propagate_ref(g, x)):
            with pytest.raises(ValueError):
                f()
    for out in (two[::2], x0[:-1].clone(), other):
        with pytest.raises(ValueError):
            propagate_ref(g, x0, out)
    with pytest.raises(TypeError):
        propagate_ref(g, x0, x0.double())


def test_no_nodes_cpu():
    check_no_nodes(CPU)


def test_zero_iters_cpu():
    g, x, _, _ = case(("mixed", 65))
    check_zero_iters(g, x, [1, 4])


def test_rejections_cpu():
    g, x, _, _ = case(("mixed", 65))
    check_rejections(g, x)
    with pytest.raises(ValueError):  # blocked sweeps have no CPU backend
        propagate(g, x, blocks=2)
    with pytest.raises(ValueError):
        iterate(block_columns(g, 2), x, 2)


# ======================================================== GPU: one sweep, exact
# The gpu tests loop over their cases inside one test each (every case runs
# before the test fails and the message names all that differ): the suite
# already holds thousands of gpu test ids, and these add four.
def single_sweep_gpu(name, gpu, wrong):
    _, _, out, y = case(name)
    g, x = on_gpu(name, gpu)
    runs = [(f"group {k}", g, k) for k in GROUPS]
    for blocks in BLOCKS:
        bg = block_columns(g, blocks)
        check_blocked(case(name)[0], bg, blocks)
        if name[0] in ("low_cols", "high_cols") and blocks > 1:
            per_block = np.diff(bg.rp.cpu().numpy().astype(np.int64)[::g.n])
            assert (per_block == 0).any() and per_block[0 if name[0] == "low_cols" else -1] > 0
            assert (per_block[0] == 0) == (name[0] == "high_cols")
        runs += [(f"blocks {blocks}, group {k}", bg, k) for k in BLOCKED_GROUPS]

    def compare(got, want, what):
        try:
            G.assert_same(got, want, f"{name}: {what}")
        except AssertionError as e:
            wrong.append(str(e))

    compare(propagate_ref(g, x), out, "pr_ref_kernel")
    for what, gr, group in runs:
        o, yn = propagate(gr, x, group)
        compare(o, out, f"{what}: out")
        compare(yn, y, f"{what}: y_next")


@pytest.mark.gpu
def test_gpu_single_sweep_exact(gpu):
    """Every graph of CASES through pr_ref_kernel; prescale_kernel +
    pr_scalar_kernel / pr_group_kernel<G>; prescale_kernel +
    pr_blocked_kernel<G> over ``blocks`` launches (first, middle, last) for
    every G: ``out`` and ``y_next`` equal the int64 oracle. Then
    ``propagate(g, x, group, blocks=b)`` on a CSR graph, which blocks it first."""
    wrong = []
    for name in CASES:
        single_sweep_gpu(name, gpu, wrong)
    assert not wrong, f"{len(wrong)} comparisons differ:\n" + "\n".join(wrong[:40])
    _, _, out, y = case(("mixed", 257))
    g, x = on_gpu(("mixed", 257), gpu)
    o, yn = propagate(g, x, 2, blocks=3)
    G.assert_same(o, out, "blocks=3: out")
    G.assert_same(yn, y, "blocks=3: y_next")


# ======================================================= GPU: several sweeps
def multi_sweep_gpu(which, gpu, wrong):
    g = multi_graph(which)
    gd, x0 = g.to(gpu), uniform(g.n).to(gpu)
    blocked = {b: block_columns(gd, b) for b in (1, 2, 3, 8)}
    worst = 0.0
    for iters in (2, 4, 20):
        ref, bound = multi_ref(which, iters)
        runs = [(f"group {k}", gd, k) for k in GROUPS]
        runs += [(f"blocks {b}, group {k}", blocked[b], k) for b, k in ((1, 1), (2, 2), (3, 4), (8, 8), (2, 1), (8, 2))]
        for what, gr, group in runs:
            try:
                worst = max(worst, G.assert_within(iterate(gr, x0, iters, group), ref, bound,
                                                   f"{which}, {iters} sweeps, {what}") / bound)
            except AssertionError as e:
                wrong.append(str(e))
    print(f"{which}: worst error / bound = {worst:.4f}")
    # group 1 keeps the CPU order: bitwise equal to the CPU backend
    if not torch.equal(iterate(gd, x0, 20, 1).cpu(), iterate(g, uniform(g.n), 20)):
        wrong.append(f"{which}: group 1 differs from the CPU backend")


@pytest.mark.gpu
def test_gpu_multi_sweep_within_bound(gpu):
    wrong = []
    for which in ("make_graph", "mixed_true"):
        multi_sweep_gpu(which, gpu, wrong)
    assert not wrong, "\n".join(wrong)


@pytest.mark.gpu
def test_gpu_mass(gpu):
    n = 1024
    g = G.mass_graph(n, seed=11)
    gd, x0 = g.to(gpu), uniform(n).to(gpu)
    ref, bound = G.sweeps64(g, uniform(n), 20), G.sweep_bound(g, 20)
    assert abs(ref.sum() - 1.0) <= 1e-12
    runs = [(gd, k) for k in GROUPS] + [(block_columns(gd, b), k) for b, k in ((2, 1), (3, 2), (5, 4), (8, 8))]
    for gr, group in runs:
        out = iterate(gr, x0, 20, group)
        G.assert_within(out, ref, bound, f"mass graph, group {group}")
        assert abs(out.double().sum().item() - 1.0) <= bound * ref.sum() + 1e-12


# ================================================================== GPU: edges
@pytest.mark.gpu
def test_edges_gpu(gpu):
    """No nodes; ``iters == 0``; everything that raises before a launch."""
    check_no_nodes(gpu)
    g, x = on_gpu(("mixed", 65), gpu)
    check_zero_iters(g, x, GROUPS)
    check_zero_iters(block_columns(g, 3), x, BLOCKED_GROUPS)
    check_rejections(g, x, block_columns(g, 2))
