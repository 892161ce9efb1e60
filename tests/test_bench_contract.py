"""bench.py contract: the multi-rank control flow (torch.distributed.run
launch, decomposition, barriers, max-over-ranks timing, one JSON line from
rank 0) exercised end to end on CPU ranks (gloo + OpenMP backend)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from dist_util import free_port

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _launch(nproc, extra):
    env = dict(os.environ, OMP_NUM_THREADS="1", MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(REPO, "bench.py"),
           "--gpus", str(nproc), "--steps", "5", "--warmup", "1", "--grid", "192", "--device", "cpu", "--full",
           *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout  # exactly one JSON line (rank 0)
    return json.loads(lines[0])


@pytest.mark.parametrize("nproc,extra", [(2, []), (4, ["--method", "2"]), (3, ["--mode", "sync", "--tblock", "1"])])
def test_bench_multirank_cpu(nproc, extra):
    rec = _launch(nproc, extra)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in rec
    assert rec["n_gpus"] == nproc and rec["steps"] == 5 and rec["warmup"] == 1
    assert rec["sanity_ok"] is True and rec["value"] > 0
    assert rec["config"]["loop"] == "torch.distributed"


@pytest.mark.parametrize("mode", ["halo", "allgather"])
def test_dist_spmv_bench_cpu(mode):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=3", "--master-addr",
           "127.0.0.1", "--master-port", str(free_port()), os.path.join(REPO, "benchmarks", "bench_dist_spmv.py"),
           "--grid", "64", "--steps", "3", "--warmup", "1", "--device", "cpu", "--mode", mode]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["n_gpus"] == 3 and rec["max_abs_err"] < 1e-4
    if mode == "halo":  # 64x64 grid in 3 row blocks: neighbours only, about one grid row each way
        assert rec["max_peers_per_rank"] == 2 and rec["max_halo_values_per_rank"] <= 2 * 64 + 2


def _launch_gpu(nproc, extra):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}",
           "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.join(REPO, "bench.py"),
           "--gpus", str(nproc), "--steps", "20", "--warmup", "3", "--spinup", "0", "--grid", "2048", "--full",
           *extra]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
@pytest.mark.timeout(300)
@pytest.mark.parametrize("nproc,extra", [(2, []), (4, ["--method", "2", "--tblock", "4"])])
def test_bench_multirank_shared_gpu_ipc(gpu, nproc, extra):
    """The driver's N>1 bench flow (torch.distributed.run, one process per
    rank, native loop after its bitwise self-test) rehearsed on ONE GPU: every
    rank on cuda:0, gloo control plane, IPC halo transport."""
    rec = _launch_gpu(nproc, ["--share-gpu", *extra])
    assert rec["n_gpus"] == nproc and rec["sanity_ok"] is True
    assert rec["native_selftest"] is True and rec["selftest"] is True
    assert rec["config"]["loop"] == "native-ipc" and rec["config"]["rehearsal_shared_gpu"] is True
    assert rec["config"]["transport"] == "ipc" and rec["config"]["schedule"].split()[0] in ("fused", "events")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_single_gpu_selftest(gpu):
    """N = 1 (the driver's BENCH run): the timed path -- one native
    multi-pass call per loop -- passes its bitwise self-test against single
    FMA steps and names its schedule."""
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--steps", "9", "--warmup", "5", "--grid", "2048",
           "--spinup", "0.05", "--full"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    rec = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("{")][0])
    assert rec["selftest"] is True and rec["sanity_ok"] is True
    assert rec["steps"] == 9 and rec["warmup"] == 5
    assert rec["config"]["schedule"] and rec["config"]["transport"] == "none"


# keys only --full puts into the line (a plain run times the headline alone)
FULL_ONLY = ("ms_per_step_uniform", "value_uniform", "ms_per_step_dist_schedule", "cpu_transpose_1024_ms", "copy_ms",
             "transpose_vec_ms", "scan_lookback_ms", "spmv_csr_ms")


def _plain(extra, dump):
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", *extra,
           "--dump-outputs", str(dump)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=REPO,
                         env=dict(os.environ, OMP_NUM_THREADS="1"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    rec = json.loads(lines[0])
    assert rec["steps"] == 7 and rec["warmup"] == 2 and rec["ms_per_step"] > 0 and rec["value"] > 0
    for k in ("metric", "unit", "higher_is_better", "dtype"):
        assert k in rec
    assert rec["selftest"] is None and rec["sanity_ok"] is None
    assert not [k for k in FULL_ONLY if k in rec] and not [k for k in rec if k.endswith(("_fma", "_fast"))]
    assert os.listdir(dump) == ["state_rank0.npy"]
    return np.load(os.path.join(dump, "state_rank0.npy"))


def test_bench_plain_dump_cpu(tmp_path):
    """A plain run prints the headline alone, and --dump-outputs writes the
    state after the last timed step: here (CPU dry run, 96^2, uniform IC) the
    whole owned interior, equal to 2 + 7 steps of the single-grid oracle and
    the same from run to run."""
    import torch

    from cme213x.models.heat2d import HeatGrid
    from cme213x.utils.params import SimParams

    extra = ["--grid", "96", "--device", "cpu", "--arith", "exact"]
    a = _plain(extra, tmp_path / "a")
    b = _plain(extra, tmp_path / "b")
    assert a.dtype == np.float32 and a.shape == (96, 96) and np.array_equal(a, b)
    p = SimParams(nx=96, ny=96, iters=9, order=8, ic=5.0, bc=(0.0, 10.0, 0.0, 10.0), flavor="hw5")  # bench.py's
    g = HeatGrid(p, torch.float32, "cpu")
    g.run(9, "naive")
    B = p.border
    want = g.state()[B:B + 96, B:B + 96]
    assert np.array_equal(a, np.asarray(want, dtype=np.float32))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_plain_dump_gpu(gpu, tmp_path):
    """The plain N = 1 run on the GPU (random-init headline, 4096^2: above the
    dump's size cap, so a sample): no --full key in the line, and two runs
    dump the same finite values bit for bit."""
    extra = ["--grid", "4096", "--spinup", "0.05"]
    a = _plain(extra, tmp_path / "a")
    b = _plain(extra, tmp_path / "b")
    assert a.dtype == np.float32 and a.ndim == 1 and a.nbytes == 32 << 20
    # bench.py's own sanity bound; the order-8 weights are not all positive, so no maximum principle
    assert np.isfinite(a).all() and np.abs(a).max() <= 1e3 and a.min() < a.max()
    assert np.array_equal(a, b)
