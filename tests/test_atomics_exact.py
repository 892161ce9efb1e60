"""The lecture atomics (csrc/hip/atomics.hip), exactly: global_max over the
whole float range and at every position of its three loops, monte_carlo_pi
against the sample stream written out here, and the work queue against int64
prefix-sum differences.

Every test body runs on the CPU path (unmarked) and on the HIP kernels
(``gpu``); the argument checks sit in the wrapper and run on the CPU.
"""
import struct

import numpy as np
import pytest
import torch
from text_util import dev, seeded, view_at  # noqa: F401

from cme213x.ops.atomics import global_max, monte_carlo_pi, segment_sums_workqueue

FLT_MAX = float(np.finfo(np.float32).max)
INF = float("inf")


def bits(f: float) -> int:
    return struct.unpack("<I", struct.pack("<f", f))[0]


# ================================================================ global_max
# 15..17: one 16-float row of the launch-size formula; 1023..1025: one block of
# 256 lanes x 4 floats; 20 003: 5 blocks, where a lane runs the 4x unrolled
# vector loop or the single-vector loop, and three floats are left for the
# scalar tail
GM_N = [1, 2, 3, 4, 5, 15, 16, 17, 1023, 1024, 1025, 20_003]


@pytest.mark.parametrize("n", GM_N)
def test_global_max_sizes(dev, n):
    a = seeded("gmax", n).standard_normal(n).astype(np.float32)
    for off in (0, 1, 2, 3):  # 1..3 floats past an aligned address: the scalar path
        got = global_max(view_at(a, off, dev))
        assert isinstance(got, float) and got == float(a.max()), (n, off)


# n = 20 003 aligned: 5000 vectors, then elements 20 000..20 002 in the scalar
# tail. The grid is 5 blocks, so the stride is 1280 vectors: lanes 0..1159 take
# four vectors in the unrolled loop, lanes 1160..1279 three in the single loop.
PLANTS = [0, 20_002, 19_999, 20_000, 4 * 1159 + 3, 4 * 1160, 4 * 1279 + 2, 4 * 1280, 4 * (1160 + 2560) + 1,
          4 * (1159 + 3840), 10_001, 20_001]


def test_global_max_finds_a_plant_anywhere(dev):
    n = 20_003
    base = (-seeded("plant").random(n) - 1.0).astype(np.float32)
    x = view_at(base, 0, dev)
    assert global_max(x) == float(base.max()) <= -1.0
    for k, i in enumerate(PLANTS):
        was = float(x[i])
        x[i] = -0.5 + k / 64  # exact in float32, larger than everything else
        assert global_max(x) == -0.5 + k / 64, i
        x[i] = was
    assert global_max(x) == float(base.max())


def test_global_max_bottom_of_the_range(dev):
    """The mapped result cell starts below the image of every float, -inf
    included: maxima in [-inf, -3.3961514e38) come back as they are."""
    lowest = np.float32(-3.397e38)
    assert -FLT_MAX < float(lowest) < -3.3961514e38
    cases = {
        "-inf": np.array([-INF]),
        "all -inf": np.full(1027, -INF),
        "-FLT_MAX": np.array([-FLT_MAX]),
        "all -FLT_MAX": np.full(20_003, -FLT_MAX),
        "inside": np.linspace(-FLT_MAX, float(lowest), 1027),
        "-inf and -FLT_MAX": np.where(np.arange(1027) == 700, -FLT_MAX, -INF),
    }
    for name, a in cases.items():
        a = a.astype(np.float32)
        assert float(a.max()) <= float(lowest)
        for off in (0, 1):
            got = global_max(view_at(a, off, dev))
            assert bits(got) == bits(float(a.max())), (name, off, got)


def test_global_max_special_values(dev):
    rng = seeded("special")
    a = rng.standard_normal(1027).astype(np.float32)
    a[513] = INF
    assert global_max(view_at(a, 0, dev)) == INF
    tiny = np.float32(1e-45)  # the smallest denormal
    den = (rng.integers(-200, 200, 1027) * tiny).astype(np.float32)
    den[5] = 300 * tiny
    assert 0 < float(den.max()) < float(np.finfo(np.float32).tiny)
    for off in (0, 1):
        assert bits(global_max(view_at(den, off, dev))) == bits(float(den.max()))
    neg = (-(rng.integers(1, 200, 1027)) * tiny).astype(np.float32)  # negative denormals only
    assert bits(global_max(view_at(neg, 0, dev))) == bits(float(neg.max()))
    zeros = np.where(np.arange(1027) % 3 == 0, 0.0, -0.0).astype(np.float32)
    assert global_max(view_at(zeros, 0, dev)) == 0.0  # by value: either zero
    assert bits(global_max(view_at(np.full(17, -0.0, dtype=np.float32), 0, dev))) == bits(-0.0)
    assert global_max(view_at(np.array([FLT_MAX, -FLT_MAX], dtype=np.float32), 0, dev)) == FLT_MAX


def test_global_max_ignores_nan(dev):
    rng = seeded("nan")
    for n in (1, 5, 1027, 20_003):
        a = rng.standard_normal(n).astype(np.float32)
        a[rng.random(n) < 0.3] = np.nan
        a[0] = np.nan  # a leading NaN too
        if n > 1:
            a[n - 1] = -2.5
        want = float(np.fmax.reduce(np.concatenate([[np.float32(-INF)], a])))  # -inf when nothing else is left
        for off in (0, 1):
            assert global_max(view_at(a, off, dev)) == want, (n, off)
    for n in (1, 4, 1027):  # no number at all: -inf, as documented
        assert global_max(view_at(np.full(n, np.nan, dtype=np.float32), 0, dev)) == -INF


def test_global_max_empty_raises(dev):
    with pytest.raises(ValueError):
        global_max(torch.empty(0, dtype=torch.float32, device=dev))
    with pytest.raises(ValueError):
        global_max(torch.empty(3, 0, dtype=torch.float32, device=dev))
    with pytest.raises(TypeError):
        global_max(torch.zeros(3, dtype=torch.float64, device=dev))


# ============================================================ monte_carlo_pi
# blocks of 256 samples, waves of 64; 262 144 = the 1024-block cap x 256
MC_SAMPLES = [1, 63, 64, 65, 255, 256, 257, 262_143, 262_144, 262_145]
MC_SEEDS = [0, 1, 2**63, 2**64 - 1]
M64 = 2**64 - 1
SCALE = np.float32(2.3283064365386963e-10)  # 2^-32


def splitmix64(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def hits_scalar(samples: int, seed: int) -> int:
    """The sample stream one sample at a time, in Python integers and
    float32 scalars (each operation rounded once)."""
    h = 0
    for i in range(samples):
        r = splitmix64(seed ^ ((i * 0xD1B54A32D192ED03) & M64))
        x = np.float32(r & 0xFFFFFFFF) * SCALE
        y = np.float32(r >> 32) * SCALE
        h += bool(np.float32(x * x) + np.float32(y * y) <= np.float32(1.0))
    return h


_stream_hits: dict = {}


def hits_numpy(samples: int, seed: int) -> int:
    """The same stream, vectorised in uint64 / float32 numpy."""
    key = (samples, seed)
    if key not in _stream_hits:
        u = np.uint64
        with np.errstate(over="ignore"):
            x = u(seed) ^ (np.arange(samples, dtype=np.uint64) * u(0xD1B54A32D192ED03))
            x = x + u(0x9E3779B97F4A7C15)
            x = (x ^ (x >> u(30))) * u(0xBF58476D1CE4E5B9)
            x = (x ^ (x >> u(27))) * u(0x94D049BB133111EB)
            r = x ^ (x >> u(31))
        fx = (r & u(0xFFFFFFFF)).astype(np.float32) * SCALE
        fy = (r >> u(32)).astype(np.float32) * SCALE
        _stream_hits[key] = int(np.count_nonzero(fx * fx + fy * fy <= np.float32(1.0)))
    return _stream_hits[key]


def test_splitmix64_known_values():
    # the generator's published test vector: the first outputs for state 0
    # are splitmix64(0), splitmix64(0 + gamma), ...
    assert splitmix64(0) == 0xE220A8397B1DCDAF
    assert splitmix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4


@pytest.mark.parametrize("seed", MC_SEEDS)
def test_monte_carlo_pi_stream(dev, seed):
    name = "cpu" if dev.type == "cpu" else dev
    for samples in MC_SAMPLES:
        pi, hits = monte_carlo_pi(samples, seed, name)
        assert hits == hits_numpy(samples, seed), (samples, seed)
        assert pi == 4.0 * hits / samples
        if samples <= 1000:
            assert hits == hits_scalar(samples, seed), (samples, seed)


def test_monte_carlo_pi_arguments():
    for device in ("cpu", "cuda"):  # checked before the device is looked at
        for samples in (0, -1, -(2**40)):
            with pytest.raises(ValueError):
                monte_carlo_pi(samples, 1, device)
        with pytest.raises(ValueError):
            monte_carlo_pi(10, -1, device)
        with pytest.raises(ValueError):
            monte_carlo_pi(10, 2**64, device)


# ==================================================== segment_sums_workqueue
def wq_case(lens, first=0, seed=0):
    lens = np.asarray(lens, dtype=np.int64)
    offs = first + np.concatenate([[0], np.cumsum(lens)])
    v = seeded("wq", seed, lens.size).integers(-3, 4, int(offs[-1]) + 5)  # |sum| <= 3e5 < 2^24: exact in any order
    c = np.concatenate([[0], np.cumsum(v)])
    want = (c[offs[1:]] - c[offs[:-1]]).astype(np.float32)
    return offs.astype(np.int32), v.astype(np.float32), want


CYCLE = [0, 1, 63, 64, 65, 127, 128, 129]  # around one and two waves
WQ_CASES = {
    "no segment": ([], 0),
    "no segment, offset": ([], 7),
    "one": ([100], 0),
    "one empty": ([0], 3),
    "cycle": (CYCLE * 5, 0),
    "all empty": ([0] * 300, 11),
    "first offset not 0": (CYCLE * 3, 1000),
    "one long": ([3, 0, 70, 100_000, 1, 64, 0, 5], 2),
    # 5000 > the 4096 waves of the grid: waves come back for a second segment
    "more segments than waves": ([CYCLE[i % 8] for i in range(5000)], 0),
}


@pytest.mark.parametrize("name", list(WQ_CASES))
def test_workqueue_segment_sums(dev, name):
    lens, first = WQ_CASES[name]
    offs, v, want = wq_case(lens, first, seed=len(name))
    got = segment_sums_workqueue(torch.from_numpy(offs).to(dev), torch.from_numpy(v).to(dev))
    assert got.dtype == torch.float32 and got.device.type == dev.type
    assert torch.equal(got.cpu(), torch.from_numpy(want)), name
    if len(lens) and max(lens) == 0:
        assert not got.cpu().any()


def test_workqueue_int64_offsets(dev):
    offs, v, want = wq_case(CYCLE * 2, 5)
    got = segment_sums_workqueue(torch.from_numpy(offs.astype(np.int64)).to(dev), torch.from_numpy(v).to(dev))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_workqueue_arguments():
    with pytest.raises(ValueError):
        segment_sums_workqueue(torch.empty(0, dtype=torch.int32), torch.zeros(4))
    with pytest.raises(TypeError):
        segment_sums_workqueue(torch.tensor([0, 2], dtype=torch.int32), torch.zeros(4, dtype=torch.float64))
