"""Final project: the iterated segmented "SpMV-scan".

Problem (``hw/hw_final/Final.pdf``; reference checker
``hw/hw_final/programming/aux/reference_spMVscan-released.cu:38-54``):
repeat N times ``b_j = sum_{l=s_i}^{j} a_l * x[k_l]`` for j in segment
``[s_i, s_{i+1})``, then ``a <- b``.

MI355X design (vs. the reference's one-32-lane-warp-per-segment kernel,
``fp.cu:28-59``, which is racy on anything but lock-step Fermi and loses badly
on short segments): x is pre-gathered once (``xx = x[k]``, outside the timed
region, as the rules allow -- ``fp.cu:124-125``), segment heads become a 1-bit
mask, and each iteration is ONE single-pass kernel: 16-B loads of a and xx,
fused multiply, DPP segmented wave scans, decoupled look-back across 4096-
element tiles whose walk stops at the first tile containing a head. Traffic:
12 B/element/iteration + n/8 B of flags -- independent of segment lengths.

I/O parity: ``a.txt`` (``n p q N`` / a[n] / s[p] / k[n]), ``x.txt`` (x[q]),
``b.txt`` (``v `` per element), the line ``"The running time of my code for
<N> iterations is: <ms> milliseconds."`` and the checker's L2 / Linf errors.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _ext
from ..ops.scan import head_flags_from_offsets, segmented_scan, spmv_scan_run
from ..utils.gridio import write_vector
from ..utils.timer import EventTimer


@dataclass
class SpmvScanProblem:
    a: np.ndarray  # float32 [n] (float64 when loaded / generated in double)
    s: np.ndarray  # int32 [p]   (s[0] = 0, s[p-1] = n)
    k: np.ndarray  # int32 [n]   (0 <= k < q)
    x: np.ndarray  # float32 [q] (float64 in double)
    iters: int

    @property
    def n(self) -> int:
        return self.a.size

    @property
    def p(self) -> int:
        return self.s.size

    @property
    def q(self) -> int:
        return self.x.size

    def validate(self) -> None:
        """The loader's invariants (``aux/mp1-util.h:104-147``)."""
        assert self.s[0] == 0 and self.s[-1] == self.n, "s must start at 0 and end at n"
        assert np.all(np.diff(self.s) > 0), "s must be strictly increasing"
        assert self.k.min() >= 0 and self.k.max() < self.q, "k out of range"


def load(a_path: str, x_path: str, dtype=np.float32) -> SpmvScanProblem:
    """``dtype``: the element type of ``a`` and ``x`` (float32, or float64 to
    keep every digit of the files)."""
    tok = np.fromfile(a_path, sep=" ")
    n, p, q, N = (int(v) for v in tok[:4])
    a = tok[4:4 + n].astype(dtype)
    s = tok[4 + n:4 + n + p].astype(np.int64).astype(np.int32)
    k = tok[4 + n + p:4 + n + p + n].astype(np.int64).astype(np.int32)
    x = np.fromfile(x_path, sep=" ")[:q].astype(dtype)
    prob = SpmvScanProblem(a, s, k, x, N)
    prob.validate()
    return prob


def save(prob: SpmvScanProblem, a_path: str, x_path: str) -> None:
    with open(a_path, "w") as f:
        f.write(f"{prob.n} {prob.p} {prob.q} {prob.iters}\n")
        f.write(" ".join(repr(float(v)) for v in prob.a) + " \n")
        f.write(" ".join(str(int(v)) for v in prob.s) + "\n")
        f.write(" ".join(str(int(v)) for v in prob.k) + " \n")
    with open(x_path, "w") as f:
        f.write(" ".join(repr(float(v)) for v in prob.x) + " \n")


def generate(n: int, p: int, q: int, iters: int, seed: int = 0, values: np.ndarray | None = None,
             dtype=np.float32) -> SpmvScanProblem:
    """readMM.py's generator (``aux/readMM.py:16-61``): s = 0, a sorted random
    sample of size p (its first element dropped), n; k ~ U[0, q); x ~ U(-1, 1).
    ``values`` (the matrix entries) default to U(-1, 1) -- the benchmark
    matrices themselves are not in the reference repo. ``dtype``: float32 or float64
    (the same random stream, not rounded to float32)."""
    rng = np.random.default_rng(seed)
    a = values.astype(dtype) if values is not None else rng.uniform(-1, 1, n).astype(dtype)
    samp = np.sort(rng.choice(n, size=p, replace=False))
    s = np.empty(p, dtype=np.int32)
    s[0] = 0
    s[1:p - 1] = samp[1:p - 1]
    s[p - 1] = n
    k = rng.integers(0, q, size=n, dtype=np.int64).astype(np.int32)
    x = rng.uniform(-1, 1, q).astype(dtype)
    return SpmvScanProblem(a, s, k, x, iters)


# (n, p, N) of the 15 benchmark matrices (from the checker log)
BENCH_SHAPES = {
    "cant": (4007383, 62450, 50), "consph": (6010480, 83333, 20), "cop20k_A": (2624331, 121191, 73),
    "dense2": (4000000, 1999, 10), "jonheart": (37035, 3128, 60), "mac_econ_fwd500": (1273389, 206499, 12),
    "mc2depi": (2100225, 525824, 70), "pdb1HYS": (4344765, 36416, 30), "pwtk": (11634424, 217917, 25),
    "qcd5_4": (1916928, 49151, 63), "rail4284": (11279748, 4283, 10), "rma10": (2374001, 46834, 74),
    "scircuit": (958936, 170997, 30), "shipsec1": (7813404, 140873, 10), "webbase-1M": (3105536, 1000004, 77),
}
# GTX 580 ms for each (Final_Report_DongBang_Tsai.tex:237-251)
REF_MS = {"cant": 107.911, "consph": 62.117, "cop20k_A": 146.603, "dense2": 26.676, "jonheart": 2.665,
          "mac_econ_fwd500": 23.544, "mc2depi": 302.068, "pdb1HYS": 63.582, "pwtk": 158.697, "qcd5_4": 74.608,
          "rail4284": 58.752, "rma10": 99.947, "scircuit": 47.816, "shipsec1": 42.401, "webbase-1M": 592.115}


_ext.proto(_ext.HIP_PROTOS, "cme_segscan_offsets_run", "pppiiip")

ALGOS = ("lookback", "wave", "serial")


class SpmvScanSolver:
    """Device-resident state: a (updated in place), xx = x[k], head bitmask.

    ``algo``: "lookback" (default; single-pass decoupled look-back segmented
    scan over the whole array, load-balanced whatever the segment lengths),
    "wave" (one wave per segment: the reference's ``fp.cu`` algorithm, made
    race-free with a DPP scan), "serial" (one lane per segment: ``fp_old.cu``).
    The last two are GPU-only comparison variants, float32 only.

    ``dtype``: ``torch.float32`` or ``torch.float64``, the type the state is
    held and every step is computed in (the problem's arrays are converted)."""

    def __init__(self, prob: SpmvScanProblem, device="cuda", algo: str = "lookback",
                 dtype: torch.dtype = torch.float32):
        if algo not in ALGOS:
            raise ValueError(f"algo must be one of {ALGOS}")
        if dtype not in (torch.float32, torch.float64):
            raise ValueError("dtype must be torch.float32 or torch.float64")
        if dtype == torch.float64 and algo != "lookback":
            raise ValueError(f"algo {algo!r} is float32 only; float64 takes 'lookback'")
        self.dtype = dtype
        self.prob = prob
        self.algo = algo
        self.device = torch.device(device)
        if algo != "lookback" and self.device.type != "cuda":
            raise ValueError(f"algo {algo!r} is a GPU kernel")
        self.offsets = torch.from_numpy(prob.s.astype(np.int32)).to(self.device)
        x = torch.from_numpy(prob.x).to(dtype).to(self.device)
        k = torch.from_numpy(prob.k.astype(np.int64)).to(self.device)
        self.xx = x[k].contiguous()  # pre-flattened gather (untimed, fp.cu:124-125)
        self.flags = head_flags_from_offsets(torch.from_numpy(prob.s), prob.n, self.device)
        self.a = torch.from_numpy(prob.a.copy()).to(dtype).to(self.device)

    def reset(self) -> None:
        self.a.copy_(torch.from_numpy(self.prob.a).to(self.dtype))

    def step(self) -> None:
        if self.algo != "lookback":
            self.run(1)
            return
        segmented_scan(self.a, self.flags, out=self.a, mul=self.xx)

    def run(self, iters: int | None = None) -> torch.Tensor:
        iters = self.prob.iters if iters is None else iters
        if self.algo == "lookback":
            return spmv_scan_run(self.a, self.xx, self.flags, iters)
        _ext.call_hip("cme_segscan_offsets_run", self.a.data_ptr(), self.xx.data_ptr(), self.offsets.data_ptr(),
                      self.prob.p - 1, 0 if self.algo == "serial" else 1, iters, _ext.stream_ptr(self.device))
        return self.a


def reference_solution(prob: SpmvScanProblem, iters: int | None = None) -> np.ndarray:
    """fp64 serial result (the instructor checker's algorithm), vectorised:
    per iteration, a segmented cumulative sum of a*x[k] in double."""
    a = prob.a.astype(np.float64)
    xx = prob.x.astype(np.float64)[prob.k]
    starts = prob.s[:-1].astype(np.int64)
    seg_id = np.repeat(np.arange(starts.size), np.diff(prob.s.astype(np.int64)))
    for _ in range(prob.iters if iters is None else iters):
        v = a * xx
        c = np.cumsum(v)
        base = np.concatenate([[0.0], c])[starts]  # cumsum just before each segment start
        a = c - base[seg_id]
    return a


def reference_solution_quadratic(prob: SpmvScanProblem, iters: int | None = None) -> np.ndarray:
    """The OLDER checker's algorithm (``aux/CheckOutput/serialMV.cu:27-37``):
    every output element re-sums its segment prefix from the segment start,
    O(len^2) per segment, in double. Same result as :func:`reference_solution`
    up to summation order; only for small inputs (the CheckOutput fixture)."""
    a = prob.a.astype(np.float64)
    xx = prob.x.astype(np.float64)[prob.k]
    s = prob.s.astype(np.int64)
    for _ in range(prob.iters if iters is None else iters):
        b = np.empty_like(a)
        for lo, hi in zip(s[:-1], s[1:]):
            for j in range(lo, hi):
                acc = 0.0
                for l in range(lo, j + 1):
                    acc += a[l] * xx[l]
                b[j] = acc
        a = b
    return a


def errors(ref: np.ndarray, b: np.ndarray) -> dict:
    """The checker's metrics (``reference_spMVscan-released.cu:64-144``)."""
    ref = ref.astype(np.float64)
    b = b.astype(np.float64)
    d = ref - b
    l2 = float(np.sqrt(np.dot(d, d)))
    na = float(np.sqrt(np.dot(ref, ref)))
    linf = float(np.abs(d).max())
    ninf = float(np.abs(ref).max())
    return {"L2": l2, "relL2": l2 / na if na > 0 else float("inf"), "Linf": linf,
            "relLinf": linf / ninf if ninf > 0 else float("inf")}


def run_fp(a_path: str, x_path: str, cpu_check: bool = False, device: str | None = None,
           out_path: str = "b.txt", algo: str = "lookback", graph: bool = False, double: bool = False) -> dict:
    """The ``./fp a.txt x.txt [check]`` driver (``fp.cu:74-216``). ``double``:
    load, iterate and write in float64 (``b.txt`` and ``b_cpu.txt`` then carry
    17 significant digits, not the reference format's 6)."""
    device = device or ("cuda" if torch.cuda.is_available() else "cpu")
    prob = load(a_path, x_path, dtype=np.float64 if double else np.float32)
    print(f"\nDim of a: {prob.n}\nDim of x: {prob.q}\nDim of s: {prob.p}\n# of iters: {prob.iters}\n")
    sol = SpmvScanSolver(prob, device, algo, dtype=torch.float64 if double else torch.float32)
    sol.run(1)  # warm-up (code object load), then restore a
    sol.reset()
    runner = None
    if graph and sol.device.type == "cuda":
        # record the N-iteration loop as one hipGraph (recording does not
        # execute it); the timed region is a single replay
        from ..utils.graphs import GraphRunner

        runner = GraphRunner(lambda: sol.run(), warmup=0)
    t = EventTimer("spmv-scan", device=device if device != "cpu" else None, print_result=False)
    with t:
        if runner is not None:
            runner()
        else:
            sol.run()
    print(f"The running time of my code for {prob.iters} iterations is: {t.ms:g} milliseconds.\n")
    b = sol.a.cpu().numpy()
    res = {"ms": t.ms, "n": prob.n, "p": prob.p, "N": prob.iters,
           "GBps": (24.0 if double else 12.0) * prob.n * prob.iters / t.ms / 1e6}  # read a, xx, write a
    digits = 17 if double else None
    if cpu_check:
        ref = reference_solution(prob)
        res.update(errors(ref, b))
        write_vector("b_cpu.txt", ref if double else ref.astype(np.float32), digits)
    write_vector(out_path, b, digits)
    return res
