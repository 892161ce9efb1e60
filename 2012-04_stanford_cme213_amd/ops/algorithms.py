"""Data-parallel algorithms: the Thrust calls of the reference, native on MI355X.

================================  ===========================================
reference (Thrust 1.x)            here
================================  ===========================================
``remove_copy_if`` / ``copy_if``  :func:`copy_if` (``invert=True`` = remove)
``remove_copy`` (value)           :func:`remove_value`
``unique`` (sorted)               :func:`unique`
``stable_partition`` / split      :func:`stable_partition`, :func:`split`
index of set flags                :func:`nonzero`
``lower_bound``/``upper_bound``   :func:`lower_bound`, :func:`upper_bound`
``reduce_by_key`` (sorted keys)   :func:`reduce_by_key`
dense / sparse histogram          :func:`histogram_dense`, :func:`histogram_sparse`
histogram by atomics (Lecture21)  :func:`bincount` (unsorted uint8 / int32 / int64)
counting sort (Lecture16)         :func:`counting_sort`
``max_element``/``min_element``   :func:`max_element`, :func:`min_element`
``inner_product``                 :func:`inner_product` (``op="mul"|"eq"``)
================================  ===========================================

Call sites in the reference: ``hw/hw3/programming/create_cipher.cu:111-113``
(remove_copy_if), ``hw/hw3/programming/solve_cipher.cu:136-154`` (sort +
upper_bound dense histogram), ``hw/hw3/solution/solve_cipher_solution.cu:
131-200`` (reduce_by_key, sort_by_key, max_element, inner_product); the scan
applications are ``slides/Lecture16.pdf`` 2-19.

GPU tensors run ``csrc/hip/algorithms.hip`` (deterministic reduce-then-scan
compaction, stable); CPU tensors the OpenMP backend
``csrc/cpu/algorithms_cpu.cpp`` (count -> scan -> write, stable). The
``ref_*`` functions are plain-PyTorch oracles, used only by the tests.
"""
from __future__ import annotations

import ctypes
import math

import torch

from .. import _ext
from .sort import sort as _sort

_ext.proto(_ext.HIP_PROTOS, "cme_select", "ppqiiQiipppp")
_ext.proto(_ext.HIP_PROTOS, "cme_search", "pqpqiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_seg_reduce", "ppqiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_arg_reduce", "pqiipppp")
_ext.proto(_ext.HIP_PROTOS, "cme_inner_product", "ppqippp")

_ext.proto(_ext.CPU_PROTOS, "cme_cpu_select", "ppqiiQiipp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_search", "pqpqiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_seg_reduce", "ppqiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_arg_reduce", "pqiipp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_inner_product", "ppqip")
_ext.proto(_ext.HIP_PROTOS, "cme_bincount", "pqiqpp")
_ext.proto(_ext.HIP_PROTOS, "cme_bincount_plan", "qiqp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_bincount", "pqiqp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_bincount_path", "pqiqpi")

_SEARCH_DT = {torch.float32: 0, torch.int32: 1, torch.uint32: 2, torch.int64: 3, torch.float64: 4}
_RED_DT = {torch.float32: 0, torch.int32: 1, torch.int64: 3, torch.float64: 4}
_OPS = {"sum": 0, "max": 1, "min": 2}
_PRED = {"flags": 0, "neq": 1, "head": 2}
_TILE = 4096  # kTile in algorithms.hip


# GPU select algorithm for values / indices: "rts" (reduce-then-scan, two
# reads of the input; default, faster at 2^26) or "lookback" (one pass with a
# two-level decoupled look-back; csrc/hip/algorithms.hip select_lookback_kernel)
SELECT_ALGO = "rts"


def _select_ws_bytes(n: int) -> int:  # = cme_select_ws_bytes
    t = (n + _TILE - 1) // _TILE
    return 16 * t + 16 * ((t + 63) // 64) + 4096 + 64


_ws: dict = {}


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    t = _ws.get(dev.index)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=dev)
        _ws[dev.index] = t
    return t


def _dtype_code(table: dict, t: torch.Tensor, what: str) -> int:
    if t.dtype not in table:
        names = ", ".join(str(d).split(".")[-1] for d in table)
        raise TypeError(f"{what}: unsupported dtype {t.dtype} (takes {names})")
    return table[t.dtype]


def _flag_bytes(flags: torch.Tensor) -> torch.Tensor:
    """uint8 flags for the kernels, which test every byte against zero: bool
    and uint8 as they are, every other dtype as ``flags != 0`` (256 and 0.5
    are set flags; a cast to uint8 would clear them)."""
    if flags.dtype == torch.uint8:
        return flags
    return (flags if flags.dtype == torch.bool else flags != 0).view(torch.uint8)


def _esize(x: torch.Tensor) -> int:
    e = x.element_size()
    if e not in (1, 4, 8):
        raise TypeError(f"unsupported element size {e} ({x.dtype})")
    return e


def _bits(x: torch.Tensor, value) -> int:
    """Raw bit pattern of a scalar in x's dtype (predicates compare bitwise)."""
    t = torch.tensor([value], dtype=x.dtype)
    u = {1: torch.uint8, 4: torch.int32, 8: torch.int64}[x.element_size()]
    v = int(t.view(u).item())
    return v & ((1 << (8 * x.element_size())) - 1)


def _select(x: torch.Tensor, flags: torch.Tensor | None, pred: str, value=0, invert: bool = False,
            mode: int = 0) -> tuple[torch.Tensor, int]:
    x = x.contiguous().view(-1)
    n = x.numel()
    if flags is not None:
        flags = flags.contiguous().view(-1)
        if flags.numel() != n:
            raise ValueError("flags must match x")
        flags = _flag_bytes(flags)
    out = torch.empty(n, dtype=torch.int64 if mode == 1 else x.dtype, device=x.device)
    if not x.is_cuda:
        cnt = ctypes.c_longlong(0)
        _ext.call_cpu("cme_cpu_select", x.data_ptr(), flags.data_ptr() if flags is not None else None, n, _esize(x),
                      _PRED[pred], _bits(x, value) if pred == "neq" else 0, int(invert), mode, out.data_ptr(),
                      ctypes.addressof(cnt))
        return out, cnt.value
    from .scan import _check_lookback

    lookback = SELECT_ALGO == "lookback" and mode != 2
    cnt = torch.zeros(1, dtype=torch.int64, device=x.device)
    ws = _workspace(x.device, _select_ws_bytes(n))
    if lookback:
        _check_lookback(x, before=True)
    _ext.call_hip("cme_select", x.data_ptr(), flags.data_ptr() if flags is not None else None, n, _esize(x),
                  _PRED[pred], _bits(x, value) if pred == "neq" else 0, int(invert), mode | (8 if lookback else 0),
                  out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), _ext.stream_ptr(x.device))
    if lookback:
        _check_lookback(x)
    return out, int(cnt.item())


def copy_if(x: torch.Tensor, flags: torch.Tensor, invert: bool = False) -> torch.Tensor:
    """Stable stream compaction: elements whose flag is set (``invert``: not
    set -- ``remove_copy_if``). A flag of any dtype is set iff it is ``!= 0``."""
    out, c = _select(x, flags, "flags", invert=invert)
    return out[:c]


def remove_value(x: torch.Tensor, value) -> torch.Tensor:
    """``thrust::remove_copy``: every element not equal (bitwise) to value."""
    out, c = _select(x, None, "neq", value)
    return out[:c]


def unique(x: torch.Tensor) -> torch.Tensor:
    """First element of every run of bitwise equal values (``thrust::unique``
    on sorted input = dedup via head flags, Lecture16): -0.0 and 0.0 are two
    values, two NaNs are equal iff their bits are."""
    out, c = _select(x, None, "head")
    return out[:c]


def run_starts(x: torch.Tensor) -> torch.Tensor:
    """int64 indices where a new run of bitwise equal values begins."""
    out, c = _select(x, None, "head", mode=1)
    return out[:c]


def nonzero(flags: torch.Tensor) -> torch.Tensor:
    """int64 indices of the set flags (stable); a flag of any dtype is set iff
    it is ``!= 0``."""
    fb = _flag_bytes(flags.contiguous().view(-1))
    out, c = _select(fb, fb, "flags", mode=1)
    return out[:c]


def stable_partition(x: torch.Tensor, flags: torch.Tensor) -> tuple[torch.Tensor, int]:
    """Selected elements first, then the rest, both in input order; returns
    (permuted, number selected)."""
    return _select(x, flags, "flags", mode=2)


def split(x: torch.Tensor, flags: torch.Tensor) -> tuple[torch.Tensor, int]:
    """Lecture16 ``split``: flag-0 elements first, then flag-1 (the radix
    sort step); returns (permuted, number of zeros)."""
    return _select(x, flags, "flags", invert=True, mode=2)


def _search(sorted_: torch.Tensor, q: torch.Tensor, upper: bool) -> torch.Tensor:
    if sorted_.dtype != q.dtype:
        raise TypeError(f"sorted and queries must share a dtype ({sorted_.dtype} and {q.dtype})")
    dt = _dtype_code(_SEARCH_DT, sorted_, "search")
    s, qq = sorted_.contiguous().view(-1), q.contiguous().view(-1)
    out = torch.empty(qq.numel(), dtype=torch.int64, device=q.device)
    if not sorted_.is_cuda:
        _ext.call_cpu("cme_cpu_search", s.data_ptr(), s.numel(), qq.data_ptr(), qq.numel(), dt, int(upper),
                      out.data_ptr())
        return out
    _ext.call_hip("cme_search", s.data_ptr(), s.numel(), qq.data_ptr(), qq.numel(), dt, int(upper), out.data_ptr(),
                  _ext.stream_ptr(q.device))
    return out


def lower_bound(sorted_: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """First index i with sorted[i] >= q, per query (vectorised). The order is
    numeric (-0.0 == 0.0); NaN keys or queries are unsupported."""
    return _search(sorted_, q, False)


def upper_bound(sorted_: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """First index i with sorted[i] > q, per query (vectorised). The order is
    numeric (-0.0 == 0.0); NaN keys or queries are unsupported."""
    return _search(sorted_, q, True)


def segment_reduce(vals: torch.Tensor, offsets: torch.Tensor, op: str = "sum") -> torch.Tensor:
    """out[s] = op(vals[offsets[s]:offsets[s+1]]); offsets int64 (nseg + 1).
    Empty segments give the op's identity (0; -inf / +inf; the integer's
    lowest / largest). vals: float32, int32, int64 or float64."""
    nseg = offsets.numel() - 1
    dt = _dtype_code(_RED_DT, vals, "segment_reduce")
    if not vals.is_cuda:
        v = vals.contiguous().view(-1)
        off = offsets.to(torch.int64).contiguous()
        out = torch.empty(nseg, dtype=v.dtype)
        _ext.call_cpu("cme_cpu_seg_reduce", v.data_ptr(), off.data_ptr(), nseg, dt, _OPS[op], out.data_ptr())
        return out
    v = vals.contiguous().view(-1)
    off = offsets.to(torch.int64).contiguous()
    out = torch.empty(nseg, dtype=v.dtype, device=v.device)
    _ext.call_hip("cme_seg_reduce", v.data_ptr(), off.data_ptr(), nseg, dt, _OPS[op], out.data_ptr(),
                  _ext.stream_ptr(v.device))
    return out


def reduce_by_key(keys: torch.Tensor, vals: torch.Tensor, op: str = "sum") -> tuple[torch.Tensor, torch.Tensor]:
    """Runs of equal consecutive keys -> (unique keys, reduced values)."""
    starts = run_starts(keys)
    offsets = torch.cat([starts, torch.tensor([keys.numel()], dtype=torch.int64, device=starts.device)])
    return keys.reshape(-1)[starts], segment_reduce(vals, offsets, op)


def histogram_dense(sorted_: torch.Tensor, nbins: int) -> torch.Tensor:
    """Counts of values 0..nbins-1 in SORTED integer data, the Thrust idiom
    ``upper_bound(sorted, counting_iterator)`` + ``adjacent_difference``
    (``hw/hw3/programming/solve_cipher.cu:136-154``)."""
    q = torch.arange(nbins, dtype=sorted_.dtype, device=sorted_.device)
    ub = upper_bound(sorted_, q)
    return torch.diff(ub, prepend=torch.zeros(1, dtype=ub.dtype, device=ub.device))


def histogram_sparse(sorted_: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(distinct values, counts) of sorted data: ``reduce_by_key`` with a
    constant-1 value stream (``solve_cipher_solution.cu:185-200``)."""
    ones = torch.ones(sorted_.numel(), dtype=torch.int32, device=sorted_.device)
    return reduce_by_key(sorted_, ones, "sum")


_BINCOUNT_DT = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}  # dtype -> the native element size
_BINCOUNT_REGIMES = {1: "lds", 2: "window", 3: "global", 4: "sorted"}
# CPU backend: 0 the rule, 1 serial, 2 per-thread tables, 3 bins partitioned over the threads (tests force each)
BINCOUNT_CPU_PATH = 0


def _bincount_plan(n: int, esize: int, nbins: int) -> list[int]:
    """cme_bincount_plan under the current knobs; ``ValueError`` where the
    regime forced by ``bincount_regime`` cannot run the shape."""
    info = (ctypes.c_longlong * 11)()
    if _ext._fn("hip", "cme_bincount_plan")(n, esize, nbins, ctypes.addressof(info)) != 0:
        from ..utils import tuning

        raise ValueError(f"bincount: the forced regime (bincount_regime={tuning.get('bincount_regime')}) cannot run "
                         f"n={n}, nbins={nbins}, {esize}-byte elements")
    return [int(v) for v in info]


def _bincount_sorted(x: torch.Tensor, nbins: int, out: torch.Tensor) -> torch.Tensor:
    """The ``sorted`` regime: the dense histogram of the sorted copy. Unlike
    :func:`histogram_dense`, bin 0 starts at the first element >= 0, so
    negative elements are not counted."""
    s = _sort(x)
    q = torch.arange(nbins, dtype=x.dtype, device=x.device)
    ub = upper_bound(s, q)
    first = lower_bound(s, torch.zeros(1, dtype=x.dtype, device=x.device))
    torch.sub(ub, torch.cat([first, ub[:-1]]), out=out)
    return out


def _bincount_fixed(x: torch.Tensor, nbins: int, out: torch.Tensor | None) -> torch.Tensor:
    esize = _BINCOUNT_DT[x.dtype]
    if out is None:
        out = torch.empty(nbins, dtype=torch.int64, device=x.device)
    if nbins == 0:
        return out
    if not x.is_cuda:
        if BINCOUNT_CPU_PATH:
            _ext.call_cpu("cme_cpu_bincount_path", x.data_ptr(), x.numel(), esize, nbins, out.data_ptr(),
                          BINCOUNT_CPU_PATH)
        else:
            _ext.call_cpu("cme_cpu_bincount", x.data_ptr(), x.numel(), esize, nbins, out.data_ptr())
        return out
    with torch.cuda.device(x.device):
        if _bincount_plan(x.numel(), esize, nbins)[0] == 4:
            return _bincount_sorted(x, nbins, out) if x.numel() else out.zero_()
        _ext.call_hip("cme_bincount", x.data_ptr(), x.numel(), esize, nbins, out.data_ptr(), _ext.stream_ptr(x.device))
    return out


def bincount(x: torch.Tensor, minlength: int = 0, nbins: int | None = None,
             out: torch.Tensor | None = None) -> torch.Tensor:
    """Counts of the values ``0, 1, 2, ...`` in UNSORTED integer data (int64).

    ``x``: a 1-D ``uint8``, ``int32`` or ``int64`` tensor on the CPU or the
    GPU, any contiguous view at element alignment (``x[1:]`` runs without a
    padded copy); a non-contiguous view is made contiguous first. Other dtypes
    raise ``TypeError``, other ranks ``ValueError``.

    ``nbins=None``: ``torch.bincount(x, minlength=minlength)`` exactly -- the
    result has ``max(max(x) + 1, minlength)`` entries, a negative element
    raises ``ValueError``, an empty ``x`` gives ``zeros(minlength)``. The
    length is data dependent, so this form reads the extremes back to the host
    once (``scan.reduce`` "min" / "max"; uint8 counts into 256 bins and trims).

    ``nbins=K``: exactly ``K`` entries. An element outside ``[0, K)`` is not
    counted and raises nothing; the comparison is made in the element's own
    width (an int64 ``2**32 + 3`` is out of range for ``K = 8``). No host
    synchronisation, no data-dependent shape. ``minlength`` must stay 0.
    ``out``: a contiguous int64 tensor of ``K`` entries on ``x``'s device,
    overwritten (not accumulated into) and returned; this form only.

    GPU: ``csrc/hip/bincount.hip`` -- per-workgroup LDS tables (``lds``), the
    same over bin windows (``window``), one global atomic per element
    (``global``), or the histogram of the sorted copy (``sorted``);
    :func:`bincount_launch_info` reports which. Integer counts are exact
    whatever the order of the atomics, so every run gives the same bits. CPU:
    ``cme_cpu_bincount`` (OpenMP).

    There is no ``weights=``: float atomics are not reproducible, and the
    deterministic weighted form exists as ``sort`` + :func:`reduce_by_key`.
    Float binning (``histc``) and counting along a dimension are out of scope
    too."""
    if not isinstance(x, torch.Tensor):
        raise TypeError("bincount: x must be a tensor")
    _dtype_code(_BINCOUNT_DT, x, "bincount")
    if x.dim() != 1:
        raise ValueError(f"bincount: x must be 1-D, got {x.dim()} dimensions")
    if isinstance(minlength, bool) or not isinstance(minlength, int) or minlength < 0:
        raise ValueError(f"bincount: minlength must be a non-negative integer, got {minlength!r}")
    x = x.contiguous()
    if nbins is not None:
        if isinstance(nbins, bool) or not isinstance(nbins, int) or nbins < 0:
            raise ValueError(f"bincount: nbins must be a non-negative integer, got {nbins!r}")
        if minlength != 0:
            raise ValueError("bincount: minlength goes with nbins=None; with nbins given the length is nbins")
        if out is not None:
            if not isinstance(out, torch.Tensor) or out.dtype != torch.int64:
                raise TypeError("bincount: out must be an int64 tensor")
            if out.dim() != 1 or out.numel() != nbins:
                raise ValueError(f"bincount: out must have shape ({nbins},), got {tuple(out.shape)}")
            if not out.is_contiguous():
                raise ValueError("bincount: out must be contiguous")
            if out.device != x.device:
                raise ValueError(f"bincount: out is on {out.device}, x on {x.device}")
        return _bincount_fixed(x, nbins, out)
    if out is not None:
        raise ValueError("bincount: out= needs nbins (the data-dependent form allocates its result)")
    if x.numel() == 0:
        return torch.zeros(minlength, dtype=torch.int64, device=x.device)
    if x.dtype == torch.uint8:
        c = _bincount_fixed(x, 256, None)
        k = max(int(torch.nonzero(c)[-1]) + 1, minlength)  # the one host read
        return c[:k].clone() if k <= 256 else torch.cat([c, c.new_zeros(k - 256)])
    from .scan import reduce as _reduce

    lo, hi = torch.stack([_reduce(x, "min"), _reduce(x, "max")]).tolist()  # the one host read
    if lo < 0:
        raise ValueError("bincount: x has a negative element (give nbins to leave out-of-range elements uncounted)")
    return _bincount_fixed(x, max(hi + 1, minlength), None)


def bincount_launch_info(n: int, nbins: int, dtype: torch.dtype = torch.int64,
                         device: torch.device | str = "cuda") -> dict:
    """How ``bincount(x, nbins=nbins)`` of ``n`` elements runs on ``device``
    under the current knobs: ``regime`` ("lds", "window", "global", "sorted";
    "cpu" on the CPU), ``window`` (``W``, the bins of one LDS table),
    ``windows``, ``copies`` (replicas of a workgroup's table), ``workgroups``
    (= ``windows * chunks``), ``chunks`` (workgroups per window), ``threads``,
    ``vector`` (elements of one 16-byte lane vector), ``pass`` (elements one
    workgroup takes per grid stride), ``lds_bytes`` and ``ws_bytes``. A regime
    forced where it cannot run raises ``ValueError``. The CPU backend has no
    plan: it reports ``vector`` and zeros."""
    if dtype not in _BINCOUNT_DT:
        names = ", ".join(str(d).split(".")[-1] for d in _BINCOUNT_DT)
        raise TypeError(f"bincount: unsupported dtype {dtype} (takes {names})")
    esize = _BINCOUNT_DT[dtype]
    d = {"regime": "cpu", "window": 0, "windows": 0, "copies": 0, "workgroups": 0, "chunks": 0, "threads": 0,
         "vector": 16 // esize, "pass": 0, "lds_bytes": 0, "ws_bytes": 0}
    if torch.device(device).type != "cuda":
        return d
    i = _bincount_plan(int(n), esize, int(nbins))
    d.update(regime=_BINCOUNT_REGIMES[i[0]], window=i[1], windows=i[2], copies=i[3], workgroups=i[4], lds_bytes=i[5],
             ws_bytes=i[6], threads=i[7], vector=i[8], chunks=i[10])
    d["pass"] = i[9]
    return d


def counting_sort(keys: torch.Tensor, num_keys: int, values: torch.Tensor | None = None):
    """Stable sort of int32 keys in [0, num_keys): a radix sort restricted to
    ceil(log2(num_keys)) bits (one 8-bit counting pass when num_keys <= 256).
    CPU tensors use a stable torch sort."""
    bits = max(1, math.ceil(math.log2(max(num_keys, 2))))
    kdt = keys.dtype
    if kdt == torch.int64:  # keys < num_keys <= 2^31: sorted as int32
        keys = keys.to(torch.int32)
    if not keys.is_cuda and values is None:  # keys only: carry a dummy payload through the key-value pass
        k = _sort(keys, torch.zeros_like(keys), "radix", key_bits=bits)[0]
        return k.to(kdt)
    res = _sort(keys, values, "radix", key_bits=bits)
    if isinstance(res, tuple):
        return res[0].to(kdt), res[1]
    return res.to(kdt)


def _arg(x: torch.Tensor, is_max: bool) -> tuple[float, int]:
    if x.numel() == 0:
        raise ValueError("empty input")
    dt = _dtype_code(_RED_DT, x, "max_element / min_element")
    xs = x.reshape(-1).contiguous()
    if not x.is_cuda:  # first index on ties, like thrust::max_element
        val = torch.empty(1, dtype=xs.dtype)
        idx = ctypes.c_longlong(0)
        _ext.call_cpu("cme_cpu_arg_reduce", xs.data_ptr(), xs.numel(), dt, int(is_max), val.data_ptr(),
                      ctypes.addressof(idx))
        return val.item(), idx.value
    ov = torch.empty(1, dtype=xs.dtype, device=xs.device)
    oi = torch.empty(1, dtype=torch.int64, device=xs.device)
    ws = _workspace(xs.device, 16 * 2048)
    _ext.call_hip("cme_arg_reduce", xs.data_ptr(), xs.numel(), dt, int(is_max), ws.data_ptr(), ov.data_ptr(),
                  oi.data_ptr(), _ext.stream_ptr(xs.device))
    return ov.item(), int(oi.item())


def max_element(x: torch.Tensor) -> tuple[float, int]:
    """(max value, first index of it) of float32 / int32 / int64 / float64
    data. NaN never wins: NaNs are skipped, the result is the first index of
    the maximum of the other elements (-0.0 == 0.0: the first of them); an
    all-NaN input gives ``(nan, 0)``."""
    return _arg(x, True)


def min_element(x: torch.Tensor) -> tuple[float, int]:
    """(min value, first index of it); NaNs are skipped as in
    :func:`max_element`, an all-NaN input gives ``(nan, 0)``."""
    return _arg(x, False)


def inner_product(a: torch.Tensor, b: torch.Tensor, op: str = "mul") -> float:
    """``op="mul"``: sum(a*b) of fp32 data with fp64 accumulation;
    ``op="eq"``: number of positions where the 32-bit words are equal (the
    ``inner_product(.., plus, equal_to)`` of the index of coincidence)."""
    if a.shape != b.shape:
        raise ValueError("shape mismatch")
    if a.element_size() != 4:
        raise TypeError(f"inner_product: 32-bit elements expected, got {a.dtype}")
    if op == "mul" and a.dtype != torch.float32:
        raise TypeError(f"inner_product: op='mul' takes float32, got {a.dtype}")
    aa, bb = a.contiguous().view(-1), b.contiguous().view(-1)
    if not a.is_cuda:
        out = ctypes.c_double(0.0)
        _ext.call_cpu("cme_cpu_inner_product", aa.data_ptr(), bb.data_ptr(), aa.numel(), 0 if op == "mul" else 1,
                      ctypes.addressof(out))
        return out.value
    part = _workspace(a.device, 8 * 2048)
    out = torch.empty(1, dtype=torch.float64, device=a.device)
    _ext.call_hip("cme_inner_product", aa.data_ptr(), bb.data_ptr(), aa.numel(), 0 if op == "mul" else 1,
                  part.data_ptr(), out.data_ptr(), _ext.stream_ptr(a.device))
    return float(out.item())


# ------------------------------------------------------------------ oracles
# Numeric semantics (torch's ==): ref_unique / ref_run_starts / ref_remove_value
# merge -0.0 with 0.0 and keep every NaN apart, where the backends compare bit
# patterns; ref_arg does not skip NaN. tests/test_algorithms_edges.py has the
# bit-pattern oracles.
def _ref_mask(x: torch.Tensor, flags, pred: str, value, invert: bool) -> torch.Tensor:
    x = x.reshape(-1)
    if pred == "flags":
        m = flags.reshape(-1) != 0
    elif pred == "neq":
        m = x != value
    else:
        m = torch.ones_like(x, dtype=torch.bool)
        if x.numel() > 1:
            m[1:] = x[1:] != x[:-1]
    return ~m if invert else m


def ref_copy_if(x, flags, invert=False):
    return x.reshape(-1)[_ref_mask(x, flags, "flags", 0, invert)]


def ref_remove_value(x, value):
    return x.reshape(-1)[_ref_mask(x, None, "neq", value, False)]


def ref_unique(x):
    return x.reshape(-1)[_ref_mask(x, None, "head", 0, False)]


def ref_run_starts(x):
    return torch.nonzero(_ref_mask(x, None, "head", 0, False)).view(-1)


def ref_nonzero(flags):
    return torch.nonzero(flags.reshape(-1) != 0).view(-1)


def ref_stable_partition(x, flags):
    m = _ref_mask(x, flags, "flags", 0, False)
    xs = x.reshape(-1)
    return torch.cat([xs[m], xs[~m]]), int(m.sum())


def ref_split(x, flags):
    m = _ref_mask(x, flags, "flags", 0, True)
    xs = x.reshape(-1)
    return torch.cat([xs[m], xs[~m]]), int(m.sum())


def ref_search(sorted_, q, upper):
    if sorted_.dtype == torch.uint32:  # no uint32 searchsorted in torch: widen (order-preserving)
        sorted_, q = sorted_.to(torch.int64), q.to(torch.int64)
    return torch.searchsorted(sorted_.reshape(-1), q.reshape(-1), right=upper)


def ref_segment_reduce(vals, offsets, op="sum"):
    nseg = offsets.numel() - 1
    out = torch.empty(nseg, dtype=vals.dtype)
    lens = (offsets[1:] - offsets[:-1]).tolist()
    for i, part in enumerate(torch.split(vals.reshape(-1)[int(offsets[0]):int(offsets[-1])], lens)):
        if part.numel() == 0:
            out[i] = {"sum": 0, "max": -math.inf if vals.is_floating_point() else torch.iinfo(vals.dtype).min,
                      "min": math.inf if vals.is_floating_point() else torch.iinfo(vals.dtype).max}[op]
        else:
            out[i] = {"sum": part.sum, "max": part.max, "min": part.min}[op]()
    return out


def ref_arg(x, is_max):
    xs = x.reshape(-1)
    v = xs.max() if is_max else xs.min()
    return v.item(), int(torch.nonzero(xs == v)[0])


def ref_inner_product(a, b, op="mul"):
    if op == "mul":
        return float((a.double() * b.double()).sum())
    return float((a == b).sum())
