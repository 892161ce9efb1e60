"""Scan / reduction / segmented-scan ops.

* :func:`scan` -- single-pass decoupled look-back (default) or the lecture's
  multi-level scan-then-add with a Blelloch or Hillis-Steele block algorithm
  (``slides/Lecture16.pdf``; ``my-refs/scan.pdf`` Fig. 5).
* :func:`cummax` / :func:`cummin` (``scan(..., op="max" / "min")``) -- the
  running maximum / minimum, ``torch.cummax`` / ``torch.cummin`` values bit for
  bit, with ``algo="lookback"`` or ``"rts"``.
* ``scan`` / ``cummax`` / ``cummin`` with ``dim=d`` -- the same along one
  dimension of a tensor of any rank (``csrc/hip/scan_dim.hip``; no look-back,
  chunked reduce-then-scan where the lines are few), :func:`summed_area_table`
  on top of it, :func:`scan_dim_launch_info`.
* ``cummax`` / ``cummin`` with ``return_indices=True`` -- ``(values, indices)``
  as ``torch.cummax`` / ``torch.cummin`` return them, along any dimension or
  over the flattened tensor (``csrc/hip/scan_dim_arg.hip``: the same batched
  kernels with a (value, index) carry).
* :func:`reduce` -- sum / max / min; the lecture's shared-memory tree
  (``slides/Lecture05.pdf`` 15-16) as ``algo="tree"``. With ``dim=`` /
  ``keepdim`` / ``return_indices`` it reduces along one dimension of a tensor
  of any rank, every scan dtype (``csrc/hip/reduce_dim.hip``), as do
  :func:`argmax` / :func:`argmin`; :func:`reduce_dim_launch_info`.
* Both take float32 / int32 and int64 / float64 (``scan`` also uint32); the
  64-bit kernels are ``csrc/hip/scan64.hip`` (``algo="rts"`` / ``"lookback"``
  only; everything else here is 32-bit).
* :func:`segmented_scan` -- inclusive, head-flag segmented scan (Lecture21;
  nvr-2008-003), optionally fused with an element-wise multiply: the final
  project's ``a *= x[k]; b = segscan(a)`` step (``hw/hw_final/programming/
  fp.cu:168-185``) in one pass. float32, and int64 / float64
  (``csrc/hip/segscan64.hip``).

CPU tensors use the OpenMP oracles in ``csrc/cpu/scan_cpu.cpp``.
"""
from __future__ import annotations

import collections

import torch

from .. import _ext

_ext.proto(_ext.HIP_PROTOS, "cme_scan", "ppqiipup")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_rts", "ppqiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_mlevel", "ppqiiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_tree", "ppqiiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_reduce", "pqiiippp")
_ext.proto(_ext.HIP_PROTOS, "cme_segscan", "ppppiqpup")
_ext.proto(_ext.HIP_PROTOS, "cme_spmv_scan_run", "pppqipp")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_op", "ppqiiipup")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_rts_op", "ppqiiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_op_info", "qiiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_scan", "ppqii")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_scan_op", "ppqiii")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_reduce", "pqiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_segscan", "ppppiq")

# native dtype codes; 3 / 4 are the 64-bit kernels (csrc/hip/scan64.hip), the
# codes algorithms.py uses for int64 / float64 as well
_DT = {torch.float32: 0, torch.int32: 1}
_DT_SCAN = {torch.float32: 0, torch.int32: 1, torch.uint32: 2}
_DT64 = {torch.int64: 3, torch.float64: 4}
_OPS = {"sum": 0, "max": 1, "min": 2}
TILE = 4096
TILE64 = 8192  # elements per tile of the 64-bit look-back scan (scan64.h kScan64Tile; "rts" tiles are half)
_ALGOS64 = ("rts", "lookback")
_VECTOR_ALGOS = ("lookback", "rts", "blelloch", "hillis")  # 32-bit: 16-byte loads and stores (the *_mlevel are scalar)
# "auto" for int64: the look-back measured faster than reduce-then-scan at
# both 2^25 and 2^27 elements (benchmarks/bench_primitives.py --only scan64,
# profiles/scan64_r8.md)
_AUTO_INT64 = "lookback"
# max / min scans: "rts" and "lookback" only, every dtype. Their operator is
# exactly associative on floats too, so the single-pass look-back is bitwise
# reproducible and "auto" is "lookback" for every dtype. Measured
# (benchmarks/bench_primitives.py --only scan_minmax, profiles/scan_minmax.md):
# the look-back is the faster arm at 2^25 and 2^27 for int32, int64 and float64
# and at 2^27 for float32; float32 at 2^25 has "rts" ahead (0.081 against 0.091
# ms) inside the spread of both arms, which does not earn a size switch.
_ALGOS_MINMAX = ("rts", "lookback")
_AUTO_MINMAX = {torch.float32: "lookback", torch.int32: "lookback", torch.uint32: "lookback",
                torch.int64: "lookback", torch.float64: "lookback"}

_ws_cache: dict = {}


def workspace(device: torch.device, nbytes: int, key: str = "lookback") -> torch.Tensor:
    """Per-device scratch, grown on demand (never allocated inside a launch)."""
    k = (key, device.index)
    t = _ws_cache.get(k)
    if t is None or t.numel() < nbytes:
        t = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
        _ws_cache[k] = t
    return t


_epochs: dict = {}
_EPOCH_LIMIT = 1 << 24  # lookback.h: status word = (epoch << 8) | bits, 32 bits


def _lookback_ws(x: torch.Tensor) -> tuple[torch.Tensor, int]:
    """Descriptor array of a look-back launch and the epoch to run it with.
    Keyed by (device, STREAM): two scans enqueued on different streams must
    not overwrite each other's descriptors. The array is zeroed once when it
    is (re)allocated; every launch then gets the next epoch, so stale
    descriptors of earlier launches never match and no per-launch memset is
    needed. Under stream capture the epoch is 0 (the native side zeroes the
    array inside the graph), because a replayed graph repeats its arguments."""
    tiles = (x.numel() + TILE - 1) // TILE  # >= the launch's tile count (its tiles are >= TILE elements)
    nbytes = 16 * tiles + 16 * (tiles // 64 + 1) + 64  # lookback.h lb2_ws_bytes (>= the one-level layout)
    k = (f"lookback:{_ext.stream_ptr(x.device)}", x.device.index)
    t = _ws_cache.get(k)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=x.device)
        _ws_cache[k] = t
        _epochs[k] = 0
    if torch.cuda.is_current_stream_capturing():
        # the graph zeroes the array at replay and writes epoch-0 words, which
        # later epochs (>= 1) ignore; the count is NOT restarted: before a
        # replay, words of the earlier epochs are still there
        return t, 0
    e = _epochs[k] + 1
    if e >= _EPOCH_LIMIT:
        t.zero_()
        e = 1
    _epochs[k] = e
    return t, e


def _aligned(t: torch.Tensor, nbytes: int = 16) -> torch.Tensor:
    """``t`` itself if its data is ``nbytes``-aligned, else a copy that is (a
    fresh allocation). The 32-bit GPU kernels load and store whole 16-byte
    vectors (and four uint8 flags per 4-byte load) without a scalar path, so a
    view such as ``x[1:]`` is staged through an aligned temporary; aligned
    operands are passed as they are."""
    return t if t.data_ptr() % nbytes == 0 else t.clone()


_ext.proto(_ext.HIP_PROTOS, "cme_scan32_info", "qiiip")
_SCAN32_KINDS = {"lookback": 0, "segscan": 1}


_OP_INFO_KEYS = ("tile", "tiles", "workgroups", "blocks_per_cu", "rts_chunks", "rts_tiles_per_chunk", "rts_tile",
                 "lookback_ws_bytes")


def _scan_op_info(n: int, dtype: torch.dtype, op: str, exclusive: bool, device) -> dict:
    """``cme_scan_op_info``: the launch shape of the kernels of (dtype, op,
    exclusive) -- the max / min kernels are instantiations of their own."""
    import ctypes

    if op not in _OPS:
        raise ValueError(f"scan: op {op!r} is not one of {sorted(_OPS)}")
    info = (ctypes.c_longlong * 8)()
    code = _DT64[dtype] if dtype in _DT64 else _DT_SCAN[dtype]
    with torch.cuda.device(torch.device(device)):
        _ext.call_hip("cme_scan_op_info", n, code, _OPS[op], int(exclusive), ctypes.addressof(info))
    return dict(zip(_OP_INFO_KEYS, (int(v) for v in info)))


def scan_launch_info(n: int, kind: str = "lookback", exclusive: bool = False, device: torch.device | str = "cuda",
                     dtype: torch.dtype = torch.float32, op: str = "sum") -> dict:
    """How a 32-bit look-back launch of ``n`` elements is shaped on ``device``:
    ``tile`` (elements), ``tiles``, ``workgroups`` (the persistent, co-resident
    grid) and ``blocks_per_cu``. ``kind``: "lookback" (:func:`scan` with
    ``algo="lookback"``; ``exclusive``, ``dtype`` and ``op`` pick the kernel) or
    "segscan" (the float32 :func:`segmented_scan`). With ``op="max"`` /
    ``"min"`` the dict also has ``rts_chunks``, ``rts_tiles_per_chunk`` and
    ``rts_tile`` of ``algo="rts"``, and ``lookback_ws_bytes``."""
    import ctypes

    if kind not in _SCAN32_KINDS:
        raise ValueError(f"scan_launch_info: kind {kind!r} is not one of {sorted(_SCAN32_KINDS)}")
    if op != "sum":
        if kind != "lookback":
            raise ValueError("scan_launch_info: only the plain scans take an op")
        return _scan_op_info(n, dtype, op, exclusive, device)
    info = (ctypes.c_longlong * 4)()
    with torch.cuda.device(torch.device(device)):
        _ext.call_hip("cme_scan32_info", n, _SCAN32_KINDS[kind], _DT_SCAN[dtype], int(exclusive),
                      ctypes.addressof(info))
    return dict(zip(("tile", "tiles", "workgroups", "blocks_per_cu"), (int(v) for v in info)))


_ext.proto(_ext.HIP_PROTOS, "cme_scan64_info", "qp")


def scan64_launch_info(n: int, device: torch.device | str = "cuda", op: str = "sum",
                       dtype: torch.dtype = torch.int64, exclusive: bool = False) -> dict:
    """How the 64-bit scans of ``n`` elements are launched on ``device``:
    ``tile`` (elements), ``tiles``, ``lookback_workgroups`` (the persistent,
    co-resident grid of ``algo="lookback"``), ``rts_chunks`` and
    ``rts_tiles_per_chunk`` (``algo="rts"``, whose tiles are ``rts_tile``
    elements), ``lookback_ws_bytes``. ``op="max"`` / ``"min"``: the same keys
    (and ``blocks_per_cu``) for the max / min kernels of ``dtype`` and
    ``exclusive``."""
    import ctypes

    if op != "sum":
        d = _scan_op_info(n, dtype, op, exclusive, device)
        d["lookback_workgroups"] = d.pop("workgroups")
        return d
    info = (ctypes.c_longlong * 7)()
    with torch.cuda.device(torch.device(device)):
        _ext.call_hip("cme_scan64_info", n, ctypes.addressof(info))
    keys = ("tile", "tiles", "lookback_workgroups", "rts_chunks", "rts_tiles_per_chunk", "lookback_ws_bytes", "rts_tile")
    return dict(zip(keys, (int(v) for v in info)))


def _lookback64_ws(x: torch.Tensor, tile: int = TILE64, family: str = "lookback64") -> tuple[torch.Tensor, int]:
    """Descriptor array and epoch of a 64-bit look-back launch. As
    :func:`_lookback_ws`, but an array and an epoch count of their own per
    (device, stream): a slot is two 8-byte granules there (twice the bytes),
    and a 32-bit and a 64-bit scan issued back to back on one stream never
    read each other's words. ``family`` keeps the plain and the segmented
    64-bit scans (tiles of ``tile`` elements) apart in the same way."""
    tiles = (x.numel() + tile - 1) // tile
    nbytes = 32 * tiles + 32 * (tiles // 64 + 1) + 64  # scan64.h lb64_ws_bytes
    k = (f"{family}:{_ext.stream_ptr(x.device)}", x.device.index)
    t = _ws_cache.get(k)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=x.device)
        _ws_cache[k] = t
        _epochs[k] = 0
    if torch.cuda.is_current_stream_capturing():
        return t, 0  # the graph zeroes the array at every replay (see _lookback_ws)
    e = _epochs[k] + 1
    if e >= _EPOCH_LIMIT:
        t.zero_()
        e = 1
    _epochs[k] = e
    return t, e


def _run_ws(x: torch.Tensor) -> torch.Tensor:
    """Descriptors for launches that zero them natively and number their own
    epochs (spmv_scan_run, tuning arms): kept apart from :func:`_lookback_ws`,
    whose epoch count their words would otherwise collide with."""
    import ctypes

    nbytes = ctypes.c_longlong(0)
    _ext.call_hip("cme_spmv_scan_ws_bytes", x.numel(), ctypes.addressof(nbytes))
    return workspace(x.device, nbytes.value, f"lookback-run:{_ext.stream_ptr(x.device)}")


_ext.proto(_ext.HIP_PROTOS, "cme_spmv_scan_ws_bytes", "qp")
_ext.proto(_ext.HIP_PROTOS, "cme_lookback_timeout_word", "p")
_timeout_words: dict = {}


def _tw(device: torch.device | str | None = None):
    """The look-back give-up word of ``device`` (default: the current one):
    pinned host memory the kernels store to (lookback.h), one word per
    device, readable without a device synchronisation."""
    import ctypes

    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    w = _timeout_words.get(idx)
    if w is None:
        p = ctypes.c_void_p()
        with torch.cuda.device(idx):
            _ext.call_hip("cme_lookback_timeout_word", ctypes.addressof(p))
        w = ctypes.c_uint.from_address(p.value)
        _timeout_words[idx] = w
    return w


def lookback_timed_out(device: torch.device | str = "cuda") -> bool:
    """True if a look-back launch on ``device`` (since the last check) hit its
    bounded-spin limit -- its result is wrong. Synchronises the device."""
    torch.cuda.synchronize(torch.device(device))
    return _tw(device).value != 0


def check_lookback(device: torch.device | str = "cuda") -> None:
    """Synchronise and raise if any look-back launch gave up (then clear)."""
    if lookback_timed_out(device):
        _tw(device).value = 0
        raise RuntimeError("look-back scan spin limit exceeded: a result since the last check is invalid")


def _check_lookback(x: torch.Tensor, before: bool = False) -> None:
    """Called around every look-back launch. Before one: the give-up word of
    EARLIER launches is read without a sync (it is sticky host memory) and
    raised. After one: only under CME_SYNC_CHECK (which synchronises)."""
    w = _tw(x.device)
    if before:
        if w.value != 0:
            w.value = 0
            raise RuntimeError("an earlier look-back scan hit its spin limit (its result was invalid)")
    elif _ext.SYNC_CHECK:
        check_lookback(x.device)


def scan(x: torch.Tensor, exclusive: bool = False, out: torch.Tensor | None = None,
         algo: str = "auto", op: str = "sum", dim: int | None = None, return_indices: bool = False):
    """Prefix sum of a 1-D contiguous float32/int32/uint32/int64/float64 tensor.
    ``op="max"`` / ``"min"``: the running maximum / minimum instead, see
    :func:`cummax`. ``dim=None`` scans the flattened tensor; ``dim=d`` scans a
    tensor of any rank along dimension ``d`` and returns a tensor of ``x``'s
    shape, see :func:`_scan_dim`. ``return_indices=True`` (max / min only):
    the named pair ``(values, indices)`` of :func:`_cumarg`.
    algo: "auto" ("lookback" for 32-bit integers, whose sums are exact in any
    order; "rts" for float32 and float64, whose fixed summation tree is bitwise
    reproducible -- look-back's float prefixes depend on which predecessor had
    published its inclusive value, so neither float32 nor float64 is bitwise
    reproducible with it; int64: see ``_AUTO_INT64``), "lookback" (single
    pass), "rts" (reduce-then-scan with DPP wave scans, deterministic),
    "blelloch" / "hillis" (reduce-then-scan whose block level is the lecture's
    LDS tree algorithm), "blelloch_mlevel" / "hillis_mlevel" (the recursive
    scan-then-add of my-refs/scan.pdf Fig. 5).

    int64 and float64 take "rts" and "lookback" only (a ``TypeError`` names
    them otherwise). int64 sums wrap modulo 2^64, as ``torch.cumsum`` and numpy
    do; a uint64 sum is the int64 sum of the same bits (``.view``). The data
    need only be 8-byte aligned (``x[1:]`` is fine); a 32-bit ``x`` or ``out``
    that is not 16-byte aligned is staged through an aligned copy on the GPU
    (the ``_mlevel`` forms take it as it is). ``out`` (same dtype and length,
    contiguous) may be ``x`` itself for "rts" and "lookback"."""
    if op not in _OPS:
        raise ValueError(f"scan: op {op!r} is not one of {sorted(_OPS)}")
    if return_indices:
        return _cumarg(x, exclusive, out, algo, op, dim)
    if dim is not None:
        return _scan_dim(x, exclusive, out, algo, op, dim)
    if op != "sum":
        return _scan_minmax(x, exclusive, out, algo, op)
    if not x.is_contiguous():
        x = x.contiguous()
    if out is not None and (out.dtype != x.dtype or out.numel() != x.numel() or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError("scan: out must be a contiguous tensor of x's dtype, length and device")
    out = torch.empty_like(x) if out is None else out
    n = x.numel()
    wide = x.dtype in _DT64
    if wide and algo not in ("auto",) + _ALGOS64:
        raise TypeError(f"scan: algo {algo!r} is 32-bit only; {x.dtype} input takes "
                        + " or ".join(repr(a) for a in _ALGOS64))
    if algo == "auto":
        if wide:
            algo = "rts" if x.dtype == torch.float64 else _AUTO_INT64
        else:
            algo = "rts" if x.dtype == torch.float32 else "lookback"
    if x.is_cuda and wide:
        s = _ext.stream_ptr(x.device)
        if algo == "lookback":
            _check_lookback(x, before=True)
            ws, epoch = _lookback64_ws(x)
            _ext.call_hip("cme_scan", x.data_ptr(), out.data_ptr(), n, _DT64[x.dtype], int(exclusive),
                          ws.data_ptr(), epoch, s)
            _check_lookback(x)
        else:
            _ext.call_hip("cme_scan_rts", x.data_ptr(), out.data_ptr(), n, _DT64[x.dtype], int(exclusive),
                          workspace(x.device, 8192, "rts").data_ptr(), s)
    elif x.is_cuda and algo in _VECTOR_ALGOS and (x.data_ptr() % 16 or out.data_ptr() % 16):
        # a view that is only 4-byte aligned (x[1:]): scan an aligned copy,
        # into an aligned result (see _aligned)
        staged = scan(_aligned(x), exclusive, out if out.data_ptr() % 16 == 0 else None, algo)
        if staged is not out:
            out.copy_(staged)
    elif x.is_cuda:
        s = _ext.stream_ptr(x.device)
        if algo == "lookback":
            _check_lookback(x, before=True)
            ws, epoch = _lookback_ws(x)
            _ext.call_hip("cme_scan", x.data_ptr(), out.data_ptr(), n, _DT_SCAN[x.dtype], int(exclusive),
                          ws.data_ptr(), epoch, s)
            _check_lookback(x)
        elif algo == "rts":
            _ext.call_hip("cme_scan_rts", x.data_ptr(), out.data_ptr(), n, _DT_SCAN[x.dtype], int(exclusive),
                          workspace(x.device, 8192, "rts").data_ptr(), s)
        elif algo in ("blelloch", "hillis"):
            # one 4-B sum / prefix per 4096-element tile
            ws = workspace(x.device, 4 * ((n + 4095) // 4096) + 256, "tree")
            _ext.call_hip("cme_scan_tree", x.data_ptr(), out.data_ptr(), n, _DT_SCAN[x.dtype],
                          0 if algo == "blelloch" else 1, int(exclusive), ws.data_ptr(), s)
        elif algo in ("blelloch_mlevel", "hillis_mlevel"):
            if out.data_ptr() == x.data_ptr() and not exclusive:
                raise ValueError("in-place inclusive multi-level scan is not supported")
            levels, b = 0, (n + 511) // 512
            while b > 1:
                levels += b
                b = (b + 511) // 512
            ws = workspace(x.device, (levels + 1) * 4, "mlevel")
            _ext.call_hip("cme_scan_mlevel", x.data_ptr(), out.data_ptr(), n, _DT[x.dtype],
                          0 if algo == "blelloch_mlevel" else 1, int(exclusive), ws.data_ptr(), s)
        else:
            raise ValueError(f"unknown scan algo {algo!r}")
    else:
        _ext.call_cpu("cme_cpu_scan", x.data_ptr(), out.data_ptr(), n, _DT64[x.dtype] if wide else _DT_SCAN[x.dtype],
                      int(exclusive))
    return out


def _scan_minmax(x: torch.Tensor, exclusive: bool, out: torch.Tensor | None, algo: str, op: str) -> torch.Tensor:
    if x.dtype not in _DT_SCAN and x.dtype not in _DT64:
        raise TypeError(f"scan: {x.dtype} is not supported")
    if algo not in ("auto",) + _ALGOS_MINMAX:
        raise TypeError(f"scan: algo {algo!r} is sum only; op={op!r} takes "
                        + " or ".join(repr(a) for a in _ALGOS_MINMAX))
    if not x.is_contiguous():
        x = x.contiguous()
    if out is not None and (out.dtype != x.dtype or out.numel() != x.numel() or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError("scan: out must be a contiguous tensor of x's dtype, length and device")
    out = torch.empty_like(x) if out is None else out
    if algo == "auto":
        algo = _AUTO_MINMAX[x.dtype]
    n = x.numel()
    wide = x.dtype in _DT64
    code = _DT64[x.dtype] if wide else _DT_SCAN[x.dtype]
    if not x.is_cuda:
        _ext.call_cpu("cme_cpu_scan_op", x.data_ptr(), out.data_ptr(), n, code, _OPS[op], int(exclusive))
        return out
    if not wide and (x.data_ptr() % 16 or out.data_ptr() % 16):
        # a 32-bit view that is only 4-byte aligned: see scan() and _aligned
        staged = _scan_minmax(_aligned(x), exclusive, out if out.data_ptr() % 16 == 0 else None, algo, op)
        if staged is not out:
            out.copy_(staged)
        return out
    s = _ext.stream_ptr(x.device)
    if algo == "lookback":
        # the descriptors and the epoch count of the sum scans of this width
        _check_lookback(x, before=True)
        ws, epoch = _lookback64_ws(x) if wide else _lookback_ws(x)
        _ext.call_hip("cme_scan_op", x.data_ptr(), out.data_ptr(), n, code, _OPS[op], int(exclusive),
                      ws.data_ptr(), epoch, s)
        _check_lookback(x)
    else:
        _ext.call_hip("cme_scan_rts_op", x.data_ptr(), out.data_ptr(), n, code, _OPS[op], int(exclusive),
                      workspace(x.device, 8192, "rts").data_ptr(), s)
    return out


def cummax(x: torch.Tensor, exclusive: bool = False, out: torch.Tensor | None = None,
           algo: str = "auto", dim: int | None = None, return_indices: bool = False):
    """Running maximum of a 1-D float32/int32/uint32/int64/float64 tensor:
    ``out[i] = max(x[0..i])``, the values of ``torch.cummax(x, 0)`` bit for bit.
    NaN is sticky -- every output from the first NaN on is
    NaN -- and among equal values the later element wins, which shows only
    between ``+0.0`` and ``-0.0``. ``exclusive``: ``out[0]`` is the identity
    (``-inf``; the type's minimum for integers) and ``out[i]`` the inclusive
    ``out[i-1]``.

    ``algo``: "lookback" (single pass; also "auto" for every dtype: the
    operator is exactly associative, so the result does not depend on the order
    in which workgroups publish) or "rts" (reduce-then-scan); any other raises
    a ``TypeError``. ``out``, alignment and the CPU backend as :func:`scan`.
    ``dim=d``: ``torch.cummax(x, d).values`` of a tensor of any rank.

    ``return_indices=True``: the named pair ``(values, indices)`` of
    ``torch.cummax`` -- ``values`` as above, ``indices`` the int64 position of
    the winner along ``dim`` (in the flattened tensor for ``dim=None``), the
    later of equal values and of NaNs; see :func:`_cumarg`."""
    return scan(x, exclusive, out, algo, op="max", dim=dim, return_indices=return_indices)


def cummin(x: torch.Tensor, exclusive: bool = False, out: torch.Tensor | None = None,
           algo: str = "auto", dim: int | None = None, return_indices: bool = False):
    """Running minimum: the mirror image of :func:`cummax` (identity ``+inf`` /
    the type's maximum)."""
    return scan(x, exclusive, out, algo, op="min", dim=dim, return_indices=return_indices)


_ext.proto(_ext.HIP_PROTOS, "cme_scan_dim", "ppqqqiiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_dim_info", "qqqiiip")
_ext.proto(_ext.HIP_PROTOS, "cme_scan_dim_ws_bytes", "qqqip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_scan_dim", "ppqqqiii")

_DIM_FORMS = ("flat", "row", "col")
_retired_graph_ws: list = []


def _dtype_code(dtype: torch.dtype) -> int:
    if dtype in _DT64:
        return _DT64[dtype]
    if dtype in _DT_SCAN:
        return _DT_SCAN[dtype]
    raise TypeError(f"scan: {dtype} is not supported")


def _split_dim(shape, dim: int) -> tuple[int, int, int]:
    """(outer, n, inner) of scanning ``shape`` along ``dim``."""
    nd = len(shape)
    if nd == 0:
        raise ValueError("scan: dim= needs a tensor of at least one dimension")
    if not -nd <= dim < nd:
        raise IndexError(f"scan: dim {dim} is out of range for a tensor of {nd} dimension(s)")
    d = dim % nd
    outer = inner = 1
    for s in shape[:d]:
        outer *= int(s)
    for s in shape[d + 1:]:
        inner *= int(s)
    return outer, int(shape[d]), inner


def _dim_ws(device: torch.device, nbytes: int, family: str = "scan_dim") -> torch.Tensor | None:
    """Chunk totals of a scan along a dimension, grown before the launch and
    never under stream capture. Eager launches use a buffer per (device,
    stream). A capture (whose stream is not the one of the warm-up) uses one
    buffer per device, which every eager launch keeps at least as large as its
    own, so the scan is run once before it is captured; a buffer that a graph
    may still write to is kept alive when a larger one replaces it. ``family``
    keeps the buffers of the indexed scans ("cumarg_dim") apart from those of
    the values-only ones: a captured scan of one kind never shares its totals
    with a scan of the other."""
    if nbytes == 0:
        return None
    gkey = (f"{family}:graph", device.index)
    g = _ws_cache.get(gkey)
    if torch.cuda.is_current_stream_capturing():
        if g is None or g.numel() < nbytes:
            raise RuntimeError("scan: the chunk-total workspace cannot grow under stream capture; "
                               "run the scan once before capturing it")
        return g
    if g is None or g.numel() < nbytes:
        if g is not None:
            _retired_graph_ws.append(g)
        _ws_cache[gkey] = torch.empty(max(nbytes, 1 << 16), dtype=torch.uint8, device=device)
    return workspace(device, nbytes, f"{family}:{_ext.stream_ptr(device)}")


def _scan_dim(x: torch.Tensor, exclusive: bool, out: torch.Tensor | None, algo: str, op: str, dim: int) -> torch.Tensor:
    """``scan(..., dim=d)``: the scan of a tensor of any rank along dimension
    ``d``, seen as ``(outer, n, inner)`` with element ``(o, i, j)`` at
    ``(o*n + i)*inner + j`` (``csrc/hip/scan_dim.hip``: the row form for
    ``inner == 1``, the column form otherwise; CPU: ``cme_cpu_scan_dim``). The
    rules are those of the 1-D scans: integer sums wrap, max / min are the
    values of ``torch.cummax`` / ``torch.cummin``, ``exclusive`` starts every
    line with the identity. Float sums are bitwise reproducible from run to
    run: no kernel waits for another workgroup, ``n`` is split by chunked
    reduce-then-scan where the lines alone cannot fill the device. ``out``
    (contiguous, ``x``'s dtype, shape and device) may be ``x``. With
    ``outer == inner == 1`` the call is the 1-D scan and takes its ``algo``;
    otherwise ``algo`` must be "auto"."""
    outer, n, inner = _split_dim(x.shape, dim)
    code = _dtype_code(x.dtype)
    if not x.is_contiguous():
        x = x.contiguous()
    if out is not None and (out.dtype != x.dtype or out.shape != x.shape or out.device != x.device
                            or not out.is_contiguous()):
        raise ValueError("scan: out must be a contiguous tensor of x's dtype, shape and device")
    if outer == 1 and inner == 1 and n > 0:
        flat = scan(x.reshape(-1), exclusive, None if out is None else out.reshape(-1), algo, op)
        return flat.view(x.shape) if out is None else out
    if algo != "auto":
        raise TypeError(f"scan: algo {algo!r} is for the 1-D scans; a scan along a dimension of a batched shape "
                        "takes algo='auto' only")
    out = torch.empty_like(x) if out is None else out
    if x.numel() == 0:
        return out
    if not x.is_cuda:
        _ext.call_cpu("cme_cpu_scan_dim", x.data_ptr(), out.data_ptr(), outer, n, inner, code, _OPS[op], int(exclusive))
        return out
    import ctypes

    nbytes = ctypes.c_longlong(0)
    with torch.cuda.device(x.device):
        _ext.call_hip("cme_scan_dim_ws_bytes", outer, n, inner, code, ctypes.addressof(nbytes))
        ws = _dim_ws(x.device, nbytes.value)
        _ext.call_hip("cme_scan_dim", x.data_ptr(), out.data_ptr(), outer, n, inner, code, _OPS[op], int(exclusive),
                      None if ws is None else ws.data_ptr(), _ext.stream_ptr(x.device))
    return out


_ext.proto(_ext.HIP_PROTOS, "cme_cumarg_dim", "pppqqqiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_cumarg_dim_info", "qqqiip")
_ext.proto(_ext.HIP_PROTOS, "cme_cumarg_dim_ws_bytes", "qqqip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_cumarg_dim", "pppqqqii")

ScanWithIndices = collections.namedtuple("ScanWithIndices", ["values", "indices"])


def _cumarg(x: torch.Tensor, exclusive: bool, out, algo: str, op: str, dim: int | None) -> ScanWithIndices:
    """``cummax`` / ``cummin`` with ``return_indices=True``: the named pair
    ``(values, indices)`` of ``torch.cummax`` / ``torch.cummin``. ``values`` is
    what the call without indices returns, bit for bit; ``indices`` is int64,
    contiguous, of ``x``'s shape: the position along ``dim`` (in the flattened
    tensor for ``dim=None``) of the element the running value comes from. Of
    equal values (``+0.0`` / ``-0.0`` included) the later one is named, a
    later NaN takes the index from an earlier one, and every output has a real
    index, a line of all ``-inf`` or all type-minimum too.

    The tensor is seen as ``(outer, n, inner)`` like :func:`_scan_dim` and run
    by the kernels of ``csrc/hip/scan_dim_arg.hip`` under the same launch plan
    (:func:`scan_dim_launch_info` with ``indices=True``); a single line, the
    flattened case included, is a row chunked across the device -- the
    look-back kernels have no index output. CPU: ``cme_cpu_cumarg_dim``.
    ``out`` may be a pair ``(values_out, indices_out)`` of contiguous tensors
    of ``x``'s shape and device (``x``'s dtype and int64); ``values_out`` may
    be ``x``, ``indices_out`` must overlap neither. There is no exclusive mode
    (element 0 would have no index) and ``algo`` must be "auto". The chunk
    totals have buffers of their own, apart from those of the values-only
    scans; under stream capture the same rule holds: run the call once before
    capturing it."""
    if op == "sum":
        raise ValueError("scan: return_indices is for op='max' / 'min'; a sum has no index")
    if exclusive:
        raise ValueError("scan: return_indices has no exclusive mode (element 0 would have no index)")
    if algo != "auto":
        raise TypeError(f"scan: algo {algo!r} has no index output; return_indices takes algo='auto' only")
    if x.ndim == 0:
        raise ValueError("scan: return_indices needs a tensor of at least one dimension")
    outer, n, inner = (1, x.numel(), 1) if dim is None else _split_dim(x.shape, dim)
    code = _dtype_code(x.dtype)
    if out is None:
        vout = iout = None
    elif isinstance(out, (tuple, list)) and len(out) == 2 and all(isinstance(t, torch.Tensor) for t in out):
        vout, iout = out
    else:
        raise ValueError("scan: with return_indices, out must be a pair (values_out, indices_out) of tensors")
    if not x.is_contiguous():
        x = x.contiguous()
    if vout is not None and (vout.dtype != x.dtype or vout.shape != x.shape or vout.device != x.device
                             or not vout.is_contiguous()):
        raise ValueError("scan: values out must be a contiguous tensor of x's dtype, shape and device")
    if iout is not None and (iout.dtype != torch.int64 or iout.shape != x.shape or iout.device != x.device
                             or not iout.is_contiguous()):
        raise ValueError("scan: indices out must be a contiguous int64 tensor of x's shape and device")
    vout = torch.empty_like(x) if vout is None else vout
    iout = torch.empty(x.shape, dtype=torch.int64, device=x.device) if iout is None else iout
    res = ScanWithIndices(vout, iout)
    if x.numel() == 0:
        return res
    if not x.is_cuda:
        _ext.call_cpu("cme_cpu_cumarg_dim", x.data_ptr(), vout.data_ptr(), iout.data_ptr(), outer, n, inner, code,
                      _OPS[op])
        return res
    import ctypes

    nbytes = ctypes.c_longlong(0)
    with torch.cuda.device(x.device):
        _ext.call_hip("cme_cumarg_dim_ws_bytes", outer, n, inner, code, ctypes.addressof(nbytes))
        ws = _dim_ws(x.device, nbytes.value, "cumarg_dim")
        _ext.call_hip("cme_cumarg_dim", x.data_ptr(), vout.data_ptr(), iout.data_ptr(), outer, n, inner, code,
                      _OPS[op], None if ws is None else ws.data_ptr(), _ext.stream_ptr(x.device))
    return res


def scan_dim_launch_info(shape, dim: int, dtype: torch.dtype = torch.float32, op: str = "sum",
                         exclusive: bool = False, device: torch.device | str = "cuda", indices: bool = False) -> dict:
    """How ``scan(x, dim=dim)`` of a 16-byte aligned tensor of ``shape`` runs on
    ``device``: ``form`` ("flat": the 1-D path, "row", "col"), ``outer``, ``n``,
    ``inner``, ``chunks`` (K along ``n``; 1 is a single pass) of ``chunk``
    elements, ``tile`` (elements of a line per workgroup -- or wave -- step;
    column form: rows of loads in flight per lane), ``vector`` (elements per
    lane access; 1 means scalar), ``waves`` (row form: waves that share a
    line), ``workgroups`` and ``ws_bytes``. The CPU backend reports the shape
    split only (``chunks`` 1, no workgroups).

    ``indices=True`` (inclusive only; the plan does not depend on ``op``, and
    the default "sum" is read as "max"): the plan of the indexed kernels behind
    ``return_indices=True``. It is the same plan; ``tile`` is that of the
    indexed row kernels, ``ws_bytes`` holds the value and the int64 index
    totals, and "flat" (a single line) runs as a row chunked across the device,
    not as the 1-D look-back scan."""
    import ctypes

    if op not in _OPS:
        raise ValueError(f"scan: op {op!r} is not one of {sorted(_OPS)}")
    if indices:
        op = "max" if op == "sum" else op
        if exclusive:
            raise ValueError("scan: return_indices has no exclusive mode")
    outer, n, inner = _split_dim(tuple(shape), dim)
    code = _dtype_code(dtype)
    form = 0 if outer == 1 and inner == 1 else 1 if inner == 1 else 2
    d = {"form": _DIM_FORMS[form], "outer": outer, "n": n, "inner": inner, "chunks": 1, "chunk": n, "tile": 0,
         "vector": 1, "waves": 0, "workgroups": 0, "ws_bytes": 0}
    dev = torch.device(device)
    if dev.type != "cuda":
        return d
    info = (ctypes.c_longlong * 8)()
    with torch.cuda.device(dev):
        if indices:
            _ext.call_hip("cme_cumarg_dim_info", outer, n, inner, code, _OPS[op], ctypes.addressof(info))
        else:
            _ext.call_hip("cme_scan_dim_info", outer, n, inner, code, _OPS[op], int(exclusive), ctypes.addressof(info))
    d.update(form=_DIM_FORMS[int(info[0])], chunks=int(info[1]), chunk=int(info[2]), tile=int(info[3]),
             vector=int(info[4]), workgroups=int(info[5]), ws_bytes=int(info[6]), waves=int(info[7]))
    return d


def summed_area_table(x: torch.Tensor, out: torch.Tensor | None = None) -> torch.Tensor:
    """Summed-area table over the last two dimensions of ``x`` (any scan
    dtype, at least 2-D): ``out[..., i, j] = sum(x[..., :i+1, :j+1])``, a row
    scan (``dim=-1``) followed by a column scan (``dim=-2``) in place. The sum
    of any box is then four look-ups. Integer sums wrap."""
    if x.ndim < 2:
        raise ValueError("summed_area_table: x must have at least two dimensions")
    out = scan(x, out=out, dim=-1)
    return scan(out, out=out, dim=-2)


_ext.proto(_ext.HIP_PROTOS, "cme_reduce_dim", "pppqqqiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_reduce_dim_info", "qqqiiip")
_ext.proto(_ext.HIP_PROTOS, "cme_reduce_dim_ws_bytes", "qqqiip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_reduce_dim", "pppqqqii")

ReduceWithIndices = collections.namedtuple("ReduceWithIndices", ["values", "indices"])


def _reduce_split(shape, dim: int | None) -> tuple[int, int, int, int | None]:
    """(outer, n, inner, d) of reducing ``shape`` along ``dim`` (``d``: the
    non-negative dimension); the flattened tensor for ``dim=None`` (``d`` None)."""
    if dim is None:
        n = 1
        for s in shape:
            n *= int(s)
        return 1, n, 1, None
    try:
        outer, n, inner = _split_dim(shape, dim)
    except (ValueError, IndexError) as e:
        raise type(e)(str(e).replace("scan:", "reduce:")) from None
    return outer, n, inner, dim % len(shape)


def _reduced_shape(shape, d: int | None, keepdim: bool) -> tuple:
    shape = tuple(int(s) for s in shape)
    if d is None:
        return (1,) * len(shape) if keepdim else ()
    return shape[:d] + ((1,) if keepdim else ()) + shape[d + 1:]


def _reduce_dim(x: torch.Tensor, op: str, dim: int | None, keepdim: bool, indices: bool):
    """The reduction of ``x`` along ``dim`` (``None``: of the flattened
    tensor), seen as ``(outer, n, inner)`` like :func:`_scan_dim`; the kernels
    of ``csrc/hip/reduce_dim.hip`` under the launch plan of the scans along a
    dimension (:func:`reduce_dim_launch_info`), ``cme_cpu_reduce_dim`` on CPU
    tensors. Returns ``(values, indices)``, ``indices`` None unless asked for.
    Neither synchronises."""
    if op not in _OPS:
        raise ValueError(f"reduce: op {op!r} is not one of {sorted(_OPS)}")
    if indices and op == "sum":
        raise ValueError("reduce: return_indices is for op='max' / 'min'; a sum has no index")
    if x.dtype not in _DT64 and x.dtype not in _DT_SCAN:
        raise TypeError(f"reduce: {x.dtype} is not supported along a dimension")
    code = _dtype_code(x.dtype)
    outer, n, inner, d = _reduce_split(x.shape, dim)
    shape = _reduced_shape(x.shape, d, keepdim)
    if n == 0:
        if op != "sum":
            raise ValueError(f"reduce: {op} of an empty dimension has no value")
        return torch.zeros(shape, dtype=x.dtype, device=x.device), None
    if not x.is_contiguous():
        x = x.contiguous()
    vout = torch.empty(shape, dtype=x.dtype, device=x.device)
    iout = torch.empty(shape, dtype=torch.int64, device=x.device) if indices else None
    if outer == 0 or inner == 0:
        return vout, iout
    iptr = None if iout is None else iout.data_ptr()
    if not x.is_cuda:
        _ext.call_cpu("cme_cpu_reduce_dim", x.data_ptr(), vout.data_ptr(), iptr, outer, n, inner, code, _OPS[op])
        return vout, iout
    import ctypes

    nbytes = ctypes.c_longlong(0)
    with torch.cuda.device(x.device):
        _ext.call_hip("cme_reduce_dim_ws_bytes", outer, n, inner, code, int(indices), ctypes.addressof(nbytes))
        ws = _dim_ws(x.device, nbytes.value, "reduce_arg_dim" if indices else "reduce_dim")
        _ext.call_hip("cme_reduce_dim", x.data_ptr(), vout.data_ptr(), iptr, outer, n, inner, code, _OPS[op],
                      None if ws is None else ws.data_ptr(), _ext.stream_ptr(x.device))
    return vout, iout


def reduce(x: torch.Tensor, op: str = "sum", algo: str = "vector", dim: int | None = None, keepdim: bool = False,
           return_indices: bool = False):
    """Reduction (``op``: "sum", "max", "min").

    Without ``dim``, ``keepdim`` and ``return_indices``: the full reduction of
    a float32/int32/int64/float64 tensor; returns a 0-d tensor on x's device.
    An int64 sum wraps modulo 2^64. ``algo="tree"`` (the lecture's LDS tree,
    sum only) is 32-bit only and raises a ``TypeError`` for 64-bit input. int32
    sums wrap modulo 2^32 on both backends. A 32-bit view that is not 16-byte
    aligned is copied for ``algo="vector"`` on the GPU.

    With any of the three: the reduction along dimension ``dim`` (one int,
    negative allowed; ``None``: the flattened tensor) of a tensor of any rank
    and any scan dtype (float32, int32, uint32, int64, float64), by
    ``csrc/hip/reduce_dim.hip`` / ``cme_cpu_reduce_dim``; ``algo`` must stay at
    its default. ``keepdim`` keeps the reduced dimension with size 1 (every
    dimension for ``dim=None``). The rules, the same on both backends:

    * "sum" keeps ``x``'s dtype (no promotion); integers wrap. A float sum is a
      tree fixed by the launch shape and the operand's 16-byte phase: two runs
      of one call are bitwise equal. An empty dimension sums to zero.
    * "max" / "min" are the IEEE 754-2019 maximum / minimum: a NaN in the line
      gives NaN, ``max(+0.0, -0.0)`` is ``+0.0`` and ``min`` is ``-0.0``. An
      empty dimension raises ``ValueError``.
    * ``return_indices=True`` ("max" / "min" only) returns the named pair
      ``(values, indices)`` of ``torch.max(x, dim)`` / ``torch.min(x, dim)`` on
      CPU tensors: the index (int64, along ``dim``, or in the flattened tensor)
      of the first NaN if the line has one, else of the first element equal to
      the extreme; ``values`` is ``x`` at that index, bit for bit.

    The chunk partials of a launch that splits ``n`` live in buffers of their
    own ("reduce_dim" / "reduce_arg_dim" families of :func:`_dim_ws`), so under
    stream capture the rule of the scans holds: run the call once before
    capturing it."""
    if dim is not None or keepdim or return_indices:
        if algo != "vector":
            raise TypeError(f"reduce: algo {algo!r} is for the flattened reduction; with dim, keepdim or "
                            "return_indices, algo stays at its default")
        v, i = _reduce_dim(x, op, dim, keepdim, return_indices)
        return ReduceWithIndices(v, i) if return_indices else v
    x = x.contiguous()
    wide = x.dtype in _DT64
    if wide and algo != "vector":
        raise TypeError(f"reduce: algo {algo!r} is 32-bit only; {x.dtype} input takes 'vector'")
    dt = _DT64[x.dtype] if wide else _DT[x.dtype]
    out = torch.empty((), dtype=x.dtype, device=x.device)
    if x.is_cuda:
        if not wide and algo == "vector":
            x = _aligned(x)  # 16-byte loads; the LDS tree loads scalars
        part = workspace(x.device, 2048 * 4, "reduce")
        _ext.call_hip("cme_reduce", x.data_ptr(), x.numel(), dt, _OPS[op], 0 if algo == "vector" else 1,
                      part.data_ptr(), out.data_ptr(), _ext.stream_ptr(x.device))
    else:
        _ext.call_cpu("cme_cpu_reduce", x.data_ptr(), x.numel(), dt, _OPS[op], out.data_ptr())
    return out


def argmax(x: torch.Tensor, dim: int | None = None, keepdim: bool = False) -> torch.Tensor:
    """``torch.argmax(x, dim, keepdim)``: the ``indices`` of
    ``reduce(x, "max", dim=dim, keepdim=keepdim, return_indices=True)``, an
    int64 tensor on ``x``'s device. No host synchronisation."""
    return _reduce_dim(x, "max", dim, keepdim, True)[1]


def argmin(x: torch.Tensor, dim: int | None = None, keepdim: bool = False) -> torch.Tensor:
    """``torch.argmin(x, dim, keepdim)``; see :func:`argmax`."""
    return _reduce_dim(x, "min", dim, keepdim, True)[1]


def reduce_dim_launch_info(shape, dim: int | None, dtype: torch.dtype = torch.float32, op: str = "sum",
                           device: torch.device | str = "cuda", indices: bool = False) -> dict:
    """How ``reduce(x, op, dim=dim)`` of a 16-byte aligned tensor of ``shape``
    runs on ``device``: the keys of :func:`scan_dim_launch_info`, from the same
    plan. ``form`` "flat" (a single line, ``dim=None`` included) runs as a row
    chunked across the device; ``workgroups`` is the grid of the reduce pass,
    and ``ws_bytes`` holds one partial per (line, chunk) when ``chunks > 1``
    (with ``indices=True``, where the default "sum" is read as "max", an int64
    index beside every value). The CPU backend reports the shape split only."""
    import ctypes

    if op not in _OPS:
        raise ValueError(f"reduce: op {op!r} is not one of {sorted(_OPS)}")
    if indices and op == "sum":
        op = "max"
    outer, n, inner, _ = _reduce_split(tuple(shape), dim)
    code = _dtype_code(dtype)
    form = 0 if outer == 1 and inner == 1 else 1 if inner == 1 else 2
    d = {"form": _DIM_FORMS[form], "outer": outer, "n": n, "inner": inner, "chunks": 1, "chunk": n, "tile": 0,
         "vector": 1, "waves": 0, "workgroups": 0, "ws_bytes": 0}
    dev = torch.device(device)
    if dev.type != "cuda":
        return d
    info = (ctypes.c_longlong * 8)()
    with torch.cuda.device(dev):
        _ext.call_hip("cme_reduce_dim_info", outer, n, inner, code, _OPS[op], int(indices), ctypes.addressof(info))
    d.update(form=_DIM_FORMS[int(info[0])], chunks=int(info[1]), chunk=int(info[2]), tile=int(info[3]),
             vector=int(info[4]), workgroups=int(info[5]), ws_bytes=int(info[6]), waves=int(info[7]))
    return d


def head_flags_from_offsets(s: torch.Tensor, n: int, device=None, bitmask: bool = True) -> torch.Tensor:
    """Segment heads from the final project's offset array ``s`` (s[0] = 0,
    s[p-1] = n, strictly increasing; segment i = [s[i-1], s[i])). Returns a
    bitmask (int32 words, bit i%32 of word i/32) or a uint8 per element."""
    heads = s[:-1].to(torch.int64)
    if bitmask:
        words = torch.zeros((n + 31) // 32, dtype=torch.int64)
        w = heads // 32
        bit = torch.ones_like(heads) << (heads % 32)
        words.index_add_(0, w, bit)  # heads are distinct: add == or
        words = torch.where(words >= 2**31, words - 2**32, words).to(torch.int32)
        return words.to(device) if device is not None else words
    f = torch.zeros(n, dtype=torch.uint8)
    f[heads] = 1
    return f.to(device) if device is not None else f


_ext.proto(_ext.HIP_PROTOS, "cme_segscan64", "ppppiqipup")
_ext.proto(_ext.HIP_PROTOS, "cme_spmv_scan_run64", "pppqipp")
_ext.proto(_ext.HIP_PROTOS, "cme_spmv_scan64_ws_bytes", "qp")
_ext.proto(_ext.HIP_PROTOS, "cme_segscan64_info", "qp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_segscan64", "ppppiqi")

SEGTILE64 = 4096  # elements per tile of the 64-bit segmented scan (scan64.h kSegScan64Tile)
_SEGSCAN_DTYPES = (torch.float32, torch.int64, torch.float64)


def segscan64_launch_info(n: int, device: torch.device | str = "cuda") -> dict:
    """How a 64-bit :func:`segmented_scan` of ``n`` elements is launched on
    ``device``: ``tile`` (elements), ``tiles``, ``workgroups`` (the persistent,
    co-resident grid), ``blocks_per_cu``, ``ws_bytes``."""
    import ctypes

    info = (ctypes.c_longlong * 5)()
    with torch.cuda.device(torch.device(device)):
        _ext.call_hip("cme_segscan64_info", n, ctypes.addressof(info))
    return dict(zip(("tile", "tiles", "workgroups", "blocks_per_cu", "ws_bytes"), (int(v) for v in info)))


def _run64_ws(x: torch.Tensor) -> torch.Tensor:
    """Descriptors of the float64 :func:`spmv_scan_run`, which zeroes them
    natively and numbers its own epochs (see :func:`_run_ws`)."""
    import ctypes

    nbytes = ctypes.c_longlong(0)
    _ext.call_hip("cme_spmv_scan64_ws_bytes", x.numel(), ctypes.addressof(nbytes))
    return workspace(x.device, nbytes.value, f"lookback-run64:{_ext.stream_ptr(x.device)}")


def _segscan_args(x: torch.Tensor, flags: torch.Tensor, out: torch.Tensor | None,
                  mul: torch.Tensor | None) -> tuple[torch.Tensor, torch.Tensor, int]:
    """The operand checks of :func:`segmented_scan` (every dtype, both
    backends): (contiguous x, out, flag mode)."""
    for name, t in (("mul", mul), ("out", out)):
        if t is not None and (t.dtype != x.dtype or t.numel() != x.numel() or t.device != x.device
                              or not t.is_contiguous()):
            raise ValueError(f"segmented_scan: {name} must be a contiguous tensor of x's dtype, length and device")
    if flags.dtype not in (torch.uint8, torch.int32):
        raise TypeError(f"segmented_scan: flags must be uint8 (one per element) or int32 bitmask words, not {flags.dtype}")
    if flags.device != x.device or not flags.is_contiguous():
        raise ValueError("segmented_scan: flags must be contiguous and on x's device")
    n = x.numel()
    mode = 0 if flags.dtype == torch.uint8 else 1
    if flags.numel() < (n if mode == 0 else (n + 31) // 32):
        raise ValueError("segmented_scan: flags are shorter than x")
    if not x.is_contiguous():
        x = x.contiguous()
    return x, (torch.empty_like(x) if out is None else out), mode


def _segscan64(x: torch.Tensor, flags: torch.Tensor, out: torch.Tensor | None, mul: torch.Tensor | None) -> torch.Tensor:
    x, out, mode = _segscan_args(x, flags, out, mul)
    n = x.numel()
    mp = mul.data_ptr() if mul is not None else None
    if x.is_cuda:
        _check_lookback(x, before=True)
        # descriptors and epochs apart from the 32-bit scans' and the plain 64-bit scan's
        ws, epoch = _lookback64_ws(x, SEGTILE64, "segscan64")
        _ext.call_hip("cme_segscan64", x.data_ptr(), mp, out.data_ptr(), flags.data_ptr(), mode, n, _DT64[x.dtype],
                      ws.data_ptr(), epoch, _ext.stream_ptr(x.device))
        _check_lookback(x)
    else:
        _ext.call_cpu("cme_cpu_segscan64", x.data_ptr(), mp, out.data_ptr(), flags.data_ptr(), mode, n, _DT64[x.dtype])
    return out


def segmented_scan(x: torch.Tensor, flags: torch.Tensor, out: torch.Tensor | None = None,
                   mul: torch.Tensor | None = None) -> torch.Tensor:
    """Inclusive segmented sum scan of float32, int64 or float64 ``x``
    (optionally of ``x * mul``). ``flags``: uint8 per element (non-zero: a
    segment head) or int32 bitmask words (bit ``i % 32`` of word ``i // 32``);
    element 0 starts a segment whether or not its flag is set.

    ``mul`` and ``out`` have ``x``'s dtype, length and device; ``out`` may be
    ``x``. int64 sums wrap modulo 2^64. 64-bit data need only be 8-byte aligned
    (``x[1:]`` is fine); float32 views that are not 16-byte aligned, and uint8
    flags that are not 4-byte aligned, are staged through aligned copies on the
    GPU. Any other dtype of ``x`` raises a ``TypeError``, and so do flags that
    are neither uint8 nor int32 (``torch.bool`` included: pass
    ``flags.view(torch.uint8)``); flags must be contiguous, on ``x``'s device
    and cover ``x``. A non-contiguous ``x`` is copied."""
    if x.dtype not in _SEGSCAN_DTYPES:
        raise TypeError(f"segmented_scan: {x.dtype} is not supported; x must be torch.float32, torch.int64 or "
                        "torch.float64")
    if x.dtype in _DT64:
        return _segscan64(x, flags, out, mul)
    x, out, mode = _segscan_args(x, flags, out, mul)
    n = x.numel()
    if x.is_cuda:
        # 16-byte vector loads and stores, four uint8 flags per 4-byte load
        # (int32 bitmask words are 4-byte aligned as they are): see _aligned
        x, flags, dst = _aligned(x), _aligned(flags, 4), out
        mul = _aligned(mul) if mul is not None else None
        if out.data_ptr() % 16:
            dst = torch.empty_like(x)
        _check_lookback(x, before=True)
        ws, epoch = _lookback_ws(x)
        _ext.call_hip("cme_segscan", x.data_ptr(), mul.data_ptr() if mul is not None else None, dst.data_ptr(),
                      flags.data_ptr(), mode, n, ws.data_ptr(), epoch, _ext.stream_ptr(x.device))
        _check_lookback(x)
        if dst is not out:
            out.copy_(dst)
        return out
    _ext.call_cpu("cme_cpu_segscan", x.data_ptr(), mul.data_ptr() if mul is not None else None, out.data_ptr(),
                  flags.data_ptr(), mode, n)
    return out


def spmv_scan_run(a: torch.Tensor, xx: torch.Tensor, flags: torch.Tensor, iters: int) -> torch.Tensor:
    """``iters`` in-place steps ``a <- segscan(a * xx)`` (bitmask heads) of
    float32 or float64 ``a`` / ``xx``, without host synchronisation: one
    persistent launch per 64 steps, with a descriptor set per step
    (``csrc/hip/scan.hip``, ``csrc/hip/segscan64.hip``)."""
    if a.dtype not in (torch.float32, torch.float64):
        raise TypeError(f"spmv_scan_run: {a.dtype} is not supported; a must be torch.float32 or torch.float64")
    if xx.dtype != a.dtype or xx.numel() != a.numel() or xx.device != a.device:
        raise ValueError("spmv_scan_run: xx must have a's dtype, length and device")
    if not a.is_cuda:
        for _ in range(iters):
            segmented_scan(a, flags, out=a, mul=xx)
        return a
    assert flags.dtype == torch.int32, "bitmask flags expected"
    _check_lookback(a, before=True)
    if a.dtype == torch.float64:
        if not (a.is_contiguous() and xx.is_contiguous() and flags.is_contiguous()):
            raise ValueError("spmv_scan_run: a, xx and flags must be contiguous")
        _ext.call_hip("cme_spmv_scan_run64", a.data_ptr(), xx.data_ptr(), flags.data_ptr(), a.numel(), iters,
                      _run64_ws(a).data_ptr(), _ext.stream_ptr(a.device))
        _check_lookback(a)
        return a
    if not (a.is_contiguous() and xx.is_contiguous() and flags.is_contiguous()):
        raise ValueError("spmv_scan_run: a, xx and flags must be contiguous")
    # 16-byte vector loads and stores: see _aligned (both copies are held until
    # the launch is enqueued, so the workspace is never allocated over one)
    run, xs = _aligned(a), _aligned(xx)
    _ext.call_hip("cme_spmv_scan_run", run.data_ptr(), xs.data_ptr(), flags.data_ptr(), a.numel(), iters,
                  _run_ws(a).data_ptr(), _ext.stream_ptr(a.device))
    _check_lookback(a)
    if run is not a:
        a.copy_(run)
    return a
