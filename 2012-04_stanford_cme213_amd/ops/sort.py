"""Sorting: GPU LSD radix sort (8-bit digits, stable, key-value), GPU
merge-path merge sort, and the hw4 OpenMP radix / merge sorts.

Keys: uint32 natively; int32 and float32 are mapped to order-preserving
uint32 codes (sign-bit flip / IEEE total-order trick) and back -- inside the
GPU kernels (first pass loads, last pass stores), on the CPU by tensor ops.
64-bit keys (uint64 / int64 / float64, with 4- or 8-byte values) take the
same route through 64-bit codes: ``csrc/hip/radix64.hip`` on the GPU
(reduce-then-scan only), ``cme_cpu_radix_sort_kv_u64`` on the CPU.
Descending order complements the code, so equal keys keep their input order
(``torch.sort(stable=True, descending=True)``); :func:`argsort` is a
key-value sort of 32-bit positions, widened to int64 at the end.

GPU radix algorithms: "radix" = reduce-then-scan (``csrc/hip/sort.hip``:
upsweep + one-launch count scan + downsweep per 8-bit digit), "onesweep"
(``csrc/hip/radix.hip``: one histogram read for every pass, then one read +
one write of the keys per digit with decoupled look-back across tiles). Both
are stable and exact; reduce-then-scan is the default because it measures
faster on MI355X (16M keys: profiles/sort_r3.md).

``sort(x, dim=d)`` / ``argsort(x, dim=d)`` sort every line of a tensor of any
rank along one dimension and return ``(values, indices)``: a batched LDS radix
sort packing several short lines into one workgroup's tile
(``csrc/hip/sort_dim.hip``), the two 1-D key-value sorts composed for lines
above the tile, ``cme_cpu_sort_dim`` on the CPU.
"""
from __future__ import annotations

import collections

import torch

from .. import _ext

_ext.proto(_ext.HIP_PROTOS, "cme_radix_sort_u32", "ppppqiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_radix_sort", "ppppppqiiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_radix_onesweep", "ppppppqiiipqp")
_ext.proto(_ext.HIP_PROTOS, "cme_radix_lane_order", "i")
_ext.proto(_ext.HIP_PROTOS, "cme_merge_sort_u32", "ppppqp")
_ext.proto(_ext.HIP_PROTOS, "cme_merge_sort", "ppppppqip")
_ext.proto(_ext.HIP_PROTOS, "cme_merge_sort_ws", "ppppppqipp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_radix_sort_u32", "ppqii")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_radix_sort_serial_u32", "ppqi")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_merge_sort_i32", "ppqqqp")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_radix_sort_kv_u32", "ppppqii")
_ext.proto(_ext.HIP_PROTOS, "cme_radix_sort64", "ppppppqiiiipp")
_ext.proto(_ext.HIP_PROTOS, "cme_radix_sort64_tile", "")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_radix_sort_kv_u64", "ppppqiii")
_ext.proto(_ext.HIP_PROTOS, "cme_sort_dim", "pppqqqiip")
_ext.proto(_ext.HIP_PROTOS, "cme_sort_dim_info", "qqqip")
_ext.proto(_ext.CPU_PROTOS, "cme_cpu_sort_dim", "pppqqqii")

SortWithIndices = collections.namedtuple("SortWithIndices", ["values", "indices"])

_MIN32 = -(2 ** 31)
_MIN64 = -(2 ** 63)


def _to_u32(k: torch.Tensor) -> torch.Tensor:
    if k.dtype == torch.uint32:
        return k.clone()
    if k.dtype == torch.int32:
        return (k.view(torch.int32) ^ torch.tensor(-(2 ** 31), dtype=torch.int32, device=k.device)).view(torch.uint32)
    if k.dtype == torch.float32:
        i = k.view(torch.int32)
        mask = torch.where(i < 0, torch.tensor(-1, dtype=torch.int32, device=k.device),
                           torch.tensor(-(2 ** 31), dtype=torch.int32, device=k.device))
        return (i ^ mask).view(torch.uint32)
    raise TypeError(f"unsupported key dtype {k.dtype}")


def _from_u32(u: torch.Tensor, dtype) -> torch.Tensor:
    if dtype == torch.uint32:
        return u
    i = u.view(torch.int32)
    if dtype == torch.int32:
        return i ^ torch.tensor(-(2 ** 31), dtype=torch.int32, device=u.device)
    mask = torch.where(i >= 0, torch.tensor(-1, dtype=torch.int32, device=u.device),
                       torch.tensor(-(2 ** 31), dtype=torch.int32, device=u.device))
    return (i ^ mask).view(torch.float32)


def _to_code64(k: torch.Tensor, descending: bool, plain: bool = False) -> torch.Tensor:
    """Order codes of 64-bit keys as a fresh int64 tensor holding the
    unsigned code's bits: uint64 as is, int64 with the sign bit flipped,
    float64 in IEEE total order; complemented for descending order.
    ``plain``: non-negative integer keys taken as they are (key_bits < 64)."""
    i = k.view(torch.int64)
    if plain or k.dtype == torch.uint64:
        c = i.clone()
    elif k.dtype == torch.int64:
        c = i ^ _MIN64
    else:
        c = i ^ torch.where(i < 0, -1, _MIN64)
    return ~c if descending else c


def _from_code64(c: torch.Tensor, dtype, descending: bool, plain: bool = False) -> torch.Tensor:
    if descending:
        c = ~c
    if plain or dtype == torch.uint64:
        return c.view(dtype)
    if dtype == torch.int64:
        return c ^ _MIN64
    return (c ^ torch.where(c >= 0, -1, _MIN64)).view(torch.float64)


def _reverse32(k: torch.Tensor) -> torch.Tensor:
    """32-bit keys whose ascending order is the descending order of ``k``
    (an involution; equal keys stay equal, so a stable sort keeps their input
    order): the complement for integers, the sign-bit flip for float32 --
    in the IEEE total order that is the exact reverse, NaNs included."""
    i = k.view(torch.int32)
    return (i ^ _MIN32 if k.dtype == torch.float32 else ~i).view(k.dtype)


_ws: dict = {}
_os_ws: dict = {}
_os_epochs: dict = {}
_OS_TILE = 8192
_OS_EPOCH_LIMIT = 1 << 27  # radix.hip: granule tag = epoch * 4 + pass, 30 bits
_MODES = {torch.uint32: 0, torch.int32: 1, torch.float32: 2}
_MODES64 = {torch.uint64: 0, torch.int64: 1, torch.float64: 2}  # cme_radix_sort64: | 4 = descending
RADIX64_TILE = 8192  # keys per downsweep tile of the 64-bit sort (= cme_radix_sort64_tile())


def _check_32bit_algo(dtype, algo: str) -> None:
    if dtype in _MODES64:
        raise TypeError(f"algo={algo!r} sorts 32-bit keys only; {dtype} keys: algo='radix'")
    if dtype not in _MODES:
        raise TypeError(f"unsupported key dtype {dtype}")


def _onesweep_ws(keys: torch.Tensor) -> tuple[torch.Tensor, int]:
    """Workspace + call epoch of a onesweep sort (cf. ops/scan.py
    _lookback_ws): zeroed once when (re)allocated, then every call gets the
    next epoch, so granules of earlier calls never match and no memset runs.
    Keyed by (device, stream); under stream capture a separate workspace with
    epoch 0, which the launcher zeroes inside the graph at every replay."""
    n = keys.numel()
    tiles = (n + _OS_TILE - 1) // _OS_TILE
    nbytes = 2 * 4 * 256 * 4 + tiles * 8 + 2 * tiles * 256 * 8 + 256  # = cme_radix_onesweep_ws_bytes
    capturing = torch.cuda.is_current_stream_capturing()
    k = (f"os:{'cap:' if capturing else ''}{_ext.stream_ptr(keys.device)}", keys.device.index)
    t = _os_ws.get(k)
    if t is None or t.numel() < nbytes:
        t = torch.zeros(max(nbytes, 1 << 16), dtype=torch.uint8, device=keys.device)
        _os_ws[k] = t
        _os_epochs[k] = 0
    if capturing:
        return t, 0
    e = _os_epochs[k] + 1
    if e >= _OS_EPOCH_LIMIT:
        t.zero_()
        e = 1
    _os_epochs[k] = e
    return t, e


def radix_lane_order(check: bool = True) -> bool:
    """Whether the current device resolves the same-address lanes of one
    returning LDS atomic in lane order -- the property the radix downsweep's
    lane-atomic ranks rely on (``csrc/hip/sort.hip`` kRankLanes). ``check``
    runs the library's one-time probe kernel if this device has not been
    checked yet; the radix sort falls back to ballot-match ranks otherwise."""
    return bool(_ext._fn("hip", "cme_radix_lane_order")(1 if check else 0))


def _merge(keys: torch.Tensor, values: torch.Tensor | None):
    """GPU merge sort (csrc/hip/sort.hip cme_merge_sort_ws): stable; 8192-key
    block sorts, then one LDS-staged merge-path pass per doubling of the run
    length; from 8M keys each pass first finds every tile's merge-path split
    in one launch (tuning knob merge_part), below that each merge block
    searches its own; key transforms fused into the first and last kernels.
    Keys-only and key-value tiles are block-sorted by an LDS radix sort
    (tuning knob merge_block_sort). A 4-way pass schedule lives in the tuning
    library (cme_merge_sort4_tune; measured slower: profiles/sort_r6.md)."""
    _check_32bit_algo(keys.dtype, "merge")
    k = keys.contiguous()
    out, tmp = torch.empty_like(k), torch.empty_like(k)
    vp = vo = vt = None
    if values is not None:
        if values.element_size() != 4 or values.numel() != k.numel():
            raise TypeError("values: one 32-bit value per key")
        v = values.contiguous()
        vout, vtmp = torch.empty_like(v), torch.empty_like(v)
        vp, vo, vt = v.data_ptr(), vout.data_ptr(), vtmp.data_ptr()
    ws = _workspace(keys.device, (k.numel() + 4095) // 4096 * 48 + 256)  # = cme_merge_ws_bytes
    _ext.call_hip("cme_merge_sort_ws", k.data_ptr(), out.data_ptr(), tmp.data_ptr(), vp, vo, vt, k.numel(),
                  _MODES[keys.dtype], ws.data_ptr(), _ext.stream_ptr(keys.device))
    return (out, vout) if values is not None else out


def _rts(keys: torch.Tensor, values: torch.Tensor | None, key_bits: int):
    """Reduce-then-scan LSD radix sort (cme_radix_sort): key transforms fused
    into the first and last passes, input untouched."""
    n = keys.numel()
    dtype = keys.dtype
    if dtype not in _MODES:
        raise TypeError(f"unsupported key dtype {dtype}")
    if key_bits < 32 and dtype not in (torch.int32, torch.uint32):
        raise TypeError("key_bits < 32 needs non-negative integer keys")
    mode = 0 if key_bits < 32 else _MODES[dtype]
    bits = 32 if key_bits >= 32 else max(1, int(key_bits))
    k = keys.contiguous()
    out, tmp = torch.empty_like(k), torch.empty_like(k)
    vp = vo = vt = None
    if values is not None:
        if values.element_size() != 4 or values.numel() != n:
            raise TypeError("values: one 32-bit value per key")
        v = values.contiguous()
        vout, vtmp = torch.empty_like(v), torch.empty_like(v)
        vp, vo, vt = v.data_ptr(), vout.data_ptr(), vtmp.data_ptr()
    tiles = (n + 4095) // 4096
    ws = _workspace(keys.device, min(tiles, 4096) * 256 * 4 + 256 * 4 + 256)  # = cme_radix_ws_bytes
    _ext.call_hip("cme_radix_sort", k.data_ptr(), out.data_ptr(), tmp.data_ptr(), vp, vo, vt, n, mode, 0, bits,
                  ws.data_ptr(), _ext.stream_ptr(keys.device))
    return (out, vout) if values is not None else out


def _check_values64(values: torch.Tensor, n: int) -> None:
    if values.element_size() not in (4, 8) or values.numel() != n or values.dim() != 1:
        raise TypeError("values: one 4- or 8-byte value per 64-bit key")


def _rts64(keys: torch.Tensor, values: torch.Tensor | None, key_bits: int, descending: bool):
    """Reduce-then-scan LSD radix sort of 64-bit keys (cme_radix_sort64):
    eight passes at full width, only those covering ``key_bits`` below it;
    the key kind and the descending complement are fused into the first
    pass's loads and the last pass's stores, the input is untouched, values
    (4 or 8 bytes each) move as raw bits."""
    n = keys.numel()
    dtype = keys.dtype
    if key_bits < 64 and dtype == torch.float64:
        raise TypeError("key_bits < 64 needs non-negative integer keys")
    mode = (0 if key_bits < 64 else _MODES64[dtype]) | (4 if descending else 0)
    bits = 64 if key_bits >= 64 else max(1, int(key_bits))
    k = keys.contiguous()
    out, tmp = torch.empty_like(k), torch.empty_like(k)
    vp = vo = vt = None
    vb = 0
    if values is not None:
        _check_values64(values, n)
        v = values.contiguous()
        vb = v.element_size()
        vout, vtmp = torch.empty_like(v), torch.empty_like(v)
        vp, vo, vt = v.data_ptr(), vout.data_ptr(), vtmp.data_ptr()
    tiles = (n + 4095) // 4096
    ws = _workspace(keys.device, min(tiles, 4096) * 256 * 4 + 256 * 4 + 256)  # = cme_radix_ws_bytes
    _ext.call_hip("cme_radix_sort64", k.data_ptr(), out.data_ptr(), tmp.data_ptr(), vp, vo, vt, n, mode, vb, 0, bits,
                  ws.data_ptr(), _ext.stream_ptr(keys.device))
    return (out, vout) if values is not None else out


def _cpu_sort64(keys: torch.Tensor, values: torch.Tensor | None, num_bits: int, key_bits: int, descending: bool):
    """OpenMP LSD radix sort of 64-bit keys (cme_cpu_radix_sort_kv_u64) over
    order codes made by tensor ops."""
    n = keys.numel()
    dtype = keys.dtype
    plain = key_bits < 64
    if plain and dtype == torch.float64:
        raise TypeError("key_bits < 64 needs non-negative integer keys")
    k = _to_code64(keys.contiguous(), descending, plain)
    kt = torch.empty_like(k)
    vp = vt = None
    vb = 0
    if values is not None:
        _check_values64(values, n)
        v = values.contiguous().clone()
        vtmp = torch.empty_like(v)
        vb = v.element_size()
        vp, vt = v.data_ptr(), vtmp.data_ptr()
    _ext.call_cpu("cme_cpu_radix_sort_kv_u64", k.data_ptr(), kt.data_ptr(), vp, vt, n, vb, num_bits,
                  min(64, max(1, int(key_bits))))
    out = _from_code64(k, dtype, descending, plain)
    return (out, v) if values is not None else out


def _onesweep(keys: torch.Tensor, values: torch.Tensor | None, key_bits: int):
    from .scan import _check_lookback

    n = keys.numel()
    dtype = keys.dtype
    _check_32bit_algo(dtype, "onesweep")
    if key_bits < 32 and dtype not in (torch.int32, torch.uint32):
        raise TypeError("key_bits < 32 needs non-negative integer keys")
    mode = 0 if key_bits < 32 else _MODES[dtype]
    bits = 32 if key_bits >= 32 else max(1, int(key_bits))
    k = keys.contiguous()
    out = torch.empty_like(k)
    tmp = torch.empty_like(k)
    vp = vo = vt = None
    if values is not None:
        if values.element_size() != 4 or values.numel() != n:
            raise TypeError("values: one 32-bit value per key")
        v = values.contiguous()
        vout, vtmp = torch.empty_like(v), torch.empty_like(v)
        vp, vo, vt = v.data_ptr(), vout.data_ptr(), vtmp.data_ptr()
    ws, epoch = _onesweep_ws(k)
    _check_lookback(k, before=True)
    _ext.call_hip("cme_radix_onesweep", k.data_ptr(), out.data_ptr(), tmp.data_ptr(), vp, vo, vt, n, mode, 0, bits,
                  ws.data_ptr(), epoch, _ext.stream_ptr(keys.device))
    _check_lookback(k)
    return (out, vout) if values is not None else out


def _workspace(dev: torch.device, nbytes: int) -> torch.Tensor:
    """Scratch of the reduce-then-scan sort (tile counts and totals; every
    call rewrites what it reads). Eager calls share one buffer per (device,
    stream): sorts on different streams never race on it. Under stream
    capture every call gets its own buffer from the graph's private pool, so
    a replay never writes into memory an eager call has since replaced and
    freed."""
    if torch.cuda.is_current_stream_capturing():
        return torch.empty(nbytes, dtype=torch.uint8, device=dev)
    key = (dev.index, _ext.stream_ptr(dev))
    t = _ws.get(key)
    if t is None or t.numel() < nbytes:
        t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        _ws[key] = t
    return t


_DT_SORT_DIM = {torch.uint32: 0, torch.int32: 1, torch.float32: 2, torch.uint64: 3, torch.int64: 4, torch.float64: 5}
_SORT_DIM_FORMS = ("flat", "row", "col")
_SORT_DIM_REGIMES = ("tile", "composed")
# bit patterns move through the tensor ops of the composed regime as signed integers
_SIGNED = {torch.uint32: torch.int32, torch.float32: torch.int32, torch.int32: torch.int32,
           torch.uint64: torch.int64, torch.float64: torch.int64, torch.int64: torch.int64}


def _sort_split(shape, dim: int) -> tuple[int, int, int]:
    from .scan import _split_dim

    try:
        return _split_dim(shape, dim)
    except (ValueError, IndexError) as e:
        raise type(e)(str(e).replace("scan:", "sort:")) from None


def _sort_dim_info(outer: int, n: int, inner: int, code: int, device: torch.device) -> list[int]:
    import ctypes

    info = (ctypes.c_longlong * 8)()
    with torch.cuda.device(device):
        _ext.call_hip("cme_sort_dim_info", outer, n, inner, code, ctypes.addressof(info))
    return [int(v) for v in info]


def _sort_dim_composed(x: torch.Tensor, outer: int, n: int, inner: int, descending: bool):
    """Lines longer than the tile kernel takes, from the 1-D sorts: a stable
    key-value sort of every key carrying its flat position, then a stable
    key-value sort of those positions by their line number (plain unsigned
    keys of ``bit_length(lines - 1)`` bits), which leaves every line's keys
    together and in sorted order; ``values`` is ``x`` gathered at that
    permutation, ``indices`` its position along the dimension. The line
    numbers, the gather and the index split are tensor ops."""
    total = outer * n * inner
    if total >= 1 << 32:
        raise ValueError("sort: dim= with lines above the tile kernel's length takes fewer than 2**32 elements")
    flat = x.reshape(-1)
    dev = x.device
    if total < 1 << 31:
        pos = torch.arange(total, dtype=torch.int32, device=dev)
    else:  # positions from 2**31 wrap into the sign bit and are unwrapped below
        pos = torch.arange(total, dtype=torch.int64, device=dev).to(torch.int32)
    perm = sort(flat, pos, descending=descending)[1]

    def wide(p):
        p = p.to(torch.int64)
        return p if total < 1 << 31 else p & 0xFFFFFFFF

    lines = outer * inner
    if lines > 1:
        p = wide(perm)
        line = ((p // (n * inner)) * inner + p % inner).to(torch.int32)  # lines < 2**32 / n
        perm = sort(line, perm, key_bits=max(1, (lines - 1).bit_length()))[1]
    p = wide(perm).view(outer, inner, n).transpose(1, 2).contiguous()  # [o, r, i]: the r-th key of line (o, i)
    values = flat.view(_SIGNED[x.dtype])[p].view(x.dtype).view(x.shape)
    indices = ((p // inner) % n).view(x.shape)
    return values, indices


def _sort_dim(x: torch.Tensor, dim: int, descending: bool):
    """``(values, indices)`` of the stable sort of ``x`` along ``dim``; see
    :func:`sort`. The tensor is seen as ``(outer, n, inner)`` like the scans
    along a dimension. GPU: ``csrc/hip/sort_dim.hip`` where a line fits the
    kernel's tile (:func:`sort_dim_launch_info`), :func:`_sort_dim_composed`
    above it; CPU: ``cme_cpu_sort_dim``. Neither synchronises."""
    outer, n, inner = _sort_split(x.shape, dim)
    if x.dtype not in _DT_SORT_DIM:
        raise TypeError(f"unsupported key dtype {x.dtype}")
    code = _DT_SORT_DIM[x.dtype]
    if not x.is_contiguous():
        x = x.contiguous()
    if x.numel() == 0 or n == 1:
        return x.clone(), torch.zeros(x.shape, dtype=torch.int64, device=x.device)
    if x.is_cuda and _sort_dim_info(outer, n, inner, code, x.device)[1] == 1:
        return _sort_dim_composed(x, outer, n, inner, descending)
    values = torch.empty_like(x)
    indices = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    if x.is_cuda:
        with torch.cuda.device(x.device):
            _ext.call_hip("cme_sort_dim", x.data_ptr(), values.data_ptr(), indices.data_ptr(), outer, n, inner, code,
                          int(descending), _ext.stream_ptr(x.device))
    else:
        _ext.call_cpu("cme_cpu_sort_dim", x.data_ptr(), values.data_ptr(), indices.data_ptr(), outer, n, inner, code,
                      int(descending))
    return values, indices


def _check_dim_args(values, algo, num_bits, key_bits) -> None:
    if values is not None or algo != "radix" or num_bits != 8 or key_bits is not None:
        raise TypeError("sort: with dim=, the returned indices replace carried values, and algo, num_bits and "
                        "key_bits stay at their defaults")


def sort_dim_launch_info(shape, dim: int, dtype: torch.dtype = torch.float32,
                         device: torch.device | str = "cuda") -> dict:
    """How ``sort(x, dim=dim)`` of a tensor of ``shape`` runs on ``device``:
    ``form`` ("flat": a single line, "row": along the last dimension, "col"),
    the shape split ``outer`` / ``n`` / ``inner``, ``regime`` ("tile": the LDS
    kernel, "composed": from the 1-D sorts), ``tile`` (the longest line the
    kernel takes), ``lines_per_tile``, ``passes`` (digit passes, the line pass
    included), ``workgroups``, ``items`` (slots per lane) and ``threads``.
    The CPU backend reports the shape split only."""
    outer, n, inner = _sort_split(tuple(shape), dim)
    if dtype not in _DT_SORT_DIM:
        raise TypeError(f"unsupported key dtype {dtype}")
    form = 0 if outer == 1 and inner == 1 else 1 if inner == 1 else 2
    d = {"form": _SORT_DIM_FORMS[form], "outer": outer, "n": n, "inner": inner, "regime": "tile", "tile": 0,
         "lines_per_tile": 0, "passes": 0, "workgroups": 0, "items": 0, "threads": 0}
    dev = torch.device(device)
    if dev.type != "cuda":
        return d
    info = _sort_dim_info(outer, n, inner, _DT_SORT_DIM[dtype], dev)
    d.update(form=_SORT_DIM_FORMS[info[0]], regime=_SORT_DIM_REGIMES[info[1]], tile=info[2], lines_per_tile=info[3],
             passes=info[4], workgroups=info[5], items=info[6], threads=info[7])
    return d


def sort(keys: torch.Tensor, values: torch.Tensor | None = None, algo: str = "radix", num_bits: int = 8,
         key_bits: int | None = None, descending: bool = False, dim: int | None = None):
    """Sort a 1-D tensor of int32 / uint32 / float32 or int64 / uint64 /
    float64 keys, optionally carrying one value per key: 4-byte values with
    32-bit keys, 4- or 8-byte values of any dtype (moved as raw bits) with
    64-bit keys. Stable; floats in IEEE total order (-NaN, -inf, ..., -0, +0,
    ..., +inf, +NaN); ``descending`` is the exact reverse with equal keys
    still in input order (``torch.sort(stable=True, descending=True)``).
    GPU algos: "radix" (reduce-then-scan, stable; "radix_rts" is an alias),
    "onesweep" (decoupled look-back, stable), "merge" (stable); 64-bit keys:
    "radix" only. CPU algos: "radix" (OpenMP, ``num_bits`` per pass),
    "radix_serial", "merge" (OpenMP tasks, keys only), the last two for
    32-bit keys. ``key_bits`` (None = the key width) below the key width
    (radix, non-negative integer keys below ``2**key_bits``) runs only the
    passes covering those bits -- a counting sort when ``key_bits <= 8``.
    Returns sorted keys (and values).

    With ``dim`` (one int, negative allowed): the sort of a tensor of any rank
    >= 1 along that dimension, as the named pair ``(values, indices)`` of
    ``torch.sort(keys, dim, descending, stable=True)``. Every line is sorted
    by the order above, stably in both directions; ``values`` (contiguous,
    ``keys``' shape and dtype) is ``keys`` gathered at ``indices`` (int64
    positions along ``dim``) bit for bit, NaN payloads and zero signs
    included. ``indices`` replaces carried values: ``values``, ``algo``,
    ``num_bits`` and ``key_bits`` must stay at their defaults (``TypeError``).
    GPU: lines that fit the tile of ``csrc/hip/sort_dim.hip`` are sorted in
    LDS, several short lines per workgroup (:func:`sort_dim_launch_info`);
    longer lines are composed from two 1-D key-value sorts and take fewer
    than 2**32 elements. CPU: ``cme_cpu_sort_dim``. No host synchronisation."""
    if dim is not None:
        _check_dim_args(values, algo, num_bits, key_bits)
        return SortWithIndices(*_sort_dim(keys, dim, descending))
    if keys.dim() != 1:
        raise ValueError("1-D keys expected")
    n = keys.numel()
    if n >= 1 << 32:
        raise ValueError("sort: fewer than 2**32 keys")
    dtype = keys.dtype
    if dtype in _MODES64:
        if algo not in ("radix", "radix_rts"):
            raise TypeError(f"algo={algo!r} sorts 32-bit keys only; {dtype} keys: algo='radix'")
        kb = 64 if key_bits is None else int(key_bits)
        if values is not None:
            _check_values64(values, n)
        if not keys.is_cuda and n > 0:
            return _cpu_sort64(keys, values, num_bits, kb, descending)
        if n <= 1:
            return (keys.clone(), values.clone()) if values is not None else keys.clone()
        return _rts64(keys, values, kb, descending)
    if descending:
        # 32-bit keys: the ascending sort of the order-reversed keys (equal
        # keys stay equal, so stability carries over), mapped back
        if dtype not in _MODES:
            raise TypeError(f"unsupported key dtype {dtype}")
        res = sort(_reverse32(keys), values, algo, num_bits, key_bits)
        return (_reverse32(res[0]), res[1]) if values is not None else _reverse32(res)
    key_bits = 32 if key_bits is None else int(key_bits)
    if keys.is_cuda and algo in ("radix", "radix_rts", "onesweep"):
        if n <= 1:
            return (keys.clone(), values.clone()) if values is not None else keys.clone()
        if algo == "onesweep":
            return _onesweep(keys, values, key_bits)
        return _rts(keys, values, key_bits)
    if keys.is_cuda and algo == "merge":
        return _merge(keys, values)
    if keys.is_cuda:
        raise ValueError(f"unknown GPU sort algo {algo!r}")
    if values is not None:
        if algo != "radix":
            raise NotImplementedError("CPU key-value sort: algo='radix'")
        if values.element_size() != 4 or values.numel() != n:
            raise TypeError("values: one 32-bit value per key")
        if key_bits < 32 and dtype not in (torch.int32, torch.uint32):
            raise TypeError("key_bits < 32 needs non-negative integer keys")
        k = keys.contiguous().clone().view(torch.uint32) if key_bits < 32 else _to_u32(keys.contiguous())
        v = values.contiguous().clone().view(torch.uint32)
        kt, vt = torch.empty_like(k), torch.empty_like(v)
        _ext.call_cpu("cme_cpu_radix_sort_kv_u32", k.data_ptr(), kt.data_ptr(), v.data_ptr(), vt.data_ptr(), n,
                      num_bits, min(32, max(1, int(key_bits))))
        out = k.view(dtype) if key_bits < 32 else _from_u32(k, dtype)
        return out, v.view(values.dtype)
    if algo == "merge":
        if dtype != torch.int32:
            raise TypeError("CPU merge sort takes int32 keys (the hw4 driver's type)")
        a = keys.clone()
        tmp = torch.empty_like(a)
        st = torch.zeros(1, dtype=torch.int32)
        _ext.call_cpu("cme_cpu_merge_sort_i32", a.data_ptr(), tmp.data_ptr(), n, 2048, 2048, st.data_ptr())
        return a if st.item() == 1 else tmp
    k = _to_u32(keys.contiguous())
    tmp = torch.empty_like(k)
    if algo == "radix":
        _ext.call_cpu("cme_cpu_radix_sort_u32", k.data_ptr(), tmp.data_ptr(), n, num_bits, 0)
    elif algo == "radix_serial":
        _ext.call_cpu("cme_cpu_radix_sort_serial_u32", k.data_ptr(), tmp.data_ptr(), n, num_bits)
    else:
        raise ValueError(algo)
    return _from_u32(k, dtype)


def argsort(keys: torch.Tensor, descending: bool = False, dim: int | None = None) -> torch.Tensor:
    """The stable sorting permutation of 1-D ``keys`` (any dtype :func:`sort`
    takes, GPU or CPU) as int64: ``keys[argsort(keys)]`` is ``sort(keys)``,
    and equal keys keep their input order, as ``torch.sort(keys, stable=True,
    descending=...).indices``. A key-value radix sort carrying 32-bit
    positions (the sort's limit is n < 2**32), widened once at the end.
    With ``dim``: the ``indices`` of ``sort(keys, dim=dim, descending=...)``,
    for a tensor of any rank >= 1."""
    if dim is not None:
        return _sort_dim(keys, dim, descending)[1]
    if keys.dim() != 1:
        raise ValueError("1-D keys expected")
    n = keys.numel()
    if n >= 1 << 32:
        raise ValueError("sort: fewer than 2**32 keys")
    if keys.dtype not in _MODES and keys.dtype not in _MODES64:
        raise TypeError(f"unsupported key dtype {keys.dtype}")
    if n < 1 << 31:
        pos = torch.arange(n, dtype=torch.int32, device=keys.device)
    else:  # positions from 2**31 wrap into the sign bit and are unwrapped below
        pos = torch.arange(n, dtype=torch.int64, device=keys.device).to(torch.int32)
    order = sort(keys, pos, descending=descending)[1].to(torch.int64)
    return order if n < 1 << 31 else order & 0xFFFFFFFF


def merge_sort_cpu(keys: torch.Tensor, sort_threshold: int, merge_threshold: int) -> tuple[torch.Tensor, int]:
    """The hw4 driver's merge sort with explicit thresholds; returns (sorted,
    status) where status 1/-1 says which ping-pong buffer held the result."""
    a = keys.clone()
    tmp = torch.empty_like(a)
    st = torch.zeros(1, dtype=torch.int32)
    _ext.call_cpu("cme_cpu_merge_sort_i32", a.data_ptr(), tmp.data_ptr(), a.numel(), sort_threshold,
                  merge_threshold, st.data_ptr())
    return (a if st.item() == 1 else tmp), int(st.item())
