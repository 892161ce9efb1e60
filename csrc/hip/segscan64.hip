// Inclusive segmented sum scan of 8-byte elements (int64, float64), written
// for wave64: the segmented form of scan64.hip's look-back over two-granule
// descriptor slots (scan64.h), with scan_kernels.h segscan_kernel's flag
// loading (uint8 per element or bitmask words) and fused multiply. Kernels:
// segscan64_kernels.h.
//
// Lanes move 16-B vectors of two elements; a tile is 8 rows of them per lane
// (4096 elements, 32 KB per operand). int64 is summed as unsigned long long,
// so sums wrap modulo 2^64. Aggregates combine as (f, v) . (f', v') =
// (f | f', f' ? v' : v + v'); the status byte of a slot carries kStFlag next
// to kStAggregate, and a flagged aggregate ends a look-back walk. The sign of
// a float64 zero result is not specified (0.0 is the identity of the lane
// shifts, as in the float32 kernel).
#include "segscan64_kernels.h"

namespace {

// Production shape of the one-shot scan (profiles/segscan64_r9.md): 8 rows,
// the next tile's loads in flight behind the look-back. Of {4, 8, 16} rows x
// {no, one} tile in flight it is the fastest arm without heads (a walk then
// ends only at an inclusive prefix: 0.60 ms at 2^27, 4 rows 0.76-0.82) and
// within 10 % of the fastest with them (0.53-0.54 ms, 4 rows 0.48-0.50).
constexpr bool kPrefetch = true;

template <typename T>
int seg64_dispatch(const void* in, const void* xmul, void* out, const void* flags, int flag_mode, long long n,
                   uint64_t* desc, int tiles, uint32_t epoch, hipStream_t s) {
    const T *i = (const T*)in, *x = (const T*)xmul;
    T* o = (T*)out;
    if (flag_mode == 0)
        return x ? seg64_launch<T, 0, true, kRows, kPrefetch, true>(i, x, o, flags, n, desc, tiles, epoch, s)
                 : seg64_launch<T, 0, false, kRows, kPrefetch, true>(i, x, o, flags, n, desc, tiles, epoch, s);
    return x ? seg64_launch<T, 1, true, kRows, kPrefetch, true>(i, x, o, flags, n, desc, tiles, epoch, s)
             : seg64_launch<T, 1, false, kRows, kPrefetch, true>(i, x, o, flags, n, desc, tiles, epoch, s);
}

}  // namespace

// Segmented inclusive scan of int64 (dtype 3) or float64 (dtype 4).
// flag_mode 0: uint8 per element; 1: bitmask words. xmul != null fuses
// in[i] * xmul[i]. ws: >= cme_segscan64_info's byte count, an array (and an
// epoch count) apart from the 32-bit scans' and scan64's. epoch 0: the
// descriptors are zeroed here first (one memset node, so a captured graph
// re-zeroes them at every replay); epoch e > 0: the caller zeroed `ws` once
// and gives every launch a new epoch.
CME_EXPORT int cme_segscan64(const void* in, const void* xmul, void* out, const void* flags, int flag_mode,
                             long long n, int dtype, void* ws, unsigned epoch, void* stream) {
    hipStream_t s = as_stream(stream);
    if (n <= 0) return 0;
    if (dtype != 3 && dtype != 4) return (int)hipErrorInvalidValue;
    const long long nt = seg64_tiles(n, kRows);
    if (nt >= (1ll << 30) || epoch >= (1u << 24)) return (int)hipErrorInvalidValue;
    const int tiles = (int)nt;
    if (epoch == 0) CME_TRY(hipMemsetAsync(ws, 0, lb64_ws_bytes(tiles), s));
    uint64_t* desc = lb_descriptors(ws);
    return dtype == 3 ? seg64_dispatch<u64>(in, xmul, out, flags, flag_mode, n, desc, tiles, epoch, s)
                      : seg64_dispatch<double>(in, xmul, out, flags, flag_mode, n, desc, tiles, epoch, s);
}

// Final-project driver in double: `iters` in-place steps a <- segscan(a * xx)
// (bitmask heads), no host synchronisation inside: all steps in one
// persistent launch per 64 steps, one descriptor set per step
// (segscan64_kernels.h MULTI). On the 15 benchmark shapes the fused launch
// beat one launch per step of the same tile shape everywhere, 1.26x
// (rail4284) to 1.7x (cop20k_A, webbase-1M), and 4 rows without prefetch was
// the fastest of the 12 arms (rows 2 / 4 / 8 x prefetch x fused) on 13; the
// two smallest (37 035 and 958 936 elements) want 2 rows, i.e. more blocks on
// the look-back chain (profiles/segscan64_r9.md). The one-launch-per-step
// form is kept as a tuning arm (hip_tune/segscan64_tune.hip).
CME_EXPORT int cme_spmv_scan_run64(double* a, const double* xx, const uint32_t* flags, long long n, int iters,
                                   void* ws, void* stream) {
    if (n <= 0 || iters <= 0) return 0;
    hipStream_t s = as_stream(stream);
    if (n <= (1ll << 20)) return spmv_scan64_launch<2, false, true>(a, xx, flags, n, iters, ws, s);
    return spmv_scan64_launch<4, false, true>(a, xx, flags, n, iters, ws, s);
}

CME_EXPORT int cme_spmv_scan64_ws_bytes(long long n, long long* bytes) {
    *bytes = spmv_scan64_ws_bytes(n);
    return 0;
}

// How a 64-bit segmented scan of n elements is launched on the current
// device: info[0] tile elements, [1] tiles, [2] workgroups (the co-resident
// grid of the float64 bitmask fused kernel; lighter instantiations may hold
// more), [3] its blocks per CU, [4] workspace bytes.
CME_EXPORT int cme_segscan64_info(long long n, long long* info) {
    const long long tiles = n > 0 ? seg64_tiles(n, kRows) : 0;
    const int cap = seg64_grid_cap<double, 1, true, kRows, kPrefetch, true>();
    info[0] = kSegScan64Tile;
    info[1] = tiles;
    info[2] = tiles < cap ? tiles : cap;
    info[3] = cap / device_cu_count();
    info[4] = (long long)lb64_ws_bytes(tiles);
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(segscan64_f64_bitmask_fused, 256, segscan64_kernel<double, 1, true, kRows, kPrefetch, true>);
CME_REGISTER_KERNEL(segscan64_f64_run_rows4, 256, segscan64_kernel<double, 1, true, 4, false, false, true>);
CME_REGISTER_KERNEL(segscan64_f64_run_rows2, 256, segscan64_kernel<double, 1, true, 2, false, false, true>);
CME_REGISTER_KERNEL(segscan64_i64_bytes, 256, segscan64_kernel<u64, 0, false, kRows, kPrefetch, true>);
