// Tuning arms of the 8-byte segmented scan and the float64 SpMV-scan run
// (libcme213_tune.so only, `make TUNE=1`); production entry points are in
// csrc/hip/segscan64.hip. benchmarks/bench_segscan64.py --arms times them.
#include "../hip/segscan64_kernels.h"

namespace {
// bitmask heads, no multiply; the descriptors are zeroed by a memset per call
template <typename T, int ROWS, bool PF>
int seg64_tune_launch(const void* in, void* out, const void* flags, long long n, void* ws, hipStream_t s) {
    const long long nt = seg64_tiles(n, ROWS);
    if (nt >= (1ll << 30)) return (int)hipErrorInvalidValue;
    CME_TRY(hipMemsetAsync(ws, 0, lb64_ws_bytes(nt), s));
    return seg64_launch<T, 1, false, ROWS, PF, true>((const T*)in, (const T*)nullptr, (T*)out, flags, n,
                                                     lb_descriptors(ws), (int)nt, 1u, s);
}
}  // namespace

// rows 4 / 8 / 16 vectors per lane x pf (the next tile's loads issued before
// the look-back wait); dtype 3 int64, 4 float64. ws: cme_spmv_scan64_ws_bytes.
CME_EXPORT int cme_segscan64_tune(const void* in, void* out, const void* flags, long long n, int dtype, int rows,
                                  int pf, void* ws, void* stream) {
    hipStream_t s = as_stream(stream);
    if (n <= 0) return 0;
#define ARM(T, R)                                                          \
    return pf ? seg64_tune_launch<T, R, true>(in, out, flags, n, ws, s)    \
              : seg64_tune_launch<T, R, false>(in, out, flags, n, ws, s)
    if (dtype == 3) {
        if (rows == 4) ARM(u64, 4);
        if (rows == 8) ARM(u64, 8);
        if (rows == 16) ARM(u64, 16);
    } else if (dtype == 4) {
        if (rows == 4) ARM(double, 4);
        if (rows == 8) ARM(double, 8);
        if (rows == 16) ARM(double, 16);
    }
#undef ARM
    return (int)hipErrorInvalidValue;
}

// rows 2 / 4 / 8 x mode: bit 0 prefetch, bit 1 all steps in one persistent
// launch per 64 steps (one descriptor set per step).
CME_EXPORT int cme_spmv_scan_run64_tune(double* a, const double* xx, const uint32_t* flags, long long n, int iters,
                                        void* ws, int rows, int mode, void* stream) {
    if (n <= 0 || iters <= 0) return 0;
    hipStream_t s = as_stream(stream);
#define SPT(R)                                                                           \
    switch (mode & 3) {                                                                  \
        case 0: return spmv_scan64_launch<R, false, false>(a, xx, flags, n, iters, ws, s); \
        case 1: return spmv_scan64_launch<R, true, false>(a, xx, flags, n, iters, ws, s);  \
        case 2: return spmv_scan64_launch<R, false, true>(a, xx, flags, n, iters, ws, s);  \
        default: return spmv_scan64_launch<R, true, true>(a, xx, flags, n, iters, ws, s);  \
    }
    if (rows == 2) SPT(2)
    if (rows == 4) SPT(4)
    if (rows == 8) SPT(8)
#undef SPT
    return (int)hipErrorInvalidValue;
}
