// Launchers of the 8-byte-element scan / reduction family (scan64.hip), called
// from the dtype dispatch of cme_scan / cme_scan_rts / cme_reduce (scan.hip),
// and the pieces scan64.hip shares with the 8-byte segmented scan
// (segscan64.hip): the 16-B two-element vector accesses and the two-granule
// look-back descriptor slots.
#pragma once
#include "cme213/common.h"
#include "cme213/lookback.h"

namespace cme {

// Elements per tile of the 64-bit look-back scan: 256 lanes x 16 rows of one
// 16-B vector (two elements). ops/scan.py mirrors it as TILE64. The
// reduce-then-scan works on half tiles (8 rows).
constexpr int kScan64LbRows = 16;
constexpr int kScan64Tile = 256 * 2 * kScan64LbRows;  // 8192 elements, 64 KB
constexpr int kRts64Rows = 8;
constexpr int kRts64Tile = 256 * 2 * kRts64Rows;  // 4096 elements, 32 KB
constexpr int kRts64Blocks = 1024;                // chunks (= partials) of the reduce-then-scan, at most

// Segmented scan of 8-byte elements (segscan64.hip): 256 lanes x 8 rows of one
// 16-B vector. ops/scan.py mirrors the tile as SEGTILE64.
constexpr int kSegScan64Rows = 8;
constexpr int kSegScan64Tile = 256 * 2 * kSegScan64Rows;  // 4096 elements, 32 KB per operand

// dtype: 3 int64 (summed as uint64: wraps modulo 2^64), 4 float64.
int scan64_lookback(const void* in, void* out, long long n, int dtype, int exclusive, void* ws, hipStream_t s,
                    uint32_t epoch);
int scan64_rts(const void* in, void* out, long long n, int dtype, int exclusive, void* ws, hipStream_t s);
// Max / min prefix scans (wave.h OpCumMax / OpCumMin; op 1 max, 2 min): int64
// compares as long long. scan64_op_info: see cme_scan_op_info (scan.hip).
int scan64_lookback_op(const void* in, void* out, long long n, int dtype, int op, int exclusive, void* ws,
                       hipStream_t s, uint32_t epoch);
int scan64_rts_op(const void* in, void* out, long long n, int dtype, int op, int exclusive, void* ws, hipStream_t s);
int scan64_op_info(long long n, int dtype, int op, int exclusive, long long* info);
// op: 0 sum, 1 max, 2 min. part: >= 1024 * 8 bytes.
int reduce64(const void* in, long long n, int dtype, int op, void* part, void* out, hipStream_t s);

template <typename T>
struct Vec2 {
    T x, y;
};

// 16-B vector of two elements that is only 8-byte aligned: x[1:] of a 64-bit
// tensor is a legal operand. Global dwordx4 accesses need dword alignment
// only, so the compiler still emits one 16-B load / store per lane.
template <typename T>
struct V2 {
    typedef T aligned16 __attribute__((ext_vector_type(2)));
    typedef aligned16 type __attribute__((aligned(8)));
};

template <typename T>
__device__ __forceinline__ Vec2<T> load_v2(const T* p, long long i, long long n, T id) {
    Vec2<T> r;
    if (i + 1 < n) {
        const typename V2<T>::aligned16 v = *reinterpret_cast<const typename V2<T>::type*>(p + i);
        r.x = v.x;
        r.y = v.y;
    } else {
        r.x = i < n ? p[i] : id;
        r.y = id;
    }
    return r;
}

template <bool NTS = false, typename T>
__device__ __forceinline__ void store_v2(T* p, long long i, long long n, const Vec2<T>& r) {
    if (i + 1 < n) {
        const typename V2<T>::aligned16 v = {r.x, r.y};
        if constexpr (NTS)  // write-once output: stream it past the caches
            __builtin_nontemporal_store(v, reinterpret_cast<typename V2<T>::type*>(p + i));
        else
            *reinterpret_cast<typename V2<T>::type*>(p + i) = v;
    } else if (i < n) {
        p[i] = r.x;
    }
}

// ------------------------------------------------- 64-bit look-back descriptors
// A slot is two naturally aligned 8-byte granules, each {(epoch << 8) | status
// : 32, 32 value bits}: the low half first, then the high half. Each granule is
// ONE relaxed agent-scope atomic store and is read by relaxed agent-scope
// atomic loads (lookback.h lb_publish / lb_poll); nothing relies on a 16-byte
// access being single-copy atomic. Slots are WRITE-ONCE per epoch (the
// two-level layout: agg, inc, gagg, ginc), so a half that carries the
// launch's epoch holds its final bits, and a slot is valid exactly when both
// halves carry the launch's epoch and the same non-zero status (kStFlag
// included, where the segmented scan sets it); until then the waiter keeps
// polling.
struct Lb64 {
    uint64_t *agg, *inc, *gagg, *ginc;
};
inline size_t lb64_ws_bytes(long long tiles) { return 16 + 32 * (size_t)tiles + 32 * (size_t)((tiles + 63) / 64); }
__host__ __device__ inline Lb64 lb64_views(uint64_t* desc, long long tiles) {
    const long long groups = (tiles + 63) / 64;
    return Lb64{desc, desc + 2 * tiles, desc + 4 * tiles, desc + 4 * tiles + 2 * groups};
}

// `flag`: 0, or kStFlag for an aggregate with a segment head inside
template <typename T>
__device__ __forceinline__ void lb64_put(uint64_t* slot, T v, uint32_t epoch, uint32_t flag = 0u) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, v);
    lb_publish(slot, kStAggregate | flag, (uint32_t)bits, epoch);
    lb_publish(slot + 1, kStAggregate | flag, (uint32_t)(bits >> 32), epoch);
}

// status of a slot for this epoch (0: not published yet, or half published)
__device__ __forceinline__ uint32_t lb64_get(uint64_t* slot, uint32_t epoch, uint64_t* bits) {
    const uint64_t lo = lb_poll(slot), hi = lb_poll(slot + 1);
    const uint32_t wl = (uint32_t)(lo >> 32), wh = (uint32_t)(hi >> 32);
    *bits = (hi << 32) | (uint32_t)lo;
    return (wl == wh && (wl >> 8) == epoch) ? (wl & 0xffu) : 0u;
}

template <typename T>
__device__ __forceinline__ T lb64_val(uint64_t bits) {
    return __builtin_bit_cast(T, bits);
}

}  // namespace cme
