// Launchers of the 8-byte-element scan / reduction family (scan64.hip), called
// from the dtype dispatch of cme_scan / cme_scan_rts / cme_reduce (scan.hip).
#pragma once
#include "cme213/common.h"

namespace cme {

// Elements per tile of the 64-bit look-back scan: 256 lanes x 16 rows of one
// 16-B vector (two elements). ops/scan.py mirrors it as TILE64. The
// reduce-then-scan works on half tiles (8 rows).
constexpr int kScan64LbRows = 16;
constexpr int kScan64Tile = 256 * 2 * kScan64LbRows;  // 8192 elements, 64 KB
constexpr int kRts64Rows = 8;
constexpr int kRts64Tile = 256 * 2 * kRts64Rows;  // 4096 elements, 32 KB
constexpr int kRts64Blocks = 1024;                // chunks (= partials) of the reduce-then-scan, at most

// dtype: 3 int64 (summed as uint64: wraps modulo 2^64), 4 float64.
int scan64_lookback(const void* in, void* out, long long n, int dtype, int exclusive, void* ws, hipStream_t s,
                    uint32_t epoch);
int scan64_rts(const void* in, void* out, long long n, int dtype, int exclusive, void* ws, hipStream_t s);
// op: 0 sum, 1 max, 2 min. part: >= 1024 * 8 bytes.
int reduce64(const void* in, long long n, int dtype, int op, void* part, void* out, hipStream_t s);

}  // namespace cme
