// Launch plan of the batched scans along one dimension (scan_dim.hip): a
// contiguous tensor seen as (outer, n, inner), element (o, i, j) at
// (o*n + i)*inner + j, scanned along i. Shared by the launcher and the
// launch-info query, so what ops/scan.py reports is what runs.
#pragma once
#include "cme213/common.h"

namespace cme {

constexpr int kScanDimThreads = 256;
// Row form (inner == 1): a lane moves 16-B vectors, four per tile step, so a
// wave covers 64 * 4 * (16 / esize) contiguous elements and a workgroup of
// four waves four times that.
constexpr int kScanDimRowVecs = 4;
// Column form (inner > 1): rows of loads in flight per lane.
constexpr int kScanDimColUnroll = 8;
// Column form: a chunk along n is at least this many rows.
constexpr int kScanDimMinChunkRows = 32;

struct ScanDimPlan {
    int form;          // 0 flat (outer == inner == 1: the 1-D path of ops/scan.py), 1 row, 2 column
    int waves;         // row form: waves that share a line (4: a workgroup per line, 1: a wave per line)
    int vector;        // elements per lane access (1: scalar lanes, column form only)
    int chunks;        // K: chunks along n (1: single pass)
    long long chunk;   // elements of a line per chunk
    long long tile;    // elements of a line per workgroup (or wave) step
    long long grid;    // workgroups of the scan pass
    long long ws_bytes;
};

// esize: 4 or 8. Reads the scan_dim_chunks / scan_dim_maxblocks knobs.
ScanDimPlan scan_dim_plan(long long outer, long long n, long long inner, int esize, bool in_aligned16);

}  // namespace cme
