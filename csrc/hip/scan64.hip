// Scan and reduction of 8-byte elements (int64, float64), written for wave64.
//
//  * scan64_lookback  single-pass decoupled look-back, persistent co-resident
//                     grid, two-level look-back with TWO 8-byte granules per
//                     descriptor slot (a granule carries 32 value bits).
//  * scan64_rts       deterministic three-kernel reduce-then-scan.
//  * reduce64         two-pass sum / max / min.
//
// Lanes move 16-B vectors of two elements; a tile is 16 rows of them per lane
// in the look-back (8192 elements, 64 KB) and 8 rows in the reduce-then-scan.
// int64 is summed as unsigned long long, so sums wrap
// modulo 2^64 (signed overflow would be undefined); max / min compare as long
// long, and so do the max / min prefix scans (wave.h OpCumMax / OpCumMin: the
// same kernels with the operator as a template parameter, called as
// op(earlier, later)). The 32-bit family (scan_kernels.h) and its tuned
// constants are not touched.
#include "scan64.h"

#include "cme213/lookback.h"
#include "cme213/wave.h"

using namespace cme;

namespace {

using u64 = unsigned long long;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
// reduce-then-scan tile: 8 rows of one 16-B vector per lane
constexpr int kRows = kRts64Rows;
constexpr int kTile = kRts64Tile;
constexpr int kWaveElems = kWave * 2 * kRows;  // 1024: a wave's contiguous share of a tile
constexpr int kRowElems = kWave * 2;           // 128: one 16-B vector per lane
// Look-back tile: 16 rows (8192 elements, 64 KB: the bytes of the 32-bit
// production tile) with two tiles of loads in flight behind the look-back.
// 252-256 VGPRs, no scratch, one resident workgroup per CU. Of {8, 12, 16}
// rows x {1, 2} tiles in flight this arm measured fastest at 2^25 and 2^27
// for both dtypes (profiles/scan64_r8.md): the scan is bound by the look-back
// hand-off, and larger tiles mean fewer hand-offs per byte.
constexpr int kLbRows = kScan64LbRows;

// Vec2 / load_v2 / store_v2 and the two-granule descriptor slots (Lb64,
// lb64_put / lb64_get) are in scan64.h, shared with segscan64.hip.

// One wave: lanes l < n inspect predecessor slot base - l of (a, inc); see
// lookback.h lb2_window (this is its unsegmented form over two-granule slots).
// The lanes hold the predecessors latest first: an ordered operator is folded
// by its mirror image, and empty slots hold its identity.
template <typename T, typename Op = OpAdd>
__device__ __forceinline__ bool lb64_window(uint64_t* a, uint64_t* inc, int base, int n, bool virt0, bool all_agg,
                                            uint32_t epoch, T* sum, T* gsum, unsigned* timeout) {
    using Fold = typename LatestFirst<Op>::type;
    const T id = Op::template identity<T>();
    const int lane = lane_id();
    for (unsigned spins = 0;; ++spins) {
        const int idx = base - lane;
        const bool act = lane < n && idx >= 0;
        const bool virt = lane < n && idx < 0 && virt0;
        uint64_t va = 0, vi = 0;
        uint32_t sa = 0u, si = 0u;
        if (act) {
            sa = lb64_get(a + 2 * (long long)idx, epoch, &va);
            si = lb64_get(inc + 2 * (long long)idx, epoch, &vi);
        }
        const bool aval = sa != 0u;
        const bool ival = si != 0u || virt;
        const uint64_t tm = __ballot(ival);
        const int k = tm ? __builtin_ctzll(tm) : kWave;  // nearest inclusive entry
        bool bad = lane < k && lane < n && !virt && !aval;
        if (all_agg) bad = bad || (act && !aval);
        if (!__any(bad)) {
            const T c = lane < k ? (aval ? lb64_val<T>(va) : id)
                                 : (lane == k && act ? lb64_val<T>(si != 0u ? vi : va) : id);
            *sum = wave_reduce<Fold>(c);
            if (all_agg) *gsum = wave_reduce<Fold>(act ? lb64_val<T>(va) : id);
            return k < kWave;
        }
        if (lb_give_up(spins, timeout, lane)) {
            *sum = id;
            if (all_agg) *gsum = id;
            return true;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Exclusive prefix of tile `tile` (its aggregate `tot` is already in agg[]);
// publishes inc[tile], and gagg / ginc for a group's last tile. One wave.
template <typename T, typename Op = OpAdd>
__device__ T lb64_lookback(Lb64 w, int tile, int tiles, T tot, unsigned* timeout, uint32_t epoch) {
    const Op op;
    const int lane = lane_id();
    const int g = tile >> 6, j = tile & 63;
    const bool last = j == 63 || tile == tiles - 1;
    T prefix = Op::template identity<T>(), gsum = prefix;
    bool done = false;
    if (j > 0) done = lb64_window<T, Op>(w.agg, w.inc, tile - 1, j, false, last, epoch, &prefix, &gsum, timeout);
    if (last && lane == 0) lb64_put(w.gagg + 2 * (long long)g, op(gsum, tot), epoch);  // unblock later groups first
    for (int gb = g - 1; !done && gb >= 0; gb -= kWave) {
        T s, gs;
        done = lb64_window<T, Op>(w.gagg, w.ginc, gb, kWave, true, false, epoch, &s, &gs, timeout);
        prefix = op(s, prefix);  // s: the earlier groups
    }
    if (lane == 0) {
        lb64_put(w.inc + 2 * (long long)tile, op(prefix, tot), epoch);
        if (last) lb64_put(w.ginc + 2 * (long long)g, op(prefix, tot), epoch);
    }
    return prefix;
}

// in-lane scan of each row's two elements, wave scans of the lane totals and
// the serial carry across the rows of one wave; leaves in v the lane-local
// terms and in ex the per-row exclusive prefix inside the wave. Returns the
// wave's total.
template <bool EXCLUSIVE, typename Op = OpAdd, typename T, int ROWS>
__device__ __forceinline__ T wave_tile_scan(Vec2<T> (&v)[ROWS], T (&ex)[ROWS]) {
    const Op op;
    const T id = Op::template identity<T>();
    T run = id;
#pragma unroll
    for (int k = 0; k < ROWS; ++k) {
        const T a = v[k].x, b = op(a, v[k].y);
        T wt;
        const T e = wave_exclusive_scan<Op>(b, &wt);
        ex[k] = op(run, e);
        run = op(run, wt);
        if (EXCLUSIVE) {
            v[k].y = a;
            v[k].x = id;
        } else {
            v[k].y = b;
        }
    }
    return run;
}

// ------------------------------------------------------------ look-back scan
// Persistent: block b scans tiles b, b + G, b + 2G, ... in order (G = grid
// size, co-resident), so every tile's predecessors are owned by running
// blocks. Two tiles of loads stay in flight behind the look-back (tile + G in
// vn, tile + 2G in vn2) and the output is stored non-temporally, as in the
// 32-bit production kernel. `in` and `out` are not restrict: out may be in
// (every lane loads exactly the elements it later stores).
template <typename T, bool EXCLUSIVE, int ROWS = kLbRows, typename Op = OpAdd>
__global__ __launch_bounds__(kThreads) void scan64_lookback_kernel(const T* in, T* out, long long n, uint64_t* desc,
                                                                   int tiles, unsigned* timeout, uint32_t epoch) {
    const Op op;
    const T id = Op::template identity<T>();
    constexpr int kRows = ROWS;
    constexpr int kTile = kThreads * 2 * ROWS;
    constexpr int kWaveElems = kWave * 2 * ROWS;
    __shared__ T s_wtot[2][kWaves];
    __shared__ T s_prefix[2];
    const int lane = lane_id();
    const int wid = threadIdx.x / kWave;
    const Lb64 views = lb64_views(desc, tiles);
    int parity = 0;
    Vec2<T> v[kRows], vn[kRows];
    auto load_tile = [&](long long tile, Vec2<T>(&dst)[kRows]) {
        const long long b = tile * kTile + wid * kWaveElems + lane * 2;
#pragma unroll
        for (int k = 0; k < kRows; ++k) dst[k] = load_v2(in, b + k * kRowElems, n, id);
    };
    if ((int)blockIdx.x < tiles) {
        load_tile(blockIdx.x, v);
        if ((long long)blockIdx.x + gridDim.x < tiles) load_tile((long long)blockIdx.x + gridDim.x, vn);
    }
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1) {
        T ex[kRows];
        const T run = wave_tile_scan<EXCLUSIVE, Op>(v, ex);
        if (lane == 0) s_wtot[parity][wid] = run;
        lds_bcast_sync();
        T wpre = id, tot = id;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const T t = s_wtot[parity][w];
            if (w < wid) wpre = op(wpre, t);
            tot = op(tot, t);
        }
        if (wid == 0 && lane == 0) lb64_put(views.agg + 2 * tile, tot, epoch);
        Vec2<T> vn2[kRows];
        const long long pf_tile = tile + 2LL * gridDim.x;
        if (pf_tile < tiles) load_tile(pf_tile, vn2);
        if (wid == 0) {
            const T pre = lb64_lookback<T, Op>(views, (int)tile, tiles, tot, timeout, epoch);
            if (lane == 0) s_prefix[parity] = pre;
        }
        lds_bcast_sync();
        const T p = op(s_prefix[parity], wpre);
        const long long base = tile * kTile + wid * kWaveElems + lane * 2;
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const T q = op(p, ex[k]);
            store_v2<true>(out, base + k * kRowElems, n, Vec2<T>{op(q, v[k].x), op(q, v[k].y)});
        }
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            v[k] = vn[k];
            vn[k] = vn2[k];
        }
    }
}

template <typename T, int ROWS, typename Op = OpAdd>
int lookback_grid_cap(int exclusive) {
    static int bpc_e = persistent_blocks_per_cu(scan64_lookback_kernel<T, true, ROWS, Op>, kThreads);
    static int bpc_i = persistent_blocks_per_cu(scan64_lookback_kernel<T, false, ROWS, Op>, kThreads);
    return device_cu_count() * (exclusive ? bpc_e : bpc_i);
}

// epoch 0: zero the descriptors first (one memset node, so a captured graph
// re-zeroes them at every replay); epoch e > 0: the caller zeroed `ws` once
// and gives every launch a new epoch.
template <typename T, typename Op = OpAdd, int ROWS = kLbRows>
int launch_lookback(const T* in, T* out, long long n, int exclusive, void* ws, hipStream_t s, uint32_t epoch) {
    if (n <= 0) return 0;
    constexpr long long kTile = kThreads * 2LL * ROWS;
    const long long nt = (n + kTile - 1) / kTile;
    if (nt >= (1ll << 30)) return (int)hipErrorInvalidValue;
    const int tiles = (int)nt;
    const int cap = lookback_grid_cap<T, ROWS, Op>(exclusive);
    const int grid = tiles < cap ? tiles : cap;
    unsigned* timeout = lb_host_timeout();
    if (!timeout) return (int)hipErrorOutOfMemory;
    uint64_t* desc = lb_descriptors(ws);
    if (epoch >= (1u << 24)) return (int)hipErrorInvalidValue;
    if (epoch == 0) CME_TRY(hipMemsetAsync(ws, 0, lb64_ws_bytes(tiles), s));
    if (exclusive)
        hipLaunchKernelGGL((scan64_lookback_kernel<T, true, ROWS, Op>), dim3(grid), dim3(kThreads), 0, s, in, out, n,
                           desc, tiles, timeout, epoch);
    else
        hipLaunchKernelGGL((scan64_lookback_kernel<T, false, ROWS, Op>), dim3(grid), dim3(kThreads), 0, s, in, out, n,
                           desc, tiles, timeout, epoch);
    CME_LAUNCH_STATUS();
}

// ------------------------------------------------------------ reduce-then-scan
// K1 reduces contiguous chunks of whole tiles, K2 scans the (at most 1024)
// chunk totals in one block, K3 rescans each chunk tile by tile with the carry
// in a register and the next tile prefetched. 24 B/element of traffic; the
// summation tree depends on n alone, so float64 results are bitwise
// reproducible.
// An ordered operator must meet the elements in element order, which the sum's
// per-thread accumulators do not: there each wave folds a contiguous quarter of
// the chunk, one wave reduction per 128-element row, and the four wave totals
// are combined in wave order (scan_kernels.h rts_reduce_kernel).
template <typename T, typename Op = OpAdd>
__global__ __launch_bounds__(kThreads) void rts64_reduce_kernel(const T* __restrict__ in, long long n, long long chunk,
                                                                T* __restrict__ part) {
    __shared__ T lds[kWaves];
    const Op op;
    const T id = Op::template identity<T>();
    const long long b0 = (long long)blockIdx.x * chunk;
    const long long b1 = b0 + chunk < n ? b0 + chunk : n;
    if constexpr (Op::kOrdered) {
        const int lane = lane_id();
        const int wid = threadIdx.x / kWave;
        const long long quarter = chunk / kWaves;  // chunk: whole tiles of 4096
        const long long w0 = b0 + wid * quarter;
        const long long w1 = w0 + quarter < b1 ? w0 + quarter : b1;
        T run = id;
        for (long long r0 = w0; r0 < w1; r0 += kWaveElems) {  // 8 rows (loads of 16 B per lane) in flight
            Vec2<T> v[kRows];
#pragma unroll
            for (int k = 0; k < kRows; ++k) v[k] = load_v2(in, r0 + k * kRowElems + lane * 2, w1, id);
#pragma unroll
            for (int k = 0; k < kRows; ++k) run = op(run, wave_reduce<Op>(op(v[k].x, v[k].y)));
        }
        if (lane == 0) lds[wid] = run;
        lds_bcast_sync();
        if (threadIdx.x == 0) {
            T r = lds[0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) r = op(r, lds[w]);
            part[blockIdx.x] = r;
        }
    } else {
        T acc = id;
        // one tile (8 loads of 16 B per lane) in flight per iteration
        for (long long t0 = b0; t0 < b1; t0 += kTile) {
            Vec2<T> v[kRows];
#pragma unroll
            for (int k = 0; k < kRows; ++k) v[k] = load_v2(in, t0 + (k * kThreads + (int)threadIdx.x) * 2, b1, id);
#pragma unroll
            for (int k = 0; k < kRows; ++k) acc = op(acc, op(v[k].x, v[k].y));
        }
        const T r = block_reduce<kWaves>(acc, lds, op);
        if (threadIdx.x == 0) part[blockIdx.x] = r;
    }
}

// exclusive scan of m <= 1024 partials in place, one block of 1024 threads,
// one partial per thread: the only LDS is the block scan's 16 wave totals of
// 8 bytes (the 32-bit kernel's 8192-value staging would be 69.6 KB here and is
// not needed for at most 1024 values).
template <typename T, typename Op = OpAdd>
__global__ __launch_bounds__(1024) void rts64_partials_kernel(T* part, int m) {
    __shared__ T lds[16];
    const int t = threadIdx.x;
    const T v = t < m ? part[t] : Op::template identity<T>();
    T tot;
    const T e = block_exclusive_scan<16>(v, lds, tot, Op());
    if (t < m) part[t] = e;
}

template <typename T, bool EXCLUSIVE, typename Op = OpAdd>
__global__ __launch_bounds__(kThreads) void rts64_scan_kernel(const T* in, T* out, long long n, long long chunk,
                                                              const T* __restrict__ part) {
    const Op op;
    const T id = Op::template identity<T>();
    __shared__ T s_wtot[2][kWaves];
    const int lane = lane_id();
    const int wid = threadIdx.x / kWave;
    const long long b0 = (long long)blockIdx.x * chunk;
    const long long b1 = b0 + chunk < n ? b0 + chunk : n;
    T carry = part[blockIdx.x];
    Vec2<T> v[kRows], nv[kRows];
    auto load_tile = [&](long long t0, Vec2<T>(&dst)[kRows]) {
#pragma unroll
        for (int k = 0; k < kRows; ++k) dst[k] = load_v2(in, t0 + wid * kWaveElems + k * kRowElems + lane * 2, b1, id);
    };
    if (b0 < b1) load_tile(b0, v);
    int parity = 0;
    for (long long t0 = b0; t0 < b1; t0 += kTile, parity ^= 1) {
        if (t0 + kTile < b1) load_tile(t0 + kTile, nv);
        T ex[kRows];
        const T run = wave_tile_scan<EXCLUSIVE, Op>(v, ex);
        if (lane == 0) s_wtot[parity][wid] = run;
        lds_bcast_sync();
        T wpre = id, tot = id;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const T t = s_wtot[parity][w];
            if (w < wid) wpre = op(wpre, t);
            tot = op(tot, t);
        }
        const T p = op(carry, wpre);
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const T q = op(p, ex[k]);
            store_v2(out, t0 + wid * kWaveElems + k * kRowElems + lane * 2, b1,
                     Vec2<T>{op(q, v[k].x), op(q, v[k].y)});
        }
        carry = op(carry, tot);
#pragma unroll
        for (int k = 0; k < kRows; ++k) v[k] = nv[k];
    }
}

struct RtsShape {
    int blocks;
    long long chunk;  // elements per block: whole tiles
};
RtsShape rts_shape(long long n) {
    const long long tiles = (n + kTile - 1) / kTile;
    int blocks = tiles < kRts64Blocks ? (int)tiles : kRts64Blocks;
    const long long chunk = ((tiles + blocks - 1) / blocks) * kTile;
    blocks = (int)((n + chunk - 1) / chunk);
    return RtsShape{blocks, chunk};
}

template <typename T, typename Op = OpAdd>
int launch_rts64(const T* in, T* out, long long n, int exclusive, void* ws, hipStream_t s) {
    if (n <= 0) return 0;
    const RtsShape sh = rts_shape(n);
    T* part = (T*)ws;
    hipLaunchKernelGGL((rts64_reduce_kernel<T, Op>), dim3(sh.blocks), dim3(kThreads), 0, s, in, n, sh.chunk, part);
    hipLaunchKernelGGL((rts64_partials_kernel<T, Op>), dim3(1), dim3(1024), 0, s, part, sh.blocks);
    if (exclusive)
        hipLaunchKernelGGL((rts64_scan_kernel<T, true, Op>), dim3(sh.blocks), dim3(kThreads), 0, s, in, out, n,
                           sh.chunk, (const T*)part);
    else
        hipLaunchKernelGGL((rts64_scan_kernel<T, false, Op>), dim3(sh.blocks), dim3(kThreads), 0, s, in, out, n,
                           sh.chunk,
                           (const T*)part);
    CME_LAUNCH_STATUS();
}

// ------------------------------------------------------------ reduction
constexpr int kReduce64Grid = 1024;

template <typename T, typename Op>
__global__ __launch_bounds__(kThreads) void reduce64_partial_kernel(const T* __restrict__ in, long long n,
                                                                    T* __restrict__ part, Op op) {
    __shared__ T lds[kWaves];
    const T id = Op::template identity<T>();
    T acc = id;
    const long long stride = (long long)gridDim.x * kThreads * 2;
    long long i = ((long long)blockIdx.x * kThreads + threadIdx.x) * 2;
    // eight 16-B loads in flight per lane on a grid of 1024: of 2 / 4 / 8 loads
    // on 512 ... 4096 blocks the fastest (profiles/scan64_r8.md)
    constexpr int U = 8;
    for (; i + (U - 1) * stride < n; i += U * stride) {
        Vec2<T> v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) v[u] = load_v2(in, i + u * stride, n, id);
#pragma unroll
        for (int u = 0; u < U; ++u) acc = op(acc, op(v[u].x, v[u].y));
    }
    for (; i < n; i += stride) {
        const Vec2<T> v = load_v2(in, i, n, id);
        acc = op(acc, op(v.x, v.y));
    }
    const T r = block_reduce<kWaves>(acc, lds, op);
    if (threadIdx.x == 0) part[blockIdx.x] = r;
}

template <typename T, typename Op>
__global__ __launch_bounds__(1024) void reduce64_final_kernel(const T* __restrict__ part, int m, T* __restrict__ out,
                                                              Op op) {
    __shared__ T lds[16];
    T acc = Op::template identity<T>();
    for (int i = threadIdx.x; i < m; i += 1024) acc = op(acc, part[i]);
    const T r = block_reduce<16>(acc, lds, op);
    if (threadIdx.x == 0) *out = r;
}

template <typename T, typename Op>
int launch_reduce64(const void* in, long long n, void* part, void* out, hipStream_t s) {
    hipLaunchKernelGGL((reduce64_partial_kernel<T, Op>), dim3(kReduce64Grid), dim3(kThreads), 0, s, (const T*)in, n,
                       (T*)part, Op());
    hipLaunchKernelGGL((reduce64_final_kernel<T, Op>), dim3(1), dim3(1024), 0, s, (const T*)part, kReduce64Grid,
                       (T*)out, Op());
    CME_LAUNCH_STATUS();
}

}  // namespace

int cme::scan64_lookback(const void* in, void* out, long long n, int dtype, int exclusive, void* ws, hipStream_t s,
                         uint32_t epoch) {
    if (dtype == 3) return launch_lookback<u64>((const u64*)in, (u64*)out, n, exclusive, ws, s, epoch);
    if (dtype == 4) return launch_lookback<double>((const double*)in, (double*)out, n, exclusive, ws, s, epoch);
    return (int)hipErrorInvalidValue;
}

int cme::scan64_rts(const void* in, void* out, long long n, int dtype, int exclusive, void* ws, hipStream_t s) {
    if (dtype == 3) return launch_rts64<u64>((const u64*)in, (u64*)out, n, exclusive, ws, s);
    if (dtype == 4) return launch_rts64<double>((const double*)in, (double*)out, n, exclusive, ws, s);
    return (int)hipErrorInvalidValue;
}

int cme::scan64_lookback_op(const void* in, void* out, long long n, int dtype, int op, int exclusive, void* ws,
                            hipStream_t s, uint32_t epoch) {
    using ll = long long;
    switch (dtype * 4 + op) {
        case 13: return launch_lookback<ll, OpCumMax>((const ll*)in, (ll*)out, n, exclusive, ws, s, epoch);
        case 14: return launch_lookback<ll, OpCumMin>((const ll*)in, (ll*)out, n, exclusive, ws, s, epoch);
        case 17: return launch_lookback<double, OpCumMax>((const double*)in, (double*)out, n, exclusive, ws, s, epoch);
        case 18: return launch_lookback<double, OpCumMin>((const double*)in, (double*)out, n, exclusive, ws, s, epoch);
        default: return (int)hipErrorInvalidValue;
    }
}

int cme::scan64_rts_op(const void* in, void* out, long long n, int dtype, int op, int exclusive, void* ws,
                       hipStream_t s) {
    using ll = long long;
    switch (dtype * 4 + op) {
        case 13: return launch_rts64<ll, OpCumMax>((const ll*)in, (ll*)out, n, exclusive, ws, s);
        case 14: return launch_rts64<ll, OpCumMin>((const ll*)in, (ll*)out, n, exclusive, ws, s);
        case 17: return launch_rts64<double, OpCumMax>((const double*)in, (double*)out, n, exclusive, ws, s);
        case 18: return launch_rts64<double, OpCumMin>((const double*)in, (double*)out, n, exclusive, ws, s);
        default: return (int)hipErrorInvalidValue;
    }
}

int cme::scan64_op_info(long long n, int dtype, int op, int exclusive, long long* info) {
    int cap;
    switch (dtype * 4 + op) {
        case 12: cap = lookback_grid_cap<u64, kLbRows>(exclusive); break;
        case 13: cap = lookback_grid_cap<long long, kLbRows, OpCumMax>(exclusive); break;
        case 14: cap = lookback_grid_cap<long long, kLbRows, OpCumMin>(exclusive); break;
        case 16: cap = lookback_grid_cap<double, kLbRows>(exclusive); break;
        case 17: cap = lookback_grid_cap<double, kLbRows, OpCumMax>(exclusive); break;
        case 18: cap = lookback_grid_cap<double, kLbRows, OpCumMin>(exclusive); break;
        default: return (int)hipErrorInvalidValue;
    }
    const long long tiles = n > 0 ? (n + kScan64Tile - 1) / kScan64Tile : 0;
    const RtsShape sh = rts_shape(n > 0 ? n : 1);
    info[0] = kScan64Tile;
    info[1] = tiles;
    info[2] = tiles < cap ? tiles : cap;
    info[3] = cap / device_cu_count();
    info[4] = n > 0 ? sh.blocks : 0;
    info[5] = sh.chunk / kTile;
    info[6] = kTile;
    info[7] = (long long)lb64_ws_bytes(tiles);
    return 0;
}

int cme::reduce64(const void* in, long long n, int dtype, int op, void* part, void* out, hipStream_t s) {
    if (n <= 0 || op < 0 || op > 2) return (int)hipErrorInvalidValue;
    if (dtype == 3) {
        if (op == 0) return launch_reduce64<u64, OpAdd>(in, n, part, out, s);
        if (op == 1) return launch_reduce64<long long, OpMax>(in, n, part, out, s);
        return launch_reduce64<long long, OpMin>(in, n, part, out, s);
    }
    if (dtype == 4) {
        if (op == 0) return launch_reduce64<double, OpAdd>(in, n, part, out, s);
        if (op == 1) return launch_reduce64<double, OpMax>(in, n, part, out, s);
        return launch_reduce64<double, OpMin>(in, n, part, out, s);
    }
    return (int)hipErrorInvalidValue;
}

// How a 64-bit scan of n elements is launched on the current device:
// info[0] look-back tile elements, [1] look-back tiles, [2] look-back
// workgroups (the co-resident grid), [3] reduce-then-scan chunks, [4] its tiles
// per chunk, [5] look-back workspace bytes, [6] reduce-then-scan tile elements.
CME_EXPORT int cme_scan64_info(long long n, long long* info) {
    const long long tiles = (n + kScan64Tile - 1) / kScan64Tile;
    const int cap = lookback_grid_cap<u64, kLbRows>(0);
    const RtsShape sh = rts_shape(n > 0 ? n : 1);
    info[0] = kScan64Tile;
    info[1] = tiles;
    info[2] = tiles < cap ? tiles : cap;
    info[3] = n > 0 ? sh.blocks : 0;
    info[4] = sh.chunk / kTile;
    info[5] = (long long)lb64_ws_bytes(tiles);
    info[6] = kTile;
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(scan64_lookback_i64, 256, scan64_lookback_kernel<u64, true>);
CME_REGISTER_KERNEL(scan64_lookback_f64, 256, scan64_lookback_kernel<double, true>);
CME_REGISTER_KERNEL(scan64_rts_reduce_f64, 256, rts64_reduce_kernel<double>);
CME_REGISTER_KERNEL(scan64_rts_scan_f64, 256, rts64_scan_kernel<double, true>);
CME_REGISTER_KERNEL(scan64_rts_scan_i64, 256, rts64_scan_kernel<u64, true>);
CME_REGISTER_KERNEL(reduce64_sum_f64, 256, reduce64_partial_kernel<double, OpAdd>);
CME_REGISTER_KERNEL(scan64_max_lookback_i64, 256, scan64_lookback_kernel<long long, true, kLbRows, OpCumMax>);
CME_REGISTER_KERNEL(scan64_max_lookback_f64, 256, scan64_lookback_kernel<double, true, kLbRows, OpCumMax>);
CME_REGISTER_KERNEL(scan64_max_rts_scan_i64, 256, rts64_scan_kernel<long long, true, OpCumMax>);
CME_REGISTER_KERNEL(scan64_max_rts_scan_f64, 256, rts64_scan_kernel<double, true, OpCumMax>);
