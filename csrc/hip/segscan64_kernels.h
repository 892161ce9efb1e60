// Kernel templates and launchers of the 8-byte segmented scan (entry points:
// segscan64.hip production, hip_tune/segscan64_tune.hip tuning arms).
#pragma once
#include "scan64.h"

#include "cme213/lookback.h"
#include "cme213/wave.h"

using namespace cme;

namespace {

using u64 = unsigned long long;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kRowElems = kWave * 2;  // 128: one 16-B vector per lane
constexpr int kRows = kSegScan64Rows;

// ------------------------------------------------------------ look-back
// One wave: lanes l < n inspect predecessor slot base - l of (a, inc): the
// segmented rule of lookback.h lb2_window over the two-granule slots of
// scan64.hip lb64_window. A walk ends at the nearest valid inc or flagged
// aggregate (its value is the running value at its end). `all_agg`: require
// EVERY lane's aggregate and fold them nearest-first up to the nearest
// flagged one into (*gsum, *gflag).
template <typename T>
__device__ __forceinline__ bool seg64_window(uint64_t* a, uint64_t* inc, int base, int n, bool virt0, bool all_agg,
                                             uint32_t epoch, T* sum, T* gsum, uint32_t* gflag, unsigned* timeout) {
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
        const bool aflag = aval && (sa & kStFlag);
        const bool ival = si != 0u || virt;
        const uint64_t tm = __ballot(ival || aflag);
        const int k = tm ? __builtin_ctzll(tm) : kWave;  // nearest terminating entry
        bool bad = lane < k && lane < n && !virt && !aval;
        if (all_agg) bad = bad || (act && !aval);
        if (!__any(bad)) {
            // lane k contributes its inclusive value (or its flagged aggregate)
            const T c = lane < k ? (aval ? lb64_val<T>(va) : T(0))
                                 : (lane == k && act ? lb64_val<T>(si != 0u ? vi : va) : T(0));
            *sum = wave_reduce(c);
            if (all_agg) {
                const uint64_t fm = __ballot(aflag);
                const int kf = fm ? __builtin_ctzll(fm) : kWave;
                *gsum = wave_reduce(act && lane <= kf ? lb64_val<T>(va) : T(0));
                *gflag = kf < kWave ? 1u : 0u;
            }
            return k < kWave;
        }
        if (lb_give_up(spins, timeout, lane)) {
            *sum = T(0);
            if (all_agg) *gsum = T(0), *gflag = 0u;
            return true;
        }
        __builtin_amdgcn_s_sleep(1);
    }
}

// Running value entering tile `tile` (its aggregate (tot, tot_flag) is already
// in agg[]; the caller ignores the value past the tile's first head);
// publishes inc[tile], and gagg / ginc for a group's last tile. One wave.
template <typename T>
__device__ T seg64_lookback(Lb64 w, int tile, int tiles, T tot, uint32_t tot_flag, unsigned* timeout, uint32_t epoch) {
    const int lane = lane_id();
    const int g = tile >> 6, j = tile & 63;
    const bool last = j == 63 || tile == tiles - 1;
    T prefix = T(0), gsum = T(0);
    uint32_t gflag = 0u;
    bool done = false;
    if (j > 0) done = seg64_window<T>(w.agg, w.inc, tile - 1, j, false, last, epoch, &prefix, &gsum, &gflag, timeout);
    if (last && lane == 0)  // unblock later groups first
        lb64_put(w.gagg + 2 * (long long)g, tot_flag ? tot : gsum + tot, epoch, (tot_flag | gflag) ? kStFlag : 0u);
    for (int gb = g - 1; !done && gb >= 0; gb -= kWave) {
        T s, gs;
        uint32_t gf;
        done = seg64_window<T>(w.gagg, w.ginc, gb, kWave, true, false, epoch, &s, &gs, &gf, timeout);
        prefix = prefix + s;
    }
    if (lane == 0) {
        const T incl = tot_flag ? tot : prefix + tot;
        const uint32_t fl = tot_flag ? kStFlag : 0u;  // informational only: inc always ends a walk
        lb64_put(w.inc + 2 * (long long)tile, incl, epoch, fl);
        if (last) lb64_put(w.ginc + 2 * (long long)g, incl, epoch, fl);
    }
    return prefix;
}

// ------------------------------------------------------------ wave level
template <typename T>
__device__ __forceinline__ void seg_combine(uint32_t& f, T& v, uint32_t fs, T vs) {
    v = f ? v : vs + v;
    f = f | fs;
}

// Wave inclusive segmented scan by DPP (one 0/1 flag per lane); 64-bit values
// move as two 32-bit halves.
template <typename T>
__device__ __forceinline__ T wave_segscan(T v, uint32_t f, uint32_t* f_out) {
#define SEG_STEP(CTRL, RM)                           \
    {                                                \
        const T vs = dpp_move<CTRL, RM>(T(0), v);    \
        const uint32_t fs = dpp_move<CTRL, RM>(0u, f); \
        seg_combine(f, v, fs, vs);                   \
    }
    SEG_STEP(kDppRowShr1, 0xf)
    SEG_STEP(kDppRowShr2, 0xf)
    SEG_STEP(kDppRowShr4, 0xf)
    SEG_STEP(kDppRowShr8, 0xf)
    SEG_STEP(kDppRowBcast15, 0xa)
    SEG_STEP(kDppRowBcast31, 0xc)
#undef SEG_STEP
    *f_out = f;
    return v;
}

// Raw inputs of one lane's row (loads only: decoding and the fused multiply
// happen at use, so a prefetch never waits on memory).
template <typename T>
struct Seg64Raw {
    Vec2<T> a, x;
    uint32_t fw;  // MODE 0: the two flag bytes; MODE 1: the bitmask word
};

typedef uint16_t u16_unaligned __attribute__((aligned(1)));

// MODE 0: one uint8 per element (any non-zero byte is a head); MODE 1: int32
// bitmask words, bit i % 32 of word i / 32. i is even, so both of a lane's
// flags lie in one word.
template <typename T, int MODE, bool FUSED_MUL>
__device__ __forceinline__ Seg64Raw<T> seg64_load(const T* in, const T* __restrict__ xmul,
                                                  const void* __restrict__ flags, long long i, long long n) {
    Seg64Raw<T> r;
    r.a = load_v2(in, i, n, T(0));
    if constexpr (FUSED_MUL) r.x = load_v2(xmul, i, n, T(0));
    if constexpr (MODE == 0) {
        const uint8_t* fp = (const uint8_t*)flags;
        if (i + 1 < n)
            r.fw = *reinterpret_cast<const u16_unaligned*>(fp + i);
        else
            r.fw = i < n ? fp[i] : 0u;
    } else {
        r.fw = i < n ? ((const uint32_t*)flags)[i >> 5] : 0u;
    }
    return r;
}

// ------------------------------------------------------------ the kernel
// Persistent: block b scans tiles b, b + G, ... in order (G = grid size,
// co-resident), so every tile's predecessors are owned by running blocks.
// PREFETCH issues the next tile's loads before the look-back wait (the raw
// registers are dead once the tile is decoded). `in` and `out` are not
// restrict: out may be in (every lane loads exactly the elements it later
// stores). NTS: non-temporal output stores, for an output written once.
//
// MULTI: `iters` in-place steps a <- segscan(a * xmul) in ONE launch (in ==
// out), as scan_kernels.h segscan_kernel does it: block b owns the same tiles
// in every step and each lane re-reads exactly the elements it stored, so a
// step's input needs no synchronisation across blocks; step i has its own
// descriptor set (`desc0 + i * desc_stride`, epoch `epoch0 + i`), because a
// block that owns only early tiles may run several steps ahead. Every wait
// depends only on earlier (step, tile) pairs of a co-resident grid, which
// every block processes in that order, so the smallest unfinished pair can
// always proceed.
template <typename T, int MODE, bool FUSED_MUL, int ROWS, bool PREFETCH, bool NTS, bool MULTI = false>
__global__ __launch_bounds__(kThreads) void segscan64_kernel(const T* in, const T* __restrict__ xmul, T* out,
                                                             const void* __restrict__ flags, long long n,
                                                             uint64_t* desc0, int tiles, unsigned* timeout,
                                                             uint32_t epoch0, int iters, long long desc_stride) {
    constexpr int kTile = kThreads * 2 * ROWS;
    constexpr int kWaveElems = kWave * 2 * ROWS;
    __shared__ T s_wv[2][kWaves];
    __shared__ uint32_t s_wf[2][kWaves];
    __shared__ T s_prefix[2];
    const int lane = lane_id();
    const int wid = threadIdx.x / kWave;
    int parity = 0;
    Seg64Raw<T> raw[ROWS];
    auto load_tile = [&](long long tile) {
        const long long b = tile * kTile + wid * kWaveElems + lane * 2;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) raw[k] = seg64_load<T, MODE, FUSED_MUL>(in, xmul, flags, b + k * kRowElems, n);
    };
    if ((int)blockIdx.x < tiles) load_tile(blockIdx.x);
    const int nit = MULTI ? iters : 1;
    for (int it = 0; it < nit; ++it) {
    const Lb64 views = lb64_views(desc0 + (MULTI ? it * desc_stride : 0), tiles);
    const uint32_t epoch = epoch0 + (uint32_t)it;
    for (long long tile = blockIdx.x; tile < tiles; tile += gridDim.x, parity ^= 1) {
        const long long base = tile * kTile + wid * kWaveElems + lane * 2;
        T val0[ROWS], val1[ROWS];  // in-lane inclusive segmented scan of the row's two elements
        uint32_t meta[ROWS];       // bit 0 / 1: a head at or before element 0 / 1 of the lane; bit 2: one in earlier lanes or rows
        T ex_v[ROWS];
        T run_v = T(0);       // running (segment-aware) value across the rows of this wave
        uint32_t run_f = 0u;  // any head so far in this wave
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            T v0 = raw[k].a.x, v1 = raw[k].a.y;
            if constexpr (FUSED_MUL) {
                v0 = v0 * raw[k].x.x;
                v1 = v1 * raw[k].x.y;
            }
            uint32_t g0, g1;
            if constexpr (MODE == 0) {
                g0 = (raw[k].fw & 0xffu) ? 1u : 0u;
                g1 = (raw[k].fw & 0xff00u) ? 1u : 0u;
            } else {
                const uint32_t f2 = raw[k].fw >> ((base + k * kRowElems) & 31);
                g0 = f2 & 1u;
                g1 = (f2 >> 1) & 1u;
            }
            v1 = g1 ? v1 : v0 + v1;
            const uint32_t c1 = g0 | g1;
            val0[k] = v0;
            val1[k] = v1;
            // wave scan of the lane totals (value v1, flag: any head in the lane)
            uint32_t lf;
            const T inc = wave_segscan(v1, c1, &lf);
            // exclusive: shift by one lane; the carry of the earlier rows
            // applies unless a head lies in earlier lanes of this row
            const T e_v = dpp_move<kDppWaveShr1>(T(0), inc);
            const uint32_t e_f = dpp_move<kDppWaveShr1>(0u, lf);
            const T row_v = wave_readlane(inc, kWave - 1);
            const uint32_t row_f = (uint32_t)__builtin_amdgcn_readlane((int)lf, kWave - 1);
            ex_v[k] = e_f ? e_v : run_v + e_v;
            meta[k] = g0 | (c1 << 1) | ((e_f | run_f) << 2);
            run_v = row_f ? row_v : run_v + row_v;
            run_f = run_f | row_f;
        }
        if (lane == 0) {
            s_wv[parity][wid] = run_v;
            s_wf[parity][wid] = run_f;
        }
        lds_bcast_sync();
        // wave prefix (segment-aware) and tile aggregate
        T wpre_v = T(0), tot_v = T(0);
        uint32_t wpre_f = 0u, tot_f = 0u;
#pragma unroll
        for (int w = 0; w < kWaves; ++w) {
            const T tv = s_wv[parity][w];
            const uint32_t tf = s_wf[parity][w];
            if (w < wid) {
                wpre_v = tf ? tv : wpre_v + tv;
                wpre_f |= tf;
            }
            tot_v = tf ? tv : tot_v + tv;
            tot_f |= tf;
        }
        const uint32_t hf = tot_f ? (uint32_t)kStFlag : 0u;
        if (wid == 0 && lane == 0) lb64_put(views.agg + 2 * tile, tot_v, epoch, hf);
        const long long next = tile + gridDim.x;
        if (PREFETCH && next < tiles) load_tile(next);
        if (wid == 0) {
            const T pre = seg64_lookback<T>(views, (int)tile, tiles, tot_v, hf, timeout, epoch);
            if (lane == 0) s_prefix[parity] = pre;
        }
        lds_bcast_sync();
        // carry into this wave: the tile's prefix unless a head precedes in the tile
        const T wcarry = wpre_f ? wpre_v : s_prefix[parity] + wpre_v;
#pragma unroll
        for (int k = 0; k < ROWS; ++k) {
            const T c = (meta[k] & 4u) ? ex_v[k] : wcarry + ex_v[k];
            Vec2<T> r;
            r.x = (meta[k] & 1u) ? val0[k] : c + val0[k];
            r.y = (meta[k] & 2u) ? val1[k] : c + val1[k];
            store_v2<NTS>(out, base + k * kRowElems, n, r);
        }
        if (!PREFETCH && next < tiles) {
            load_tile(next);
        } else if (MULTI && next >= tiles && it + 1 < nit) {
            // the next step starts at this block's first tile, which this lane
            // stored earlier (the tile just stored, if the block owns only one)
            load_tile(blockIdx.x);
        }
    }  // tile loop
    }  // step loop
}

inline long long seg64_tiles(long long n, int rows) {
    const long long tile = kThreads * 2LL * rows;
    return (n + tile - 1) / tile;
}

template <typename T, int MODE, bool FUSED_MUL, int ROWS, bool PREFETCH, bool NTS>
int seg64_grid_cap() {
    static int bpc = persistent_blocks_per_cu(segscan64_kernel<T, MODE, FUSED_MUL, ROWS, PREFETCH, NTS>, kThreads);
    return device_cu_count() * bpc;
}

// One launch (one step) on descriptors the caller zeroed; `tiles` is
// seg64_tiles(n, ROWS).
template <typename T, int MODE, bool FUSED_MUL, int ROWS, bool PREFETCH, bool NTS>
int seg64_launch(const T* in, const T* xmul, T* out, const void* flags, long long n, uint64_t* desc, int tiles,
                 uint32_t epoch, hipStream_t s) {
    const int cap = seg64_grid_cap<T, MODE, FUSED_MUL, ROWS, PREFETCH, NTS>();
    const int grid = tiles < cap ? tiles : cap;
    unsigned* timeout = lb_host_timeout();
    if (!timeout) return (int)hipErrorOutOfMemory;
    hipLaunchKernelGGL((segscan64_kernel<T, MODE, FUSED_MUL, ROWS, PREFETCH, NTS>), dim3(grid), dim3(kThreads), 0, s,
                       in, xmul, out, flags, n, desc, tiles, timeout, epoch, 1, 0LL);
    return (int)hipGetLastError();
}

// Final-project run in double: `iters` in-place steps a <- segscan(a * xx)
// with bitmask heads and plain (cached) stores, since a step's output is the
// next step's input. MULTI: up to kSpmvScan64Steps steps per persistent
// launch, one 256-B aligned descriptor set per step, zeroed by one memset per
// launch; otherwise one memset, then one launch per step with epoch step + 1.
constexpr int kSpmvScan64Steps = 64;
template <int ROWS, bool PREFETCH, bool MULTI>
int spmv_scan64_launch(double* a, const double* xx, const uint32_t* flags, long long n, int iters, void* ws,
                       hipStream_t s) {
    const long long nt = seg64_tiles(n, ROWS);
    if (nt >= (1ll << 30) || iters >= (1 << 24)) return (int)hipErrorInvalidValue;  // epochs are 24-bit
    const int tiles = (int)nt;
    uint64_t* desc = lb_descriptors(ws);
    const size_t set_bytes = lb64_ws_bytes(tiles);
    if constexpr (MULTI) {
        static int bpc = persistent_blocks_per_cu(segscan64_kernel<double, 1, true, ROWS, PREFETCH, false, true>, kThreads);
        const int cap = device_cu_count() * bpc;
        const int grid = tiles < cap ? tiles : cap;
        unsigned* timeout = lb_host_timeout();
        if (!timeout) return (int)hipErrorOutOfMemory;
        const long long stride = (long long)((set_bytes + 255) / 256 * 256 / sizeof(uint64_t));
        for (int it0 = 0; it0 < iters; it0 += kSpmvScan64Steps) {
            const int k = iters - it0 < kSpmvScan64Steps ? iters - it0 : kSpmvScan64Steps;
            CME_TRY(hipMemsetAsync(ws, 0, 16 + k * stride * sizeof(uint64_t), s));
            hipLaunchKernelGGL((segscan64_kernel<double, 1, true, ROWS, PREFETCH, false, true>), dim3(grid),
                               dim3(kThreads), 0, s, a, xx, a, flags, n, desc, tiles, timeout, 1u, k, stride);
            CME_TRY(hipGetLastError());
        }
    } else {
        CME_TRY(hipMemsetAsync(ws, 0, set_bytes, s));
        for (int it = 0; it < iters; ++it) {
            const int rc = seg64_launch<double, 1, true, ROWS, PREFETCH, false>(a, xx, a, flags, n, desc, tiles,
                                                                                (uint32_t)(it + 1), s);
            if (rc) return rc;
        }
    }
    return 0;
}

// Bytes spmv_scan64_launch needs for n elements, whatever the arm: one 256-B
// aligned descriptor set of the finest tiling (2 rows: 1024 elements per
// tile) per step of a launch.
inline long long spmv_scan64_ws_bytes(long long n) {
    const long long set = (long long)lb64_ws_bytes(seg64_tiles(n > 0 ? n : 1, 2));
    return kSpmvScan64Steps * ((set + 255) / 256 * 256) + 256;
}

}  // namespace
