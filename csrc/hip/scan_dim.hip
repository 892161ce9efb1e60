// Scans along one dimension of a contiguous tensor seen as (outer, n, inner):
// element (o, i, j) at (o*n + i)*inner + j, scanned along i. Sum, running max
// and running min (wave.h OpAdd / OpCumMax / OpCumMin, always called as
// op(earlier, later)) of float32, int32, uint32, int64 and float64.
//
//  * row form (inner == 1): outer contiguous lines of n elements. A workgroup
//    (or, for short lines, a single wave) walks its line in tiles of 16-B lane
//    vectors with a running carry and grid-strides over the lines.
//  * column form (inner > 1): lanes run along the flattened column index
//    o*inner + j, keep their columns' running values in registers and walk
//    down i with kScanDimColUnroll rows of loads in flight. No LDS, no barrier.
//
// Parallelism along n, where the lines alone cannot fill the device, is
// chunked reduce-then-scan: pass 1 writes the total of every (line, chunk) to
// the workspace, a small kernel scans those totals exclusively along the
// chunks, pass 2 rescans every chunk seeded with its carry. No kernel here
// waits for another workgroup, and the summation tree of a float sum is fixed
// by the launch shape (and the 16-byte phase of the operand's address), never
// by the order in which workgroups finish. All index arithmetic is 64-bit.
//
// `in` and `out` are not restrict: out may be in. Every lane loads exactly the
// elements it later stores, before it stores them.
#include "scan_dim.h"

#include "cme213/tuning.h"
#include "cme213/wave.h"

using namespace cme;

namespace {

using u64 = unsigned long long;
using ll = long long;
constexpr int kThreads = kScanDimThreads;
constexpr int kWaves = kThreads / kWave;
constexpr int kR = kScanDimRowVecs;
constexpr int kU = kScanDimColUnroll;

// V = 16 / sizeof(T) elements: `tight` is 16-byte aligned, `loose` aligned to
// the element only (a global dwordx4 access needs no more).
template <typename T, int V>
struct LaneVec {
    typedef T tight __attribute__((ext_vector_type(V)));
    typedef tight loose __attribute__((aligned(sizeof(T))));
};

// ------------------------------------------------------------------ row form
// NW waves share a line: NW == 4 is a workgroup per (line, chunk) item, NW == 1
// a wave per item (no LDS, no barrier). A tile step covers NW * 64 * V * kR
// elements; the walk starts at the 16-byte boundary at or below the chunk's
// first element, so every whole vector is an aligned 16-B load, and the
// elements outside [lo, hi) -- the scalar head and tail -- read as the
// operator's identity and are not stored.
// mode 0: scan (carry from ws when K > 1); mode 1: totals only, ws[item].
template <typename T, typename Op, int NW>
__global__ __launch_bounds__(kThreads) void scan_rows_kernel(const T* in, T* out, ll outer, ll n, int K, ll chunk,
                                                             T* ws, int exclusive, int mode) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int kRowElems = kWave * V;
    constexpr int kWaveElems = kRowElems * kR;
    constexpr int kTile = NW * kWaveElems;
    using Tight = typename LaneVec<T, V>::tight;
    using Loose = typename LaneVec<T, V>::loose;
    const Op op;
    const T id = Op::template identity<T>();
    __shared__ T s_wtot[2][kWaves];
    const int lane = lane_id();
    const int wid = threadIdx.x / kWave;
    const ll items = outer * K;
    ll item = NW == 1 ? (ll)blockIdx.x * kWaves + wid : (ll)blockIdx.x;
    const ll stride = NW == 1 ? (ll)gridDim.x * kWaves : (ll)gridDim.x;
    const int woff = (NW == 1 ? 0 : wid * kWaveElems) + lane * V;
    int parity = 0;
    for (; item < items; item += stride) {
        const ll r = K == 1 ? item : item / K;  // (a 64-bit division costs as much as a short row)
        const ll k = K == 1 ? 0 : item % K;
        const ll end = (r + 1) * n;
        ll lo = r * n + k * chunk;
        if (lo > end) lo = end;
        const ll hi = lo + chunk < end ? lo + chunk : end;
        T carry = (K > 1 && mode == 0) ? ws[item] : id;
        const ll phase = (ll)((reinterpret_cast<uintptr_t>(in + lo) / sizeof(T)) % V);
        T v[kR][V], nv[kR][V];
        auto load_tile = [&](ll t0, T(&dst)[kR][V]) {
#pragma unroll
            for (int q = 0; q < kR; ++q) {
                const ll i = t0 + woff + q * kRowElems;
                if (i >= lo && i + V <= hi) {
                    const Tight x = *reinterpret_cast<const Tight*>(in + i);
#pragma unroll
                    for (int e = 0; e < V; ++e) dst[q][e] = x[e];
                } else {
#pragma unroll
                    for (int e = 0; e < V; ++e) dst[q][e] = (i + e >= lo && i + e < hi) ? in[i + e] : id;
                }
            }
        };
        ll t0 = lo - phase;
        if (t0 < hi) load_tile(t0, v);
        for (; t0 < hi; t0 += kTile) {
            if (t0 + kTile < hi) load_tile(t0 + kTile, nv);
            // in-lane scan of each vector, wave scan of the lane totals, serial
            // carry across the kR vectors of the wave
            T ex[kR];
            T run = id;
#pragma unroll
            for (int q = 0; q < kR; ++q) {
#pragma unroll
                for (int e = 1; e < V; ++e) v[q][e] = op(v[q][e - 1], v[q][e]);
                T wt;
                const T x = wave_exclusive_scan<Op>(v[q][V - 1], &wt);
                ex[q] = op(run, x);
                run = op(run, wt);
            }
            T p = carry, tot = run;
            if constexpr (NW > 1) {
                if (lane == 0) s_wtot[parity][wid] = run;
                lds_bcast_sync();
                T wpre = id;
                tot = id;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const T t = s_wtot[parity][w];
                    if (w < wid) wpre = op(wpre, t);
                    tot = op(tot, t);
                }
                p = op(carry, wpre);
                parity ^= 1;
            }
            if (mode == 0) {
#pragma unroll
                for (int q = 0; q < kR; ++q) {
                    const ll i = t0 + woff + q * kRowElems;
                    const T base = op(p, ex[q]);
                    T y[V];
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        if (exclusive) y[e] = e == 0 ? base : op(base, v[q][e == 0 ? 0 : e - 1]);
                        else y[e] = op(base, v[q][e]);
                    }
                    if (i >= lo && i + V <= hi) {
                        Tight x;
#pragma unroll
                        for (int e = 0; e < V; ++e) x[e] = y[e];
                        *reinterpret_cast<Loose*>(out + i) = x;
                    } else {
#pragma unroll
                        for (int e = 0; e < V; ++e)
                            if (i + e >= lo && i + e < hi) out[i + e] = y[e];
                    }
                }
            }
            carry = op(carry, tot);
#pragma unroll
            for (int q = 0; q < kR; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) v[q][e] = nv[q][e];
        }
        if (mode == 1 && lane == 0 && (NW == 1 || wid == 0)) ws[item] = carry;
    }
}

// --------------------------------------------------------------- column form
// One lane per group of VEC adjacent columns and per chunk: thread
// t = k * G + g, so neighbouring lanes read neighbouring addresses. VEC is
// 16 / sizeof(T) only where inner % VEC == 0 and both operands are 16-byte
// aligned, and 1 otherwise (scan_dim_plan picks it). mode as scan_rows_kernel; the totals are ws[(o*K + k)*inner + j].
template <typename T, typename Op, int VEC>
__global__ __launch_bounds__(kThreads) void scan_cols_kernel(const T* in, T* out, ll outer, ll n, ll inner, int K,
                                                             ll chunk, T* ws, int exclusive, int mode) {
    using Tight = typename LaneVec<T, VEC>::tight;
    const Op op;
    const T id = Op::template identity<T>();
    const ll G = outer * inner / VEC;
    const ll total = G * K;
    const bool narrow = outer * inner < (1ll << 31);  // column indices fit 32 bits
    for (ll t = (ll)blockIdx.x * kThreads + threadIdx.x; t < total; t += (ll)gridDim.x * kThreads) {
        // the common cases without a 64-bit division, which costs as much as
        // several rows of a short column
        const ll k = K == 1 ? 0 : t / G;
        const ll g = t - k * G;
        const ll c = g * VEC;
        const ll o = outer == 1 ? 0 : narrow ? (ll)((unsigned)c / (unsigned)inner) : c / inner;
        const ll j = c - o * inner;
        ll i0 = k * chunk;
        if (i0 > n) i0 = n;
        const ll i1 = i0 + chunk < n ? i0 + chunk : n;
        T* const w = ws + (o * K + k) * inner + j;
        T run[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) run[e] = (K > 1 && mode == 0) ? w[e] : id;
        const ll off = (o * n + i0) * inner + j;
        const T* p = in + off;
        T* q = out + off;
        auto load = [&](const T* a, T(&x)[VEC]) {
            if constexpr (VEC == 1) {
                x[0] = *a;
            } else {
                const Tight y = *reinterpret_cast<const Tight*>(a);
#pragma unroll
                for (int e = 0; e < VEC; ++e) x[e] = y[e];
            }
        };
        auto step = [&](T(&x)[VEC], T* a) {
            T y[VEC];
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                const T inc = op(run[e], x[e]);
                y[e] = exclusive ? run[e] : inc;
                run[e] = inc;
            }
            if (mode != 0) return;
            if constexpr (VEC == 1) {
                *a = y[0];
            } else {
                Tight z;
#pragma unroll
                for (int e = 0; e < VEC; ++e) z[e] = y[e];
                *reinterpret_cast<Tight*>(a) = z;
            }
        };
        ll i = i0;
        for (; i + kU <= i1; i += kU) {
            T x[kU][VEC];
#pragma unroll
            for (int u = 0; u < kU; ++u) load(p + u * inner, x[u]);
#pragma unroll
            for (int u = 0; u < kU; ++u) step(x[u], q + u * inner);
            p += kU * inner;
            q += kU * inner;
        }
        for (; i < i1; ++i) {
            T x[VEC];
            load(p, x);
            step(x, q);
            p += inner;
            q += inner;
        }
        if (mode == 1) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) w[e] = run[e];
        }
    }
}

// ------------------------------------------------------- scan of the totals
// Exclusive scan, in place, of the K chunk totals of every line: a workgroup
// per line c = o*inner + j (element k at ws[(o*K + k)*inner + j]), a
// contiguous run of totals per thread, one block scan of the thread sums.
template <typename T, typename Op>
__global__ __launch_bounds__(kThreads) void scan_totals_kernel(T* ws, ll outer, int K, ll inner) {
    __shared__ T lds[kWaves];
    const Op op;
    const T id = Op::template identity<T>();
    const ll C = outer * inner;
    const int seg = (K + kThreads - 1) / kThreads;
    const int k0 = (int)threadIdx.x * seg < K ? (int)threadIdx.x * seg : K;
    const int k1 = k0 + seg < K ? k0 + seg : K;
    for (ll c = blockIdx.x; c < C; c += gridDim.x) {
        T* const p = ws + (c / inner) * K * inner + c % inner;
        T acc = id;
        for (int k = k0; k < k1; ++k) acc = op(acc, p[k * inner]);
        T tot;
        T run = block_exclusive_scan<kWaves, Op>(acc, lds, tot, op);
        for (int k = k0; k < k1; ++k) {
            const T x = p[k * inner];
            p[k * inner] = run;
            run = op(run, x);
        }
    }
}

template <typename T, typename Op>
int launch(const void* in_, void* out_, ll outer, ll n, ll inner, int exclusive, void* ws_, hipStream_t s) {
    const T* in = (const T*)in_;
    T* out = (T*)out_;
    T* ws = (T*)ws_;
    constexpr int V = 16 / (int)sizeof(T);
    const bool aligned = (reinterpret_cast<uintptr_t>(in_) | reinterpret_cast<uintptr_t>(out_)) % 16 == 0;
    const ScanDimPlan pl = scan_dim_plan(outer, n, inner, (int)sizeof(T), aligned);
    if (pl.chunks > 1 && !ws) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)pl.grid), block(kThreads);
    const int K = pl.chunks;
    auto pass = [&](int mode) {
        if (inner == 1 && pl.waves == 1)
            hipLaunchKernelGGL((scan_rows_kernel<T, Op, 1>), grid, block, 0, s, in, out, outer, n, K, pl.chunk, ws,
                               exclusive, mode);
        else if (inner == 1)
            hipLaunchKernelGGL((scan_rows_kernel<T, Op, kWaves>), grid, block, 0, s, in, out, outer, n, K, pl.chunk,
                               ws, exclusive, mode);
        else if (pl.vector == 1)
            hipLaunchKernelGGL((scan_cols_kernel<T, Op, 1>), grid, block, 0, s, in, out, outer, n, inner, K, pl.chunk,
                               ws, exclusive, mode);
        else
            hipLaunchKernelGGL((scan_cols_kernel<T, Op, V>), grid, block, 0, s, in, out, outer, n, inner, K, pl.chunk,
                               ws, exclusive, mode);
    };
    if (K > 1) {
        pass(1);
        const ll lines = outer * inner;
        const ll cap = (ll)device_cu_count() * 8;
        hipLaunchKernelGGL((scan_totals_kernel<T, Op>), dim3((unsigned)(lines < cap ? lines : cap)), block, 0, s, ws,
                           outer, K, inner);
    }
    pass(0);
    CME_LAUNCH_STATUS();
}

int esize_of(int dtype) { return dtype >= 0 && dtype <= 2 ? 4 : (dtype == 3 || dtype == 4) ? 8 : 0; }

}  // namespace

ScanDimPlan cme::scan_dim_plan(ll outer, ll n, ll inner, int esize, bool aligned16) {
    ScanDimPlan pl{};
    const int V = 16 / esize;
    const ll cus = device_cu_count();
    const long forced = tune_get(kTuneScanDimChunks);
    const long maxblocks = tune_get(kTuneScanDimMaxBlocks);
    ll K = 1;
    if (inner == 1) {
        pl.form = outer == 1 ? 0 : 1;
        pl.vector = V;
        // a wave per line where the lines are short (four wave steps at most) and
        // there is one for every SIMD; a workgroup per line otherwise
        pl.waves = (n <= 4 * kWave * V * kR && outer >= cus * 4) ? 1 : kWaves;
        pl.tile = (ll)pl.waves * kWave * V * kR;
        // chunks where the lines alone leave CUs idle: about four workgroups per
        // CU, of at least four tiles each
        if (outer < cus) K = (4 * cus + outer - 1) / outer;
        const ll most = n / (4 * pl.tile);
        if (K > most) K = most;
        if (K < 1) K = 1;
        if (forced > 0) K = forced;
        ll chunk = (n + K - 1) / K;
        if (forced <= 0 && K > 1) chunk = (chunk + pl.tile - 1) / pl.tile * pl.tile;
        pl.chunk = chunk > 0 ? chunk : 1;
        const ll items = outer * K;
        pl.grid = pl.waves == 1 ? (items + kWaves - 1) / kWaves : items;
    } else {
        pl.form = 2;
        pl.waves = 0;
        const bool vec_ok = aligned16 && inner % V == 0;
        const ll C = outer * inner;
        const ll full = cus * 512;  // lanes that fill the device: two waves per SIMD
        // scalar lanes where the columns alone fill the device: measured faster
        // than lane vectors there (profiles/scan_dim.md), as more waves share the
        // same rows; lane vectors where columns are few and every lane counts
        pl.vector = vec_ok && C < full ? V : 1;
        const ll G = C / pl.vector;
        if (G < full) K = (full + G - 1) / G;
        const ll most = n / kScanDimMinChunkRows;
        if (K > most) K = most;
        if (K < 1) K = 1;
        if (forced > 0) K = forced;
        const ll chunk = (n + K - 1) / K;
        pl.chunk = chunk > 0 ? chunk : 1;
        pl.tile = kScanDimColUnroll;
        pl.grid = (G * K + kThreads - 1) / kThreads;
    }
    pl.chunks = (int)K;
    const ll cap = maxblocks > 0 ? maxblocks : cus * 32;
    if (pl.grid > cap) pl.grid = cap;
    if (pl.grid < 1) pl.grid = 1;
    pl.ws_bytes = K > 1 ? outer * K * inner * esize : 0;
    return pl;
}

#define CME_SCAN_DIM_CASES(CALL)                                  \
    switch (dtype * 4 + op) {                                     \
        case 0: return CALL(float, OpAdd);                        \
        case 1: return CALL(float, OpCumMax);                     \
        case 2: return CALL(float, OpCumMin);                     \
        case 4: return CALL(uint32_t, OpAdd); /* wraps */         \
        case 5: return CALL(int, OpCumMax);                       \
        case 6: return CALL(int, OpCumMin);                       \
        case 8: return CALL(uint32_t, OpAdd);                     \
        case 9: return CALL(uint32_t, OpCumMax);                  \
        case 10: return CALL(uint32_t, OpCumMin);                 \
        case 12: return CALL(u64, OpAdd); /* wraps modulo 2^64 */ \
        case 13: return CALL(ll, OpCumMax);                       \
        case 14: return CALL(ll, OpCumMin);                       \
        case 16: return CALL(double, OpAdd);                      \
        case 17: return CALL(double, OpCumMax);                   \
        case 18: return CALL(double, OpCumMin);                   \
        default: return (int)hipErrorInvalidValue;                \
    }

// Scan of (outer, n, inner) along n. dtype: 0 float32, 1 int32, 2 uint32,
// 3 int64, 4 float64; op: 0 sum, 1 max, 2 min. ws: cme_scan_dim_ws_bytes bytes
// (may be null when that is 0). Never synchronises, allocates nothing.
CME_EXPORT int cme_scan_dim(const void* in, void* out, long long outer, long long n, long long inner, int dtype,
                            int op, int exclusive, void* ws, void* stream) {
    if (outer < 0 || n < 0 || inner < 0 || op < 0 || op > 2 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    hipStream_t s = as_stream(stream);
#define CME_SCAN_DIM_LAUNCH(T, OP) launch<T, OP>(in, out, outer, n, inner, exclusive, ws, s)
    CME_SCAN_DIM_CASES(CME_SCAN_DIM_LAUNCH)
#undef CME_SCAN_DIM_LAUNCH
}

// How cme_scan_dim launches (outer, n, inner) on the current device, for
// operands aligned to 16 bytes: info[0] form (0 flat, 1 row, 2 column),
// [1] chunks K, [2] elements of a line per chunk, [3] tile (row form: elements
// per workgroup or wave step; column form: rows in flight per lane),
// [4] vector (elements per lane access), [5] workgroups of the scan pass,
// [6] workspace bytes, [7] waves that share a line (row form).
CME_EXPORT int cme_scan_dim_info(long long outer, long long n, long long inner, int dtype, int op, int exclusive,
                                 long long* info) {
    if (outer < 0 || n < 0 || inner < 0 || op < 0 || op > 2 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    const ScanDimPlan pl = scan_dim_plan(outer > 0 ? outer : 1, n > 0 ? n : 1, inner > 0 ? inner : 1, esize_of(dtype),
                                         true);
    const bool empty = outer == 0 || n == 0 || inner == 0;
    info[0] = pl.form;
    info[1] = pl.chunks;
    info[2] = pl.chunk;
    info[3] = pl.tile;
    info[4] = pl.vector;
    info[5] = empty ? 0 : pl.grid;
    info[6] = empty ? 0 : pl.ws_bytes;
    info[7] = pl.waves;
    return 0;
}

// Workspace of cme_scan_dim, whatever the alignment of its operands.
CME_EXPORT int cme_scan_dim_ws_bytes(long long outer, long long n, long long inner, int dtype, long long* nbytes) {
    if (outer < 0 || n < 0 || inner < 0 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    *nbytes = 0;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    const ScanDimPlan a = scan_dim_plan(outer, n, inner, esize_of(dtype), true);
    const ScanDimPlan b = scan_dim_plan(outer, n, inner, esize_of(dtype), false);
    *nbytes = a.ws_bytes > b.ws_bytes ? a.ws_bytes : b.ws_bytes;
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(scan_dim_rows_f32, 256, scan_rows_kernel<float, OpAdd, kWaves>);
CME_REGISTER_KERNEL(scan_dim_rows_wave_f32, 256, scan_rows_kernel<float, OpAdd, 1>);
CME_REGISTER_KERNEL(scan_dim_rows_i64, 256, scan_rows_kernel<u64, OpAdd, kWaves>);
CME_REGISTER_KERNEL(scan_dim_rows_wave_f64, 256, scan_rows_kernel<double, OpAdd, 1>);
CME_REGISTER_KERNEL(scan_dim_rows_max_f64, 256, scan_rows_kernel<double, OpCumMax, kWaves>);
CME_REGISTER_KERNEL(scan_dim_rows_max_i32, 256, scan_rows_kernel<int, OpCumMax, kWaves>);
CME_REGISTER_KERNEL(scan_dim_cols_f32, 256, scan_cols_kernel<float, OpAdd, 4>);
CME_REGISTER_KERNEL(scan_dim_cols_scalar_f32, 256, scan_cols_kernel<float, OpAdd, 1>);
CME_REGISTER_KERNEL(scan_dim_cols_i64, 256, scan_cols_kernel<u64, OpAdd, 2>);
CME_REGISTER_KERNEL(scan_dim_cols_max_f64, 256, scan_cols_kernel<double, OpCumMax, 2>);
CME_REGISTER_KERNEL(scan_dim_cols_scalar_min_i64, 256, scan_cols_kernel<ll, OpCumMin, 1>);
CME_REGISTER_KERNEL(scan_dim_totals_f64, 256, scan_totals_kernel<double, OpAdd>);
