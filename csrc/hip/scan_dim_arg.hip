// Running max / min WITH the position of the winner (torch.cummax / cummin:
// values and int64 indices) along one dimension of a contiguous tensor seen as
// (outer, n, inner), element (o, i, j) at (o*n + i)*inner + j. The launch
// plan, the knobs and the three regimes are those of scan_dim.hip (row form,
// column form, chunked reduce-then-scan; a single line -- the flattened 1-D
// case -- is the row form with outer == 1, chunked across the device). No
// kernel waits for another workgroup, and nothing here touches the look-back
// kernels or their descriptors.
//
// The carry is a pair (v, i), i the position along n or "none" (negative).
// Pairs join as a (+) b with a the EARLIER operand: b replaces a iff b is not
// none and b_v >= a_v || b_v != b_v (max; mirrored for min) -- the test of
// OpCumMax. So NaN is sticky, a later NaN takes the index from an earlier
// one, of two equal values (+0.0 / -0.0 included) the later wins, and a real
// element always beats the identity value: every output carries a real index.
// The values are bit for bit those of cme_scan_dim: the identity is a
// two-sided identity of the value operator, so leaving "none" operands out
// does not change a value.
//
// `in` and `out` are not restrict: out may be in. Every lane loads exactly the
// elements it later stores, before it stores them. The index output must not
// overlap either. All index arithmetic is 64-bit; offsets inside a tile step
// (at most 4096 elements) are int.
#include "scan_dim.h"

#include "cme213/wave.h"

using namespace cme;

namespace {

using ll = long long;
constexpr int kThreads = kScanDimThreads;
constexpr int kWaves = kThreads / kWave;
// 16-B vectors per lane and tile step of the row form: the indexed kernels keep
// kScanDimRowVecs (102-153 VGPRs, no scratch), so the plan's tile is theirs
constexpr int kR = kScanDimRowVecs;
constexpr int kU = kScanDimColUnroll;

template <typename T, int V>
struct LaneVec {
    typedef T tight __attribute__((ext_vector_type(V)));
    typedef tight loose __attribute__((aligned(sizeof(T))));
};
using Idx2 = LaneVec<ll, 2>::loose;  // two int64 indices, 8-byte aligned

// later(a, b): the later value b replaces the earlier a.
struct ArgMax {
    using Val = OpCumMax;
    template <typename T> __device__ __forceinline__ static bool later(T a, T b) { return b >= a || b != b; }
};
struct ArgMin {
    using Val = OpCumMin;
    template <typename T> __device__ __forceinline__ static bool later(T a, T b) { return b <= a || b != b; }
};

// (av, ai) = (av, ai) (+) (bv, bi); a negative bi is "none" and never wins.
template <typename A, typename T, typename I>
__device__ __forceinline__ void join(T& av, I& ai, T bv, I bi) {
    const bool w = bi >= 0 && A::later(av, bv);
    av = w ? bv : av;
    ai = w ? bi : ai;
}

// V int64 indices at p (8-byte aligned), as 16-byte stores
template <int V>
__device__ __forceinline__ void store_idx(ll* p, const ll (&y)[V]) {
    if constexpr (V == 1) {
        *p = y[0];
    } else {
#pragma unroll
        for (int e = 0; e < V; e += 2) {
            LaneVec<ll, 2>::tight z;
            z[0] = y[e];
            z[1] = y[e + 1];
            *reinterpret_cast<Idx2*>(p + e) = z;
        }
    }
}

// ------------------------------------------------------------------ row form
// The walk of scan_rows_kernel: NW waves share a line, a tile step covers
// NW * 64 * V * kR elements from the 16-byte boundary at or below the chunk's
// first element, the next tile's loads are issued before this tile's scan.
// Inside a tile step positions are int offsets from the tile's start (-1:
// none). Per 16-B vector the lane folds its elements into a pair; the wave
// scans the lane VALUES with OpCumMax / OpCumMin as the values-only kernel
// does, marks a lane as a record when its pair beats that exclusive prefix,
// and takes the latest record before each lane with one int max-scan. Elements
// outside [lo, hi) -- the masked head and tail -- are "none": they hold the
// identity value but never become records. A tile whose local winner loses to
// the carry keeps the carry's index.
// mode 0: scan (carry pair from the workspace when K > 1); mode 1: pair total
// of every (line, chunk) item only.
template <typename T, typename A, int NW>
__global__ __launch_bounds__(kThreads) void cumarg_rows_kernel(const T* in, T* out, ll* idx, ll outer, ll n, int K,
                                                               ll chunk, T* wsv, ll* wsi, int mode) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int kRowElems = kWave * V;
    constexpr int kWaveElems = kRowElems * kR;
    constexpr int kTile = NW * kWaveElems;
    using Op = typename A::Val;
    using Tight = typename LaneVec<T, V>::tight;
    using Loose = typename LaneVec<T, V>::loose;
    const T id = Op::template identity<T>();
    __shared__ T s_v[2][kWaves];
    __shared__ int s_i[2][kWaves];
    const int lane = lane_id();
    const int wid = threadIdx.x / kWave;
    const ll items = outer * K;
    ll item = NW == 1 ? (ll)blockIdx.x * kWaves + wid : (ll)blockIdx.x;
    const ll stride = NW == 1 ? (ll)gridDim.x * kWaves : (ll)gridDim.x;
    const int woff = (NW == 1 ? 0 : wid * kWaveElems) + lane * V;
    int parity = 0;
    for (; item < items; item += stride) {
        const ll r = K == 1 ? item : item / K;
        const ll k = K == 1 ? 0 : item % K;
        const ll row0 = r * n;
        const ll end = row0 + n;
        ll lo = row0 + k * chunk;
        if (lo > end) lo = end;
        const ll hi = lo + chunk < end ? lo + chunk : end;
        T cv = id;
        ll ci = -1;
        if (K > 1 && mode == 0) {
            cv = wsv[item];
            ci = wsi[item];
        }
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
            // [tlo, thi): the offsets of this tile step that are elements of the chunk
            const int tlo = (int)(lo - t0 > 0 ? lo - t0 : 0);  // < V: only the first step has a head
            const int thi = (int)(hi - t0 < kTile ? hi - t0 : kTile);
            // the pair before each of the lane's vectors within the wave's part of the tile
            T exv[kR];
            int exi[kR];
            T runv = id;
            int runi = -1;
#pragma unroll
            for (int q = 0; q < kR; ++q) {
                const int o0 = woff + q * kRowElems;
                T lv = id;
                int li = -1;
#pragma unroll
                for (int e = 0; e < V; ++e) join<A>(lv, li, v[q][e], (o0 + e >= tlo && o0 + e < thi) ? o0 + e : -1);
                T wt;
                const T x = wave_exclusive_scan<Op>(lv, &wt);
                int wti;
                const int xi = wave_exclusive_scan<OpMax>((li >= 0 && A::later(x, lv)) ? li : -1, &wti);
                exv[q] = runv;
                exi[q] = runi;
                join<A>(exv[q], exi[q], x, xi);
                join<A>(runv, runi, wt, wti);
            }
            // pair before this wave's part: the carry joined with the waves before
            T tv = runv, wv = id;
            int ti = runi, wi = -1;
            if constexpr (NW > 1) {
                if (lane == 0) {
                    s_v[parity][wid] = runv;
                    s_i[parity][wid] = runi;
                }
                lds_bcast_sync();
                tv = id;
                ti = -1;
#pragma unroll
                for (int w = 0; w < NW; ++w) {
                    const T a = s_v[parity][w];
                    const int b = s_i[parity][w];
                    if (w < wid) join<A>(wv, wi, a, b);
                    join<A>(tv, ti, a, b);
                }
                parity ^= 1;
            }
            const ll base = t0 - row0;  // position along the line of the tile's offset 0
            T pv = cv;
            ll pi = ci;
            join<A>(pv, pi, wv, wi >= 0 ? base + wi : (ll)-1);
            if (mode == 0) {
#pragma unroll
                for (int q = 0; q < kR; ++q) {
                    const int o0 = woff + q * kRowElems;
                    const ll i = t0 + o0;
                    T curv = exv[q];
                    int curi = exi[q];
                    T y[V];
                    ll yi[V];
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        join<A>(curv, curi, v[q][e], (o0 + e >= tlo && o0 + e < thi) ? o0 + e : -1);
                        y[e] = pv;
                        yi[e] = pi;
                        join<A>(y[e], yi[e], curv, curi >= 0 ? base + curi : (ll)-1);
                    }
                    if (o0 >= tlo && o0 + V <= thi) {
                        Tight x;
#pragma unroll
                        for (int e = 0; e < V; ++e) x[e] = y[e];
                        *reinterpret_cast<Loose*>(out + i) = x;
                        store_idx<V>(idx + i, yi);
                    } else {
#pragma unroll
                        for (int e = 0; e < V; ++e)
                            if (o0 + e >= tlo && o0 + e < thi) {
                                out[i + e] = y[e];
                                idx[i + e] = yi[e];
                            }
                    }
                }
            }
            join<A>(cv, ci, tv, ti >= 0 ? base + ti : (ll)-1);
#pragma unroll
            for (int q = 0; q < kR; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) v[q][e] = nv[q][e];
        }
        if (mode == 1 && lane == 0 && (NW == 1 || wid == 0)) {
            wsv[item] = cv;
            wsi[item] = ci;
        }
    }
}

// --------------------------------------------------------------- column form
// The mapping of scan_cols_kernel: one lane per group of VEC adjacent columns
// and per chunk, the running pair of every column in registers (the index is
// the row i), kScanDimColUnroll rows of loads in flight, no LDS, no barrier.
// The totals are at [(o*K + k)*inner + j] of wsv / wsi.
template <typename T, typename A, int VEC>
__global__ __launch_bounds__(kThreads) void cumarg_cols_kernel(const T* in, T* out, ll* idx, ll outer, ll n, ll inner,
                                                               int K, ll chunk, T* wsv, ll* wsi, int mode) {
    using Op = typename A::Val;
    using Tight = typename LaneVec<T, VEC>::tight;
    const T id = Op::template identity<T>();
    const ll G = outer * inner / VEC;
    const ll total = G * K;
    const bool narrow = outer * inner < (1ll << 31);
    for (ll t = (ll)blockIdx.x * kThreads + threadIdx.x; t < total; t += (ll)gridDim.x * kThreads) {
        const ll k = K == 1 ? 0 : t / G;
        const ll g = t - k * G;
        const ll c = g * VEC;
        const ll o = outer == 1 ? 0 : narrow ? (ll)((unsigned)c / (unsigned)inner) : c / inner;
        const ll j = c - o * inner;
        ll i0 = k * chunk;
        if (i0 > n) i0 = n;
        const ll i1 = i0 + chunk < n ? i0 + chunk : n;
        const ll w = (o * K + k) * inner + j;
        T run[VEC];
        ll runi[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            run[e] = (K > 1 && mode == 0) ? wsv[w + e] : id;
            runi[e] = (K > 1 && mode == 0) ? wsi[w + e] : (ll)-1;
        }
        const ll off = (o * n + i0) * inner + j;
        const T* p = in + off;
        T* q = out + off;
        ll* qi = idx + off;
        auto load = [&](const T* a, T(&x)[VEC]) {
            if constexpr (VEC == 1) {
                x[0] = *a;
            } else {
                const Tight y = *reinterpret_cast<const Tight*>(a);
#pragma unroll
                for (int e = 0; e < VEC; ++e) x[e] = y[e];
            }
        };
        auto step = [&](T(&x)[VEC], ll i, T* a, ll* ai) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) join<A>(run[e], runi[e], x[e], i);
            if (mode != 0) return;
            if constexpr (VEC == 1) {
                *a = run[0];
            } else {
                Tight z;
#pragma unroll
                for (int e = 0; e < VEC; ++e) z[e] = run[e];
                *reinterpret_cast<Tight*>(a) = z;
            }
            store_idx<VEC>(ai, runi);
        };
        ll i = i0;
        for (; i + kU <= i1; i += kU) {
            T x[kU][VEC];
#pragma unroll
            for (int u = 0; u < kU; ++u) load(p + u * inner, x[u]);
#pragma unroll
            for (int u = 0; u < kU; ++u) step(x[u], i + u, q + u * inner, qi + u * inner);
            p += kU * inner;
            q += kU * inner;
            qi += kU * inner;
        }
        for (; i < i1; ++i) {
            T x[VEC];
            load(p, x);
            step(x, i, q, qi);
            p += inner;
            q += inner;
            qi += inner;
        }
        if (mode == 1) {
#pragma unroll
            for (int e = 0; e < VEC; ++e) {
                wsv[w + e] = run[e];
                wsi[w + e] = runi[e];
            }
        }
    }
}

// ------------------------------------------------------- scan of the totals
// Exclusive pair scan, in place, of the K chunk totals of every line (element
// k of line c = o*inner + j at [(o*K + k)*inner + j]): a workgroup per line, a
// contiguous run of totals per thread. The block scans the thread VALUES; a
// thread whose pair beats that exclusive prefix is a record, and the latest
// record before each thread is a max-scan of the record positions, which grow
// with the thread.
template <typename T, typename A>
__global__ __launch_bounds__(kThreads) void cumarg_totals_kernel(T* wsv, ll* wsi, ll outer, int K, ll inner) {
    using Op = typename A::Val;
    __shared__ T lds_v[kWaves];
    __shared__ ll lds_i[kWaves];
    const T id = Op::template identity<T>();
    const ll C = outer * inner;
    const int seg = (K + kThreads - 1) / kThreads;
    const int k0 = (int)threadIdx.x * seg < K ? (int)threadIdx.x * seg : K;
    const int k1 = k0 + seg < K ? k0 + seg : K;
    for (ll c = blockIdx.x; c < C; c += gridDim.x) {
        const ll at = (c / inner) * K * inner + c % inner;
        T* const pv = wsv + at;
        ll* const pi = wsi + at;
        T av = id;
        ll ai = -1;
        for (int k = k0; k < k1; ++k) join<A>(av, ai, pv[k * inner], pi[k * inner]);
        T totv;
        ll toti;
        T runv = block_exclusive_scan<kWaves, Op>(av, lds_v, totv);
        ll runi = block_exclusive_scan<kWaves, OpMax>((ai >= 0 && A::later(runv, av)) ? ai : (ll)-1, lds_i, toti);
        for (int k = k0; k < k1; ++k) {
            const T xv = pv[k * inner];
            const ll xi = pi[k * inner];
            pv[k * inner] = runv;
            pi[k * inner] = runi >= 0 ? runi : (ll)-1;
            join<A>(runv, runi, xv, xi);
        }
    }
}

int esize_of(int dtype) { return dtype >= 0 && dtype <= 2 ? 4 : (dtype == 3 || dtype == 4) ? 8 : 0; }

// workspace of K > 1: the int64 index totals first (8-byte aligned whatever
// the element size), then the value totals
ll ws_bytes_of(const ScanDimPlan& pl, ll outer, ll inner, int esize) {
    return pl.chunks > 1 ? outer * pl.chunks * inner * (esize + 8) : 0;
}

template <typename T, typename A>
int launch(const void* in_, void* out_, void* idx_, ll outer, ll n, ll inner, void* ws_, hipStream_t s) {
    const T* in = (const T*)in_;
    T* out = (T*)out_;
    ll* idx = (ll*)idx_;
    constexpr int V = 16 / (int)sizeof(T);
    const bool aligned = (reinterpret_cast<uintptr_t>(in_) | reinterpret_cast<uintptr_t>(out_)) % 16 == 0;
    const ScanDimPlan pl = scan_dim_plan(outer, n, inner, (int)sizeof(T), aligned);
    if (pl.chunks > 1 && !ws_) return (int)hipErrorInvalidValue;
    const int K = pl.chunks;
    ll* wsi = (ll*)ws_;
    T* wsv = (T*)(wsi + (K > 1 ? outer * K * inner : 0));
    const dim3 grid((unsigned)pl.grid), block(kThreads);
    auto pass = [&](int mode) {
        if (inner == 1 && pl.waves == 1)
            hipLaunchKernelGGL((cumarg_rows_kernel<T, A, 1>), grid, block, 0, s, in, out, idx, outer, n, K, pl.chunk,
                               wsv, wsi, mode);
        else if (inner == 1)
            hipLaunchKernelGGL((cumarg_rows_kernel<T, A, kWaves>), grid, block, 0, s, in, out, idx, outer, n, K,
                               pl.chunk, wsv, wsi, mode);
        else if (pl.vector == 1)
            hipLaunchKernelGGL((cumarg_cols_kernel<T, A, 1>), grid, block, 0, s, in, out, idx, outer, n, inner, K,
                               pl.chunk, wsv, wsi, mode);
        else
            hipLaunchKernelGGL((cumarg_cols_kernel<T, A, V>), grid, block, 0, s, in, out, idx, outer, n, inner, K,
                               pl.chunk, wsv, wsi, mode);
    };
    if (K > 1) {
        pass(1);
        const ll lines = outer * inner;
        const ll cap = (ll)device_cu_count() * 8;
        hipLaunchKernelGGL((cumarg_totals_kernel<T, A>), dim3((unsigned)(lines < cap ? lines : cap)), block, 0, s, wsv,
                           wsi, outer, K, inner);
    }
    pass(0);
    CME_LAUNCH_STATUS();
}

}  // namespace

// Running max (op 1) / min (op 2) of (outer, n, inner) along n with the
// position of the winner: out_values as cme_scan_dim's inclusive result (may
// be in), out_indices int64 positions along n (8-byte aligned, overlapping
// neither). dtype: 0 float32, 1 int32, 2 uint32, 3 int64, 4 float64. ws:
// cme_cumarg_dim_ws_bytes bytes, 8-byte aligned (may be null when that is 0).
// Never synchronises, allocates nothing.
CME_EXPORT int cme_cumarg_dim(const void* in, void* out_values, void* out_indices, long long outer, long long n,
                              long long inner, int dtype, int op, void* ws, void* stream) {
    if (outer < 0 || n < 0 || inner < 0 || op < 1 || op > 2 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (!in || !out_values || !out_indices) return (int)hipErrorInvalidValue;
    hipStream_t s = as_stream(stream);
#define CME_CUMARG_LAUNCH(T, A) launch<T, A>(in, out_values, out_indices, outer, n, inner, ws, s)
    switch (dtype * 4 + op) {
        case 1: return CME_CUMARG_LAUNCH(float, ArgMax);
        case 2: return CME_CUMARG_LAUNCH(float, ArgMin);
        case 5: return CME_CUMARG_LAUNCH(int, ArgMax);
        case 6: return CME_CUMARG_LAUNCH(int, ArgMin);
        case 9: return CME_CUMARG_LAUNCH(uint32_t, ArgMax);
        case 10: return CME_CUMARG_LAUNCH(uint32_t, ArgMin);
        case 13: return CME_CUMARG_LAUNCH(ll, ArgMax);
        case 14: return CME_CUMARG_LAUNCH(ll, ArgMin);
        case 17: return CME_CUMARG_LAUNCH(double, ArgMax);
        case 18: return CME_CUMARG_LAUNCH(double, ArgMin);
        default: return (int)hipErrorInvalidValue;
    }
#undef CME_CUMARG_LAUNCH
}

// How cme_cumarg_dim launches (outer, n, inner) on the current device, for
// operands aligned to 16 bytes: the eight fields of cme_scan_dim_info, with
// [6] the workspace of both totals arrays. Form 0 (a single line) runs as the
// row form with outer == 1.
CME_EXPORT int cme_cumarg_dim_info(long long outer, long long n, long long inner, int dtype, int op, long long* info) {
    if (outer < 0 || n < 0 || inner < 0 || op < 1 || op > 2 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    const int esize = esize_of(dtype);
    const ll o1 = outer > 0 ? outer : 1, i1 = inner > 0 ? inner : 1;
    const ScanDimPlan pl = scan_dim_plan(o1, n > 0 ? n : 1, i1, esize, true);
    const bool empty = outer == 0 || n == 0 || inner == 0;
    info[0] = pl.form;
    info[1] = pl.chunks;
    info[2] = pl.chunk;
    info[3] = pl.tile;  // kR == kScanDimRowVecs: the tile of the plan
    info[4] = pl.vector;
    info[5] = empty ? 0 : pl.grid;
    info[6] = empty ? 0 : ws_bytes_of(pl, o1, i1, esize);
    info[7] = pl.waves;
    return 0;
}

// Workspace of cme_cumarg_dim, whatever the alignment of its operands.
CME_EXPORT int cme_cumarg_dim_ws_bytes(long long outer, long long n, long long inner, int dtype, long long* nbytes) {
    if (outer < 0 || n < 0 || inner < 0 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    *nbytes = 0;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    const int esize = esize_of(dtype);
    const ll a = ws_bytes_of(scan_dim_plan(outer, n, inner, esize, true), outer, inner, esize);
    const ll b = ws_bytes_of(scan_dim_plan(outer, n, inner, esize, false), outer, inner, esize);
    *nbytes = a > b ? a : b;
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(cumarg_rows_max_f32, 256, cumarg_rows_kernel<float, ArgMax, kWaves>);
CME_REGISTER_KERNEL(cumarg_rows_wave_min_f32, 256, cumarg_rows_kernel<float, ArgMin, 1>);
CME_REGISTER_KERNEL(cumarg_rows_max_i64, 256, cumarg_rows_kernel<ll, ArgMax, kWaves>);
CME_REGISTER_KERNEL(cumarg_rows_wave_max_f64, 256, cumarg_rows_kernel<double, ArgMax, 1>);
CME_REGISTER_KERNEL(cumarg_cols_max_f32, 256, cumarg_cols_kernel<float, ArgMax, 4>);
CME_REGISTER_KERNEL(cumarg_cols_scalar_max_f32, 256, cumarg_cols_kernel<float, ArgMax, 1>);
CME_REGISTER_KERNEL(cumarg_cols_min_i64, 256, cumarg_cols_kernel<ll, ArgMin, 2>);
CME_REGISTER_KERNEL(cumarg_totals_max_f64, 256, cumarg_totals_kernel<double, ArgMax>);
