// Reductions along one dimension of a contiguous tensor seen as (outer, n,
// inner), element (o, i, j) at (o*n + i)*inner + j: line (o, j) is reduced over
// i to one value, or to a (value, index) pair. Sum, max and min of float32,
// int32, uint32, int64 and float64. The launch plan (form, waves per line,
// lane vector, chunks K along n, grid) and the knobs are those of scan_dim.hip
// (scan_dim_plan); only the work differs: a lane folds what it loads into
// accumulators of its own, a line costs one wave reduce (DPP) and, where four
// waves share it, one LDS hand-off.
//
//  * sum: the result has the element type; integers wrap (int32 and uint32
//    share the uint32_t kernels, int64 runs as uint64). A float sum is a tree
//    fixed by the launch shape and the 16-byte phase of the operand's address.
//  * max / min, values only: IEEE 754-2019 maximum / minimum. A NaN in the line
//    gives NaN, max(+0.0, -0.0) is +0.0 and min is -0.0.
//  * max / min with indices: the rule of torch.max(x, dim) on CPU tensors. The
//    first NaN if there is one, else the first element equal to the extreme;
//    the value is x at that index. Pairs (v, i) join as: the better value wins
//    (NaN beats any non-NaN), on a tie (equal, or both NaN) the smaller index.
//    "No candidate" is (identity value, kNone): kNone is the largest int64, so
//    it loses every tie against a real element and the join needs no validity
//    test. The join is commutative and associative: lanes hold strided subsets.
//
// K > 1: pass 1 writes the partial of every (line, chunk) to the workspace
// (int64 index plane first, then the values, element k of line (o, j) at
// [(o*K + k)*inner + j]), a finish kernel folds the K partials of every line.
// No kernel waits for another workgroup, there are no atomics, and all index
// arithmetic is 64-bit. Nothing here synchronises or allocates.
#include "scan_dim.h"

#include "cme213/wave.h"

using namespace cme;

namespace {

using u64 = unsigned long long;
using ll = long long;
constexpr int kThreads = kScanDimThreads;
constexpr int kWaves = kThreads / kWave;
constexpr int kR = kScanDimRowVecs;
constexpr int kU = kScanDimColUnroll;
constexpr ll kNone = 0x7fffffffffffffffll;
// finish kernel: a thread per line up to this many chunks, a workgroup per line above
constexpr int kFinishThreadK = 32;

template <typename T, int V>
struct LaneVec {
    typedef T tight __attribute__((ext_vector_type(V)));
};

template <typename T> struct IsFloat { static constexpr bool value = false; };
template <> struct IsFloat<float> { static constexpr bool value = true; };
template <> struct IsFloat<double> { static constexpr bool value = true; };

// ---------------------------------------------------------------- operators
// Values only. kOrdered = false: wave_reduce / block_reduce take them as they
// take OpAdd. For two equal floats the bits are equal unless they are zeros of
// both signs, so AND (max) / OR (min) of the bits picks +0.0 / -0.0.
struct RedSum {
    static constexpr bool kPair = false;
    static constexpr bool kOrdered = false;
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
    template <typename T> __device__ __forceinline__ static T identity() { return T(0); }
};
struct RedMax {
    static constexpr bool kPair = false;
    static constexpr bool kOrdered = false;
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const {
        if constexpr (IsFloat<T>::value) {
            using U = typename Bits<T>::U;
            const T eq = __builtin_bit_cast(T, (U)(__builtin_bit_cast(U, a) & __builtin_bit_cast(U, b)));
            const T r = a > b ? a : b > a ? b : eq;
            return a != a ? a : b != b ? b : r;
        } else {
            return a > b ? a : b;
        }
    }
    template <typename T> __device__ __forceinline__ static T identity() { return OpMax::identity<T>(); }
};
struct RedMin {
    static constexpr bool kPair = false;
    static constexpr bool kOrdered = false;
    template <typename T> __device__ __forceinline__ T operator()(T a, T b) const {
        if constexpr (IsFloat<T>::value) {
            using U = typename Bits<T>::U;
            const T eq = __builtin_bit_cast(T, (U)(__builtin_bit_cast(U, a) | __builtin_bit_cast(U, b)));
            const T r = a < b ? a : b < a ? b : eq;
            return a != a ? a : b != b ? b : r;
        } else {
            return a < b ? a : b;
        }
    }
    template <typename T> __device__ __forceinline__ static T identity() { return OpMin::identity<T>(); }
};
// With indices. wins(a, ai, b, bi): the pair b replaces the pair a.
struct RedArgMax {
    static constexpr bool kPair = true;
    template <typename T> __device__ __forceinline__ static bool wins(T a, ll ai, T b, ll bi) {
        if constexpr (IsFloat<T>::value) {
            const bool na = a != a, nb = b != b;
            return (nb && !na) || b > a || ((a == b || (na && nb)) && bi < ai);
        } else {
            return b > a || (a == b && bi < ai);
        }
    }
    template <typename T> __device__ __forceinline__ static T identity() { return OpMax::identity<T>(); }
};
struct RedArgMin {
    static constexpr bool kPair = true;
    template <typename T> __device__ __forceinline__ static bool wins(T a, ll ai, T b, ll bi) {
        if constexpr (IsFloat<T>::value) {
            const bool na = a != a, nb = b != b;
            return (nb && !na) || b < a || ((a == b || (na && nb)) && bi < ai);
        } else {
            return b < a || (a == b && bi < ai);
        }
    }
    template <typename T> __device__ __forceinline__ static T identity() { return OpMin::identity<T>(); }
};

// ------------------------------------------------------------- accumulators
// One interface over "a value" and "a (value, index) pair", so every kernel is
// written once. take: fold an element at position i of its line; join: fold
// another accumulator; wave: the wave's total in every lane (DPP); block: the
// workgroup's total in every thread (one LDS hand-off).
template <typename T>
struct BlockLds {
    T v[2][kWaves];
    ll i[2][kWaves];
};

template <typename T, typename R, bool = R::kPair>
struct Acc {
    T v;
    __device__ __forceinline__ void init() { v = R::template identity<T>(); }
    __device__ __forceinline__ void take(T x, ll) { v = R()(v, x); }
    __device__ __forceinline__ void join(const Acc& o) { v = R()(v, o.v); }
    __device__ __forceinline__ void wave() { v = wave_reduce<R>(v); }
    __device__ __forceinline__ void block(BlockLds<T>& s, int&) { v = block_reduce<kWaves, R>(v, s.v[0]); }
    __device__ __forceinline__ void load(const T* pv, const ll*, ll at) { v = pv[at]; }
    __device__ __forceinline__ void store(T* pv, ll*, ll at) const { pv[at] = v; }
};

template <typename T, typename R>
struct Acc<T, R, true> {
    T v;
    ll i;
    __device__ __forceinline__ void init() {
        v = R::template identity<T>();
        i = kNone;
    }
    __device__ __forceinline__ void take(T x, ll xi) {
        const bool w = R::wins(v, i, x, xi);
        v = w ? x : v;
        i = w ? xi : i;
    }
    __device__ __forceinline__ void join(const Acc& o) { take(o.v, o.i); }
    template <int CTRL, int ROW_MASK = 0xf>
    __device__ __forceinline__ void dpp_step() {
        // lanes without a source lane receive "no candidate"
        const T sv = dpp_move<CTRL, ROW_MASK>(R::template identity<T>(), v);
        const ll si = dpp_move<CTRL, ROW_MASK>(kNone, i);
        take(sv, si);
    }
    __device__ __forceinline__ void wave() {
        // the lane moves of wave_inclusive_scan: lane 63 ends with the total
        dpp_step<kDppRowShr1>();
        dpp_step<kDppRowShr2>();
        dpp_step<kDppRowShr4>();
        dpp_step<kDppRowShr8>();
        dpp_step<kDppRowBcast15, 0xa>();
        dpp_step<kDppRowBcast31, 0xc>();
        v = wave_readlane(v, kWave - 1);
        i = wave_readlane(i, kWave - 1);
    }
    // the hand-off of cumarg_rows_kernel: lane 0 of every wave writes, one
    // lds_bcast_sync, every thread folds the four; parity double-buffers it
    __device__ __forceinline__ void block(BlockLds<T>& s, int& parity) {
        wave();
        const int wid = threadIdx.x / kWave;
        if (lane_id() == 0) {
            s.v[parity][wid] = v;
            s.i[parity][wid] = i;
        }
        lds_bcast_sync();
        init();
#pragma unroll
        for (int w = 0; w < kWaves; ++w) take(s.v[parity][w], s.i[parity][w]);
        parity ^= 1;
    }
    __device__ __forceinline__ void load(const T* pv, const ll* pi, ll at) {
        v = pv[at];
        i = pi[at];
    }
    __device__ __forceinline__ void store(T* pv, ll* pi, ll at) const {
        pv[at] = v;
        pi[at] = i;
    }
};

// ------------------------------------------------------------------ row form
// NW waves share a (line, chunk) item: NW == 4 a workgroup per item, NW == 1 a
// wave per item (no LDS, no barrier). The walk of scan_rows_kernel: a tile
// step covers NW * 64 * V * kR elements from the 16-byte boundary at or below
// the chunk's first element, so every whole vector is an aligned 16-B load,
// and the next step's loads are issued before this step is folded. Elements
// outside [lo, hi) -- the masked head and tail -- read as the identity, and as
// "no candidate" for pairs. A lane folds element e of its vectors into its
// accumulator e. The result of item (r, k) goes to [r*K + k] of ov / oi: out
// and idx when K == 1, the workspace planes otherwise.
template <typename T, typename R, int NW>
__global__ __launch_bounds__(kThreads) void reduce_rows_kernel(const T* in, T* ov, ll* oi, ll outer, ll n, int K,
                                                               ll chunk) {
    constexpr int V = 16 / (int)sizeof(T);
    constexpr int kRowElems = kWave * V;
    constexpr int kWaveElems = kRowElems * kR;
    constexpr int kTile = NW * kWaveElems;
    using Tight = typename LaneVec<T, V>::tight;
    const T id = R::template identity<T>();
    __shared__ BlockLds<T> lds;
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
        Acc<T, R> acc[V];
#pragma unroll
        for (int e = 0; e < V; ++e) acc[e].init();
        ll t0 = lo - phase;
        if (t0 < hi) load_tile(t0, v);
        for (; t0 < hi; t0 += kTile) {
            if (t0 + kTile < hi) load_tile(t0 + kTile, nv);
            const ll p0 = t0 + woff;  // the lane's first element of this step
            if (!R::kPair || (t0 >= lo && t0 + kTile <= hi)) {
                // values, or a step inside the chunk: nothing to mask
#pragma unroll
                for (int q = 0; q < kR; ++q)
#pragma unroll
                    for (int e = 0; e < V; ++e) acc[e].take(v[q][e], p0 + q * kRowElems + e - row0);
            } else {
#pragma unroll
                for (int q = 0; q < kR; ++q)
#pragma unroll
                    for (int e = 0; e < V; ++e) {
                        const ll p = p0 + q * kRowElems + e;
                        acc[e].take(v[q][e], (p >= lo && p < hi) ? p - row0 : kNone);
                    }
            }
#pragma unroll
            for (int q = 0; q < kR; ++q)
#pragma unroll
                for (int e = 0; e < V; ++e) v[q][e] = nv[q][e];
        }
#pragma unroll
        for (int e = 1; e < V; ++e) acc[0].join(acc[e]);
        if constexpr (NW == 1) {
            acc[0].wave();
            if (lane == 0) acc[0].store(ov, oi, item);
        } else {
            acc[0].block(lds, parity);
            if (threadIdx.x == 0) acc[0].store(ov, oi, item);
        }
    }
}

// --------------------------------------------------------------- column form
// The mapping of scan_cols_kernel: one lane per group of VEC adjacent columns
// and per chunk, the accumulators of its columns in registers, kScanDimColUnroll
// rows of loads in flight, no LDS, no barrier, one store per column. The result
// of column j of (o, k) goes to [(o*K + k)*inner + j] of ov / oi.
template <typename T, typename R, int VEC>
__global__ __launch_bounds__(kThreads) void reduce_cols_kernel(const T* in, T* ov, ll* oi, ll outer, ll n, ll inner,
                                                               int K, ll chunk) {
    using Tight = typename LaneVec<T, VEC>::tight;
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
        Acc<T, R> acc[VEC];
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e].init();
        const T* p = in + ((o * n + i0) * inner + j);
        auto load = [&](const T* a, T(&x)[VEC]) {
            if constexpr (VEC == 1) {
                x[0] = *a;
            } else {
                const Tight y = *reinterpret_cast<const Tight*>(a);
#pragma unroll
                for (int e = 0; e < VEC; ++e) x[e] = y[e];
            }
        };
        ll i = i0;
        for (; i + kU <= i1; i += kU) {
            T x[kU][VEC];
#pragma unroll
            for (int u = 0; u < kU; ++u) load(p + u * inner, x[u]);
#pragma unroll
            for (int u = 0; u < kU; ++u)
#pragma unroll
                for (int e = 0; e < VEC; ++e) acc[e].take(x[u][e], i + u);
            p += kU * inner;
        }
        for (; i < i1; ++i) {
            T x[VEC];
            load(p, x);
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[e].take(x[e], i);
            p += inner;
        }
        const ll w = (o * K + k) * inner + j;
#pragma unroll
        for (int e = 0; e < VEC; ++e) acc[e].store(ov, oi, w + e);
    }
}

// ------------------------------------------------------------------- finish
// Folds the K partials of every line c = o*inner + j (partial k at
// [(o*K + k)*inner + j] of wsv / wsi) into out[c] / idx[c], in chunk order.
// WIDE == false: a thread per line (adjacent threads read adjacent columns).
// WIDE == true: a workgroup per line, a contiguous run of partials per thread.
template <typename T, typename R, bool WIDE>
__global__ __launch_bounds__(kThreads) void reduce_finish_kernel(const T* wsv, const ll* wsi, T* out, ll* idx,
                                                                 ll outer, int K, ll inner) {
    const ll C = outer * inner;
    if constexpr (!WIDE) {
        for (ll c = (ll)blockIdx.x * kThreads + threadIdx.x; c < C; c += (ll)gridDim.x * kThreads) {
            const ll at = inner == 1 ? c * K : (c / inner) * K * inner + c % inner;
            Acc<T, R> acc, x;
            acc.init();
            for (int k = 0; k < K; ++k) {
                x.load(wsv, wsi, at + k * inner);
                acc.join(x);
            }
            acc.store(out, idx, c);
        }
    } else {
        __shared__ BlockLds<T> lds;
        const int seg = (K + kThreads - 1) / kThreads;
        const int k0 = (int)threadIdx.x * seg < K ? (int)threadIdx.x * seg : K;
        const int k1 = k0 + seg < K ? k0 + seg : K;
        int parity = 0;
        for (ll c = blockIdx.x; c < C; c += gridDim.x) {
            const ll at = (c / inner) * K * inner + c % inner;
            Acc<T, R> acc, x;
            acc.init();
            for (int k = k0; k < k1; ++k) {
                x.load(wsv, wsi, at + k * inner);
                acc.join(x);
            }
            acc.block(lds, parity);
            if (threadIdx.x == 0) acc.store(out, idx, c);
        }
    }
}

int esize_of(int dtype) { return dtype >= 0 && dtype <= 2 ? 4 : (dtype == 3 || dtype == 4) ? 8 : 0; }

// workspace of K > 1: the int64 index partials first (8-byte aligned whatever
// the element size), then the value partials
ll ws_bytes_of(const ScanDimPlan& pl, ll outer, ll inner, int esize, bool indices) {
    return pl.chunks > 1 ? outer * pl.chunks * inner * (esize + (indices ? 8 : 0)) : 0;
}

template <typename T, typename R>
int launch(const void* in_, void* out_, void* idx_, ll outer, ll n, ll inner, void* ws_, hipStream_t s) {
    const T* in = (const T*)in_;
    T* out = (T*)out_;
    ll* idx = (ll*)idx_;
    constexpr int V = 16 / (int)sizeof(T);
    // only the operand is read in vectors; results are stored one element at a time
    const bool aligned = reinterpret_cast<uintptr_t>(in_) % 16 == 0;
    const ScanDimPlan pl = scan_dim_plan(outer, n, inner, (int)sizeof(T), aligned);
    if (pl.chunks > 1 && !ws_) return (int)hipErrorInvalidValue;
    const int K = pl.chunks;
    const ll lines = outer * inner;
    ll* wsi = (ll*)ws_;
    T* wsv = (R::kPair && K > 1) ? (T*)(wsi + lines * K) : (T*)ws_;
    T* ov = K > 1 ? wsv : out;
    ll* oi = K > 1 ? wsi : idx;
    const dim3 grid((unsigned)pl.grid), block(kThreads);
    if (inner == 1 && pl.waves == 1)
        hipLaunchKernelGGL((reduce_rows_kernel<T, R, 1>), grid, block, 0, s, in, ov, oi, outer, n, K, pl.chunk);
    else if (inner == 1)
        hipLaunchKernelGGL((reduce_rows_kernel<T, R, kWaves>), grid, block, 0, s, in, ov, oi, outer, n, K, pl.chunk);
    else if (pl.vector == 1)
        hipLaunchKernelGGL((reduce_cols_kernel<T, R, 1>), grid, block, 0, s, in, ov, oi, outer, n, inner, K, pl.chunk);
    else
        hipLaunchKernelGGL((reduce_cols_kernel<T, R, V>), grid, block, 0, s, in, ov, oi, outer, n, inner, K, pl.chunk);
    if (K > 1) {
        const ll cap = (ll)device_cu_count() * 8;
        if (K <= kFinishThreadK) {
            const ll want = (lines + kThreads - 1) / kThreads;
            hipLaunchKernelGGL((reduce_finish_kernel<T, R, false>), dim3((unsigned)(want < cap ? want : cap)), block, 0,
                               s, wsv, wsi, out, idx, outer, K, inner);
        } else {
            hipLaunchKernelGGL((reduce_finish_kernel<T, R, true>), dim3((unsigned)(lines < cap ? lines : cap)), block,
                               0, s, wsv, wsi, out, idx, outer, K, inner);
        }
    }
    CME_LAUNCH_STATUS();
}

bool bad_args(ll outer, ll n, ll inner, int dtype, int op, bool indices) {
    return outer < 0 || n < 0 || inner < 0 || op < 0 || op > 2 || !esize_of(dtype) || (indices && op == 0);
}

}  // namespace

// Reduction of (outer, n, inner) along n: out holds outer * inner elements of
// the operand's type, result of line (o, j) at [o*inner + j]. out_indices:
// null for values only, else outer * inner int64 positions along n (op 1 / 2
// only; a sum with indices is an error). dtype: 0 float32, 1 int32, 2 uint32,
// 3 int64, 4 float64; op: 0 sum, 1 max, 2 min. n == 0 is the caller's to
// refuse or fill: nothing is launched for an empty operand. ws:
// cme_reduce_dim_ws_bytes bytes, 8-byte aligned (may be null when that is 0).
CME_EXPORT int cme_reduce_dim(const void* in, void* out, void* out_indices, long long outer, long long n,
                              long long inner, int dtype, int op, void* ws, void* stream) {
    if (bad_args(outer, n, inner, dtype, op, out_indices != nullptr)) return (int)hipErrorInvalidValue;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (!in || !out) return (int)hipErrorInvalidValue;
    hipStream_t s = as_stream(stream);
#define CME_REDUCE_DIM_LAUNCH(T, R) launch<T, R>(in, out, out_indices, outer, n, inner, ws, s)
    if (out_indices) {
        switch (dtype * 4 + op) {
            case 1: return CME_REDUCE_DIM_LAUNCH(float, RedArgMax);
            case 2: return CME_REDUCE_DIM_LAUNCH(float, RedArgMin);
            case 5: return CME_REDUCE_DIM_LAUNCH(int, RedArgMax);
            case 6: return CME_REDUCE_DIM_LAUNCH(int, RedArgMin);
            case 9: return CME_REDUCE_DIM_LAUNCH(uint32_t, RedArgMax);
            case 10: return CME_REDUCE_DIM_LAUNCH(uint32_t, RedArgMin);
            case 13: return CME_REDUCE_DIM_LAUNCH(ll, RedArgMax);
            case 14: return CME_REDUCE_DIM_LAUNCH(ll, RedArgMin);
            case 17: return CME_REDUCE_DIM_LAUNCH(double, RedArgMax);
            case 18: return CME_REDUCE_DIM_LAUNCH(double, RedArgMin);
            default: return (int)hipErrorInvalidValue;
        }
    }
    switch (dtype * 4 + op) {
        case 0: return CME_REDUCE_DIM_LAUNCH(float, RedSum);
        case 1: return CME_REDUCE_DIM_LAUNCH(float, RedMax);
        case 2: return CME_REDUCE_DIM_LAUNCH(float, RedMin);
        case 4: return CME_REDUCE_DIM_LAUNCH(uint32_t, RedSum);  // wraps
        case 5: return CME_REDUCE_DIM_LAUNCH(int, RedMax);
        case 6: return CME_REDUCE_DIM_LAUNCH(int, RedMin);
        case 8: return CME_REDUCE_DIM_LAUNCH(uint32_t, RedSum);
        case 9: return CME_REDUCE_DIM_LAUNCH(uint32_t, RedMax);
        case 10: return CME_REDUCE_DIM_LAUNCH(uint32_t, RedMin);
        case 12: return CME_REDUCE_DIM_LAUNCH(u64, RedSum);  // wraps modulo 2^64
        case 13: return CME_REDUCE_DIM_LAUNCH(ll, RedMax);
        case 14: return CME_REDUCE_DIM_LAUNCH(ll, RedMin);
        case 16: return CME_REDUCE_DIM_LAUNCH(double, RedSum);
        case 17: return CME_REDUCE_DIM_LAUNCH(double, RedMax);
        case 18: return CME_REDUCE_DIM_LAUNCH(double, RedMin);
        default: return (int)hipErrorInvalidValue;
    }
#undef CME_REDUCE_DIM_LAUNCH
}

// How cme_reduce_dim launches (outer, n, inner) on the current device, for an
// operand aligned to 16 bytes: the eight fields of cme_scan_dim_info, with [5]
// the workgroups of the reduce pass and [6] the workspace of the partials
// (values, and the int64 indices when `indices`). Form 0 (a single line) runs
// as the row form with outer == 1.
CME_EXPORT int cme_reduce_dim_info(long long outer, long long n, long long inner, int dtype, int op, int indices,
                                   long long* info) {
    if (bad_args(outer, n, inner, dtype, op, indices != 0)) return (int)hipErrorInvalidValue;
    const int esize = esize_of(dtype);
    const ll o1 = outer > 0 ? outer : 1, i1 = inner > 0 ? inner : 1;
    const ScanDimPlan pl = scan_dim_plan(o1, n > 0 ? n : 1, i1, esize, true);
    const bool empty = outer == 0 || n == 0 || inner == 0;
    info[0] = pl.form;
    info[1] = pl.chunks;
    info[2] = pl.chunk;
    info[3] = pl.tile;
    info[4] = pl.vector;
    info[5] = empty ? 0 : pl.grid;
    info[6] = empty ? 0 : ws_bytes_of(pl, o1, i1, esize, indices != 0);
    info[7] = pl.waves;
    return 0;
}

// Workspace of cme_reduce_dim, whatever the alignment of its operand.
CME_EXPORT int cme_reduce_dim_ws_bytes(long long outer, long long n, long long inner, int dtype, int indices,
                                       long long* nbytes) {
    if (outer < 0 || n < 0 || inner < 0 || !esize_of(dtype)) return (int)hipErrorInvalidValue;
    *nbytes = 0;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    const int esize = esize_of(dtype);
    const ll a = ws_bytes_of(scan_dim_plan(outer, n, inner, esize, true), outer, inner, esize, indices != 0);
    const ll b = ws_bytes_of(scan_dim_plan(outer, n, inner, esize, false), outer, inner, esize, indices != 0);
    *nbytes = a > b ? a : b;
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(reduce_dim_rows_f32, 256, reduce_rows_kernel<float, RedSum, kWaves>);
CME_REGISTER_KERNEL(reduce_dim_rows_wave_max_f64, 256, reduce_rows_kernel<double, RedMax, 1>);
CME_REGISTER_KERNEL(reduce_dim_rows_argmax_f32, 256, reduce_rows_kernel<float, RedArgMax, kWaves>);
CME_REGISTER_KERNEL(reduce_dim_rows_wave_argmin_i64, 256, reduce_rows_kernel<ll, RedArgMin, 1>);
CME_REGISTER_KERNEL(reduce_dim_cols_f32, 256, reduce_cols_kernel<float, RedSum, 4>);
CME_REGISTER_KERNEL(reduce_dim_cols_scalar_min_i64, 256, reduce_cols_kernel<ll, RedMin, 1>);
CME_REGISTER_KERNEL(reduce_dim_cols_argmax_f64, 256, reduce_cols_kernel<double, RedArgMax, 2>);
CME_REGISTER_KERNEL(reduce_dim_finish_argmax_f32, 256, reduce_finish_kernel<float, RedArgMax, true>);
CME_REGISTER_KERNEL(reduce_dim_finish_thread_f64, 256, reduce_finish_kernel<double, RedSum, false>);
