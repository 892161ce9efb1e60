// bincount: counts of the values 0 .. nbins-1 in UNSORTED integer data
// (slides/Lecture12 dense histogram, Lecture21 atomics), for uint8, int32 and
// int64 elements at element alignment, into int64 counts.
//
//  out[b] = #{i : x[i] == b}, 0 <= b < nbins. An element outside [0, nbins) is
//  not counted. The range test is made on the element widened to 64 bits, so an
//  int64 2^32 + 3 is out of range for nbins = 8 and never aliases bin 3.
//
// Regimes (cme_bincount_plan reports the one a shape gets):
//
//  lds     nbins <= W: every workgroup keeps a private table of 32-bit
//          counters in LDS, grid-strides over the input, counts with
//          non-returning LDS atomic adds and flushes each non-zero bin once
//          with one non-returning 64-bit global atomic add. Small tables are
//          replicated `copies` times (lane t counts into copy t % copies, copy
//          stride odd), so that lanes and waves holding one value do not
//          serialise on one LDS address.
//  window  nbins > W: the same kernel over the bin windows [k W, (k+1) W). The
//          grid is windows x input chunks; a workgroup counts only the
//          elements of its window, so the input is read once per window.
//  global  one non-returning 64-bit global atomic add per run of equal
//          neighbours straight into out.
//  sorted  histogram of the sorted copy (sort, then upper_bound differences):
//          composed by the caller from the library's sort and search; the
//          launcher refuses it.
//
// Loads: 16-byte lane vectors, kBcUnroll of them in flight per lane. Block 0
// of each window counts the elements before the first 16-byte aligned one and
// the ones after the last whole vector. Equal neighbours within a lane's
// vector are combined before the atomic, so sorted or constant input costs one
// add per vector.
//
// Why a 32-bit LDS counter cannot wrap: a counter of a workgroup's table is
// incremented at most once per element that workgroup reads. The plan gives a
// window at least (n >> 31) + 1 input chunks. A chunk's share is at most
// ceil(passes / chunks) passes of kBcPass vectors (at most 2^14 elements per
// pass) plus fewer than 32 head and tail elements, that is less than
// n / chunks + 2 * 2^14 + 32 < 2^31 + 2^15 + 32 < 2^32 elements. The copies of
// a table are summed in 64 bits. The knob bincount_maxblocks cannot lower the
// chunk count below that bound.
//
// No kernel here waits for another workgroup; integer counts are exact
// whatever the order of the atomics.
#include <climits>

#include "cme213/common.h"
#include "cme213/tuning.h"

using namespace cme;

namespace {

using ll = long long;
using ull = unsigned long long;

constexpr int kBcThreads = 256;
constexpr int kBcUnroll = 4;                     // 16-byte loads in flight per lane
constexpr int kBcPass = kBcThreads * kBcUnroll;  // vectors per workgroup pass
constexpr int kBcMaxW = 16384;                   // 32-bit counters of one table: 64 KiB of LDS
constexpr int kBcCopyWords = 4096;               // a replicated table stays within 16 KiB
constexpr int kBcMaxCopies = 32;
constexpr int kBcMaxWindows = 12;                // windows still worth re-reading the input (profiles/bincount.md):
constexpr int kBcMaxWindows64 = 20;              // 1- and 4-byte elements, 8-byte elements
constexpr ll kBcMaxChunks = 2048;                // workgroups of a launch (8 per CU), rule

enum { kBcRule = 0, kBcLds = 1, kBcWindow = 2, kBcGlobal = 3, kBcSorted = 4 };

template <typename T> __device__ __forceinline__ ll bc_widen(T v) { return (ll)v; }

// Adds `cnt` to the counter of value v where v - lo is in [0, wb): the
// comparison is unsigned on the 64-bit difference, so every negative v and
// every v below lo is far above wb.
struct BcLdsSink {
    uint32_t* table;  // this lane's copy
    ll lo;
    ull wb;
    __device__ __forceinline__ void add(ll v, uint32_t cnt) const {
        const ull d = (ull)v - (ull)lo;
        if (d < wb) __hip_atomic_fetch_add(&table[d], cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
};

struct BcGlobalSink {
    ull* out;
    ull nbins;
    __device__ __forceinline__ void add(ll v, uint32_t cnt) const {
        if ((ull)v < nbins) __hip_atomic_fetch_add(&out[(ull)v], (ull)cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
};

// The elements of one 16-byte vector, equal neighbours combined.
template <typename T, typename Sink>
__device__ __forceinline__ void bc_vector(const uint4& w, const Sink& sink) {
    constexpr int V = 16 / (int)sizeof(T);
    T e[V];
    __builtin_memcpy(e, &w, 16);
    ll cur = bc_widen(e[0]);
    uint32_t cnt = 1;
#pragma unroll
    for (int j = 1; j < V; ++j) {
        const ll v = bc_widen(e[j]);
        if (v == cur) {
            ++cnt;
        } else {
            sink.add(cur, cnt);
            cur = v;
            cnt = 1;
        }
    }
    sink.add(cur, cnt);
}

// Chunk `chunk` of `chunks` over x[0, n): the head before the first 16-byte
// aligned element and the tail after the last whole vector go to chunk 0,
// passes chunk, chunk + chunks, ... of kBcPass vectors to this one.
template <typename T, typename Sink>
__device__ __forceinline__ void bc_stream(const T* __restrict__ x, ll n, int chunk, int chunks, const Sink& sink) {
    constexpr int V = 16 / (int)sizeof(T);
    const int tid = threadIdx.x;
    ll head = (ll)(((16 - (uintptr_t)x % 16) % 16) / sizeof(T));
    if (head > n) head = n;
    const ll nvec = (n - head) / V;
    const ll tail0 = head + nvec * V;  // first element after the vectors
    if (chunk == 0) {                  // head + tail: fewer than 2 V <= 32 elements
        if (tid < head) sink.add(bc_widen(x[tid]), 1);
        const ll t = tail0 + (tid - head);
        if (tid >= head && t < n) sink.add(bc_widen(x[t]), 1);
    }
    const uint4* __restrict__ xv = reinterpret_cast<const uint4*>(x + head);
    const ll passes = (nvec + kBcPass - 1) / kBcPass;
    for (ll p = chunk; p < passes; p += chunks) {
        const ll v0 = p * kBcPass + tid;
        uint4 w[kBcUnroll];
#pragma unroll
        for (int u = 0; u < kBcUnroll; ++u) {
            const ll vi = v0 + (ll)u * kBcThreads;
            if (vi < nvec) w[u] = xv[vi];
        }
#pragma unroll
        for (int u = 0; u < kBcUnroll; ++u) {
            const ll vi = v0 + (ll)u * kBcThreads;
            if (vi < nvec) bc_vector<T>(w[u], sink);
        }
    }
}

// grid = windows x chunks; window k = blockIdx.x / chunks covers the bins
// [k W, min((k+1) W, nbins)). sh: copies tables of `stride` words.
template <typename T>
__global__ __launch_bounds__(kBcThreads) void bincount_lds_kernel(const T* __restrict__ x, ll n, ll nbins, int W,
                                                                  int copies, int stride, int chunks,
                                                                  ull* __restrict__ out) {
    extern __shared__ uint32_t bc_sh[];
    const int tid = threadIdx.x;
    const int window = (int)(blockIdx.x / (unsigned)chunks), chunk = (int)(blockIdx.x % (unsigned)chunks);
    const ll lo = (ll)window * W;
    const int wb = (int)(nbins - lo < W ? nbins - lo : W);
    const int words = copies * stride;
    for (int i = tid; i < words; i += kBcThreads) bc_sh[i] = 0;
    __syncthreads();
    const BcLdsSink sink{bc_sh + (tid & (copies - 1)) * stride, lo, (ull)wb};
    bc_stream<T>(x, n, chunk, chunks, sink);
    __syncthreads();
    for (int b = tid; b < wb; b += kBcThreads) {
        ull c = 0;
        for (int k = 0; k < copies; ++k) c += bc_sh[k * stride + b];
        if (c) __hip_atomic_fetch_add(&out[lo + b], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

template <typename T>
__global__ __launch_bounds__(kBcThreads) void bincount_global_kernel(const T* __restrict__ x, ll n, ll nbins,
                                                                     ull* __restrict__ out) {
    const BcGlobalSink sink{out, (ull)nbins};
    bc_stream<T>(x, n, (int)blockIdx.x, (int)gridDim.x, sink);
}

struct BincountPlan {
    int regime;  // kBcLds .. kBcSorted
    int W;       // bins of a window (lds: of the one table)
    ll windows;
    int copies;
    int stride;  // words between two copies
    ll chunks;   // input chunks = workgroups per window
    ll grid;
    ll lds_bytes;
    ll ws_bytes;
};

int pow2_floor(ll v) {
    int p = 1;
    while (2LL * p <= v) p *= 2;
    return p;
}

// 0, or hipErrorInvalidValue where the arguments are bad or the forced regime
// cannot run this shape.
int bincount_plan(ll n, int esize, ll nbins, BincountPlan& pl) {
    pl = BincountPlan{};
    if (n < 0 || nbins < 0 || (esize != 1 && esize != 4 && esize != 8)) return (int)hipErrorInvalidValue;
    const long forced = tune_get(kTuneBincountRegime);
    if (forced < kBcRule || forced > kBcSorted) return (int)hipErrorInvalidValue;
    long W = tune_get(kTuneBincountWindow);
    if (W <= 0 || W > kBcMaxW) W = kBcMaxW;
    const ll windows = nbins ? (nbins + W - 1) / W : 0;
    // the sorted composition goes through the library's sort and search: 32-
    // and 64-bit elements, bins a query of the element's type can name
    const bool can_sort = esize == 8 || (esize == 4 && nbins <= (ll)INT_MAX);
    int regime = (int)forced;
    if (regime == kBcRule) {
        // measured (profiles/bincount.md): a window costs one read of the input, and past the windows
        // the 32-bit sort beats one global atomic per element, which beats the 64-bit sort
        if (nbins <= W) regime = kBcLds;
        else if (windows <= (esize == 8 ? kBcMaxWindows64 : kBcMaxWindows)) regime = kBcWindow;
        else regime = esize == 4 && can_sort ? kBcSorted : kBcGlobal;
    }
    if (regime == kBcLds && nbins > W) return (int)hipErrorInvalidValue;
    if (regime == kBcSorted && !can_sort) return (int)hipErrorInvalidValue;
    pl.regime = regime;
    const int V = 16 / esize;
    const ll passes = (n / V + kBcPass - 1) / kBcPass;
    const ll min_chunks = (n >> 31) + 1;  // a share below 2^32 elements (header)
    if (regime == kBcSorted) {
        pl.ws_bytes = n * esize + 8 * (nbins + 1);  // the sorted copy and the bounds (the sort's own buffers apart)
        return 0;
    }
    if (regime == kBcGlobal) {
        ll cap = tune_get(kTuneBincountMaxBlocks);
        if (cap <= 0) cap = kBcMaxChunks;
        ll chunks = passes < cap ? passes : cap;
        if (chunks < 1) chunks = 1;
        pl.chunks = pl.grid = chunks;
        return 0;
    }
    pl.W = (int)W;
    pl.windows = windows;
    const ll wb = nbins < W ? nbins : W;  // bins of the widest window
    pl.copies = 1;
    if (wb >= 1 && (wb | 1) * 2 <= kBcCopyWords) {
        pl.copies = pow2_floor(kBcCopyWords / (wb | 1));
        if (pl.copies > kBcMaxCopies) pl.copies = kBcMaxCopies;
    }
    pl.stride = pl.copies > 1 ? (int)(wb | 1) : (int)wb;
    pl.lds_bytes = (ll)pl.copies * pl.stride * 4;
    ll cap = tune_get(kTuneBincountMaxBlocks);
    if (cap <= 0) cap = windows > 0 ? kBcMaxChunks / windows : kBcMaxChunks;
    if (cap < 1) cap = 1;
    ll chunks = passes < cap ? passes : cap;
    if (chunks < min_chunks) chunks = min_chunks;
    pl.chunks = chunks;
    pl.grid = windows * chunks;
    if (pl.grid > (ll)INT_MAX) return (int)hipErrorInvalidValue;
    return 0;
}

template <typename T>
int launch(const void* x, ll n, ll nbins, const BincountPlan& pl, ull* out, hipStream_t s) {
    if (pl.regime == kBcGlobal)
        hipLaunchKernelGGL((bincount_global_kernel<T>), dim3((unsigned)pl.grid), dim3(kBcThreads), 0, s, (const T*)x, n,
                           nbins, out);
    else
        hipLaunchKernelGGL((bincount_lds_kernel<T>), dim3((unsigned)pl.grid), dim3(kBcThreads), (size_t)pl.lds_bytes, s,
                           (const T*)x, n, nbins, pl.W, pl.copies, pl.stride, (int)pl.chunks, out);
    CME_LAUNCH_STATUS();
}

}  // namespace

// out[b] = number of elements of x[0, n) equal to b, 0 <= b < nbins (int64).
// esize: 1 uint8, 4 int32, 8 int64; x at element alignment. out is zeroed on
// `stream` and every launch goes there; nothing else happens on the host. A
// regime forced by the knob bincount_regime that cannot run the shape, and the
// sorted regime (which the caller composes), are errors.
CME_EXPORT int cme_bincount(const void* x, long long n, int esize, long long nbins, long long* out, void* stream) {
    BincountPlan pl;
    const int rc = bincount_plan(n, esize, nbins, pl);
    if (rc) return rc;
    if (pl.regime == kBcSorted) return (int)hipErrorInvalidValue;
    if (nbins == 0) return 0;
    if (!out || (n > 0 && !x) || (uintptr_t)x % (uintptr_t)esize) return (int)hipErrorInvalidValue;
    hipStream_t s = as_stream(stream);
    CME_TRY(hipMemsetAsync(out, 0, (size_t)nbins * sizeof(ll), s));
    if (n == 0) return 0;
    ull* o = reinterpret_cast<ull*>(out);
    if (esize == 1) return launch<uint8_t>(x, n, nbins, pl, o, s);
    if (esize == 4) return launch<int32_t>(x, n, nbins, pl, o, s);
    return launch<ll>(x, n, nbins, pl, o, s);
}

// How cme_bincount runs (n, esize, nbins) under the current knobs: info[0]
// regime (1 lds, 2 window, 3 global, 4 sorted), [1] W, the bins of a window,
// [2] windows, [3] copies of a workgroup's table, [4] workgroups, [5] LDS
// bytes per workgroup, [6] workspace bytes (sorted: the sorted copy and the
// bounds), [7] lanes per workgroup, [8] elements per 16-byte lane vector, [9]
// elements of one workgroup pass, [10] input chunks (workgroups per window).
CME_EXPORT int cme_bincount_plan(long long n, int esize, long long nbins, long long* info) {
    if (!info) return (int)hipErrorInvalidValue;
    BincountPlan pl;
    const int rc = bincount_plan(n, esize, nbins, pl);
    if (rc) return rc;
    const bool run = n > 0 && nbins > 0 && pl.regime != kBcSorted;
    info[0] = pl.regime;
    info[1] = pl.W;
    info[2] = pl.windows;
    info[3] = pl.copies;
    info[4] = run ? pl.grid : 0;
    info[5] = pl.lds_bytes;
    info[6] = pl.ws_bytes;
    info[7] = kBcThreads;
    info[8] = 16 / esize;
    info[9] = (ll)kBcPass * (16 / esize);
    info[10] = run ? pl.chunks : 0;
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(bincount_lds_u8, 256, bincount_lds_kernel<uint8_t>);
CME_REGISTER_KERNEL(bincount_lds_i32, 256, bincount_lds_kernel<int32_t>);
CME_REGISTER_KERNEL(bincount_lds_i64, 256, bincount_lds_kernel<long long>);
CME_REGISTER_KERNEL(bincount_global_u8, 256, bincount_global_kernel<uint8_t>);
CME_REGISTER_KERNEL(bincount_global_i32, 256, bincount_global_kernel<int32_t>);
CME_REGISTER_KERNEL(bincount_global_i64, 256, bincount_global_kernel<long long>);
