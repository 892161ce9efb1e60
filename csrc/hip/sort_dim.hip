// Stable sort along one dimension of a contiguous tensor seen as (outer, n,
// inner), element (o, i, j) at (o*n + i)*inner + j: every line (o, j) is sorted
// over i, and the result is the pair (values, int64 positions along n). Keys:
// uint32 / int32 / float32 / uint64 / int64 / float64 through the order codes
// of the 1-D sorts (rx_key_in, rx64_key_in: floats in IEEE total order), the
// code complemented for descending order, so equal keys keep their input order
// in both directions.
//
// Tile regime, the only one here (lines of n <= kSdTile keys; longer lines are
// composed from the 1-D sorts by the caller, ops/sort.py): a workgroup sorts a
// tile of L = min(kSdTile / n, 256, lines) whole lines in LDS, by the block
// radix sort of the merge sort's base case (ms_block_radix_kernel) carrying
// one packed word (line in tile << 16 | position in line) per key:
//
//   load    tile position p -> (line l, position j):
//             row form (inner == 1)  p = l*n + j: the tile is one contiguous
//                                    block of lc*n elements;
//             column form            p = j*lc + l: n rows of lc adjacent
//                                    columns of one `outer` slice, read in
//                                    pieces of lc contiguous elements
//           (lc <= L: the lines this tile really holds);
//   passes  4 or 8 stable 8-bit digit passes over the code, then, when L > 1,
//           one stable pass whose digit is l. After it line l occupies LDS
//           positions [l*n, (l+1)*n) in sorted order;
//   store   row form: positions [0, lc*n) straight out, values and indices
//           both coalesced. Column form: the same pieces of lc contiguous
//           elements as the loads, reading LDS transposed (line l's j-th key).
//           To keep that strided read off one bank when n is a multiple of 32,
//           the line pass of the column form rotates line l by l positions.
//
// Padding. A tile has 1024 * items slots (items = ceil(L*n / 1024), the same
// for every tile of a launch), of which the first cnt = lc*n hold keys; the
// others are padding with the all-ones code and line digit 255. Claim: after
// the last pass the keys occupy [0, cnt) and the padding [cnt, slots). Proof:
// the passes together are an LSD radix sort, so the final order is THE stable
// order by the composite (line digit, code), ties in load order. Padding has
// the largest value of every digit, so no key's composite exceeds it; a key
// can equal it -- uint32 0 descending, INT_MAX ascending, an all-mantissa +NaN,
// in line 255 of a full tile -- and then the tie is broken by load order, in
// which every padding slot comes after every key (p >= cnt, in both forms:
// that is why the column form lays a partial tile out by its own lc and not by
// L, which would interleave padding columns with real ones). Hence every key
// precedes every padding slot, by stability alone; no pass looks at validity.
//
// Sizes and occupancy. kSdTile = 8192 slots and 1024 lanes for both key
// widths; 8 items per lane. 32-bit keys: 32 KiB codes + 32 KiB packed words +
// 16 KiB per-wave digit counts = 80 KiB and <= 64 VGPRs: designed for two
// workgroups per CU (8 waves per SIMD), as the block sort it comes from.
// 64-bit keys: 64 + 32 + 16 = 112 KiB: one workgroup per CU (4 waves per
// SIMD, <= 128 VGPRs), as the 64-bit downsweep. L is capped at 256 so that one
// line pass always suffices; the cost is on very short lines: below n = 32 a
// tile holds 256*n < 8192 keys, and below n = 4 fewer than its 1024 lanes (n
// = 2: half the lanes sort padding). The launch scales `items` down with L*n,
// so a short tile does not run 8 items of padding per lane.
//
// Every index into global memory is 64-bit; tile-local ones fit 14 bits. No
// kernel waits for another workgroup; nothing here synchronises or allocates.
#include <climits>

#include "sort_kernels.h"

namespace {

using ll = long long;
constexpr int kSdThreads = 1024;
constexpr int kSdWaves = kSdThreads / kWave;
constexpr int kSdItems = 8;
constexpr int kSdTile = kSdThreads * kSdItems;  // 8192 slots
constexpr int kSdMaxLines = 256;                // one 8-bit line digit
constexpr uint32_t kSdPadWord = (uint32_t)(kSdMaxLines - 1) << 16;

template <typename K> __device__ __forceinline__ K sd_code_in(K k, int mode);
template <> __device__ __forceinline__ uint32_t sd_code_in<uint32_t>(uint32_t k, int mode) {
    const uint32_t c = rx_key_in(k, mode & 3);
    return (mode & 4) ? ~c : c;
}
template <> __device__ __forceinline__ uint64_t sd_code_in<uint64_t>(uint64_t k, int mode) {
    return rx64_key_in(k, mode);
}
__device__ __forceinline__ uint32_t sd_code_out(uint32_t c, int mode) {
    return rx_key_out((mode & 4) ? ~c : c, mode & 3);
}
__device__ __forceinline__ uint64_t sd_code_out(uint64_t c, int mode) { return rx64_key_out(c, mode); }

// floor(p / d) for p < 2^14 and 1 <= d <= 2^13 by the magic m = floor(2^32 /
// d) + 1 = 2^32 / d + e, 0 < e <= 1: p*m / 2^32 = p/d + p*e / 2^32, and the
// excess is below 2^-18 while p/d is at least 1/d >= 2^-13 short of the next
// integer. d == 1 has no 32-bit magic.
__device__ __forceinline__ uint32_t sd_div(uint32_t p, uint32_t magic, uint32_t d) {
    return d == 1 ? p : __umulhi(p, magic);
}
uint32_t sd_magic(ll d) { return d <= 1 ? 0u : (uint32_t)((1ull << 32) / (unsigned long long)d) + 1u; }

// K: the code type (uint32_t / uint64_t). RANK: kRankLanes or kRankMatch.
// mode: bits 0-1 key kind (0 unsigned, 1 signed, 2 float), bit 2 descending.
// L: lines per full tile; tps: tiles per `outer` slice (column form); magic_n,
// magic_l, magic_last: sd_magic of n, of L and of the column count of a
// slice's last tile. `lines`: outer (row form).
template <typename K, int RANK>
__global__ __launch_bounds__(kSdThreads, sizeof(K) == 4 ? 8 : 4) void sort_dim_tile_kernel(
    const K* __restrict__ in, K* __restrict__ values, ll* __restrict__ indices, ll lines, int n, ll inner, int L,
    int tps, int items, int mode, uint32_t magic_n, uint32_t magic_l, uint32_t magic_last) {
    constexpr int NW = kSdWaves, NT = kSdThreads, ITEMS = kSdItems;
    constexpr int KP = (int)sizeof(K);  // digit passes over the code
    __shared__ K s_keys[kSdTile];
    __shared__ uint32_t s_pay[kSdTile];
    __shared__ uint32_t s_whist[NW][kBins];
    uint32_t* s_tmp = s_pay;  // the block scan's wave totals (s_pay is idle between reload and scatter)
    const int tid = threadIdx.x, lane = lane_id(), wid = tid / kWave;
    const bool col = inner > 1;
    ll g0;         // global index of the tile's (l = 0, j = 0)
    int lc;        // lines of this tile
    uint32_t mlc;  // sd_magic(lc)
    if (!col) {
        const ll l0 = (ll)blockIdx.x * L;
        lc = (int)(lines - l0 < L ? lines - l0 : L);
        g0 = l0 * n;
        mlc = 0;
    } else {
        const ll o = blockIdx.x / (unsigned)tps;
        const ll c0 = (ll)(blockIdx.x - (unsigned)o * (unsigned)tps) * L;
        lc = (int)(inner - c0 < L ? inner - c0 : L);
        g0 = o * n * inner + c0;
        mlc = lc == L ? magic_l : magic_last;
    }
    const uint32_t cnt = (uint32_t)lc * (uint32_t)n;
    const int wbase = wid * (kWave * items);  // wave-striped items: item k of lane l is slot wbase + k*64 + l
    K key[ITEMS];
    uint32_t pay[ITEMS], rank[ITEMS];
#pragma unroll
    for (int k = 0; k < ITEMS; ++k) {
        key[k] = ~(K)0;
        pay[k] = kSdPadWord;
        rank[k] = 0;
        if (k < items) {
            const uint32_t i = (uint32_t)(wbase + k * kWave + lane);
            if (i < cnt) {
                uint32_t l, j;
                ll g;
                if (!col) {
                    l = sd_div(i, magic_n, (uint32_t)n);
                    j = i - l * (uint32_t)n;
                    g = g0 + i;
                } else {
                    j = sd_div(i, mlc, (uint32_t)lc);
                    l = i - j * (uint32_t)lc;
                    g = g0 + (ll)j * inner + l;
                }
                key[k] = sd_code_in<K>(in[g], mode);
                pay[k] = (l << 16) | j;
            }
        }
    }
    const int npass = KP + (L > 1 ? 1 : 0);
    for (int p = 0; p < npass; ++p) {
        const bool linep = p >= KP;
        const int shift = linep ? 0 : p * kRadixBits;
        auto digit = [&](int k) {
            return linep ? (pay[k] >> 16) & (uint32_t)(kBins - 1) : (uint32_t)(key[k] >> shift) & (uint32_t)(kBins - 1);
        };
#pragma unroll
        for (int w = 0; w < NW * kBins / NT; ++w) (&s_whist[0][0])[w * NT + tid] = 0u;
        __syncthreads();
        // stable in-wave ranks in (k, lane) order = slot order; every lane holds
        // a slot (padding included), so the whole wave takes part in each step
        if constexpr (RANK == kRankLanes) {
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                if (k < items) {
                    const uint32_t d = digit(k);
                    const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
                    if (__ballot(d != d0) == 0) {  // one digit in the wave: one atomic
                        uint32_t b = 0;
                        if (lane == 0) b = atomicAdd(&s_whist[wid][d0], (uint32_t)kWave);
                        rank[k] = (uint32_t)__builtin_amdgcn_readfirstlane((int)b) + (uint32_t)lane;
                    } else {
                        rank[k] = atomicAdd(&s_whist[wid][d], 1u);  // same-address lanes resolve in lane order
                    }
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                if (k < items) {
                    const uint32_t d = digit(k);
                    const uint64_t peers = match_digit(d, true);
                    const uint32_t below = (uint32_t)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
                    const uint32_t prev = s_whist[wid][d];
                    rank[k] = prev + below;
                    if (below == 0) s_whist[wid][d] = prev + (uint32_t)__builtin_popcountll(peers);
                    __builtin_amdgcn_sched_barrier(0);  // keep each item's ballots next to its LDS update
                }
            }
        }
        __syncthreads();
        // per digit: exclusive prefix over the waves, then the block scan of the digit totals
        uint32_t run = 0;
        if (tid < kBins) {
#pragma unroll
            for (int w = 0; w < NW; ++w) {
                const uint32_t c = s_whist[w][tid];
                s_whist[w][tid] = run;
                run += c;
            }
        }
        uint32_t tot;
        const uint32_t ex = block_exclusive_scan<NW>(tid < kBins ? run : 0u, s_tmp, tot, OpAdd());
        if (tid < kBins) {
#pragma unroll
            for (int w = 0; w < NW; ++w) s_whist[w][tid] += ex;
        }
        __syncthreads();
        // column form, line pass (the last one): a key of line d lands in
        // [d*n, (d+1)*n), see the header; it goes to that line's slot (r + d)
        // mod n instead of r, so the transposed read of the store walks the
        // banks. Padding (pos >= cnt) stays where it is.
        const bool rot = col && linep;
#pragma unroll
        for (int k = 0; k < ITEMS; ++k) {
            if (k < items) {
                const uint32_t d = digit(k);
                uint32_t pos = s_whist[wid][d] + rank[k];
                if (rot && pos < cnt) {
                    const uint32_t r = pos - d * (uint32_t)n + d;  // < n + 256
                    pos = d * (uint32_t)n + r - (uint32_t)n * sd_div(r, magic_n, (uint32_t)n);
                }
                s_keys[pos] = key[k];
                s_pay[pos] = pay[k];
            }
        }
        __syncthreads();
        if (p + 1 < npass) {
#pragma unroll
            for (int k = 0; k < ITEMS; ++k) {
                if (k < items) {
                    key[k] = s_keys[wbase + k * kWave + lane];
                    pay[k] = s_pay[wbase + k * kWave + lane];
                }
            }
        }
    }
    if (!col) {
        for (uint32_t i = tid; i < cnt; i += NT) {
            values[g0 + i] = sd_code_out(s_keys[i], mode);
            indices[g0 + i] = (ll)(s_pay[i] & 0xffffu);
        }
    } else {
        const bool rotated = L > 1;  // the line pass ran
        for (uint32_t q = tid; q < cnt; q += NT) {
            const uint32_t j = sd_div(q, mlc, (uint32_t)lc);
            const uint32_t c = q - j * (uint32_t)lc;
            uint32_t r = j;
            if (rotated) {
                r = j + c;
                r -= (uint32_t)n * sd_div(r, magic_n, (uint32_t)n);
            }
            const uint32_t src = c * (uint32_t)n + r;
            const ll g = g0 + (ll)j * inner + c;
            values[g] = sd_code_out(s_keys[src], mode);
            indices[g] = (ll)(s_pay[src] & 0xffffu);
        }
    }
}

int esize_of(int dtype) { return dtype >= 0 && dtype <= 2 ? 4 : dtype >= 3 && dtype <= 5 ? 8 : 0; }

struct SortDimPlan {
    int form;    // 0 a single line, 1 row (inner == 1), 2 column
    int regime;  // 0 tile kernel, 1 composed from the 1-D sorts by the caller
    int lines;   // L: lines per full tile (0: composed)
    int tps;     // column form: tiles per `outer` slice
    int items;   // slots per lane
    int passes;  // digit passes, the line pass included
    ll tiles;    // workgroups
};

SortDimPlan sort_dim_plan(ll outer, ll n, ll inner, int esize) {
    SortDimPlan pl{};
    pl.form = outer == 1 && inner == 1 ? 0 : inner == 1 ? 1 : 2;
    long max_n = cme::tune_get(cme::kTuneSortDimMaxN);
    if (max_n <= 0 || max_n > kSdTile) max_n = kSdTile;
    pl.regime = n <= max_n ? 0 : 1;
    if (pl.regime == 1 || n <= 0) return pl;
    ll L = kSdTile / n < kSdMaxLines ? kSdTile / n : kSdMaxLines;
    const ll avail = inner == 1 ? outer : inner;  // lines one tile can draw from
    if (L > avail) L = avail > 0 ? avail : 1;      // (an empty operand still gets a plan: the info query)
    pl.lines = (int)L;
    pl.tps = inner == 1 ? 1 : (int)((inner + L - 1) / L);
    pl.items = (int)((L * n + kSdThreads - 1) / kSdThreads);
    pl.passes = esize + (L > 1 ? 1 : 0);
    pl.tiles = inner == 1 ? (outer + L - 1) / L : outer * pl.tps;
    return pl;
}

bool bad_args(ll outer, ll n, ll inner, int dtype) { return outer < 0 || n < 0 || inner < 0 || !esize_of(dtype); }

template <typename K>
int launch(const void* in, void* values, void* indices, ll outer, ll n, ll inner, const SortDimPlan& pl, int mode,
           bool lanes, hipStream_t s) {
    const ll L = pl.lines;
    const ll last = inner - (ll)(pl.tps - 1) * L;  // columns of a slice's last tile
    const dim3 grid((unsigned)pl.tiles), block(kSdThreads);
    if (lanes)
        hipLaunchKernelGGL((sort_dim_tile_kernel<K, kRankLanes>), grid, block, 0, s, (const K*)in, (K*)values,
                           (ll*)indices, outer, (int)n, inner, (int)L, pl.tps, pl.items, mode, sd_magic(n), sd_magic(L),
                           sd_magic(last));
    else
        hipLaunchKernelGGL((sort_dim_tile_kernel<K, kRankMatch>), grid, block, 0, s, (const K*)in, (K*)values,
                           (ll*)indices, outer, (int)n, inner, (int)L, pl.tps, pl.items, mode, sd_magic(n), sd_magic(L),
                           sd_magic(last));
    CME_LAUNCH_STATUS();
}

}  // namespace

extern "C" int cme_radix_lane_order(int check);  // sort.hip

// Stable sort of (outer, n, inner) along n by the tile kernel: out_values gets
// the sorted lines in the operand's type and layout, out_indices the int64
// position along n every output element came from. dtype: 0 uint32, 1 int32,
// 2 float32, 3 uint64, 4 int64, 5 float64. Only element alignment is assumed.
// A shape that cme_sort_dim_info puts in the composed regime (n above the
// tile, or above the knob sort_dim_max_n) is an error: the caller composes it
// from the 1-D sorts. Ranks: lane-ordered LDS atomics where the device passed
// cme_radix_lane_order and the knob sort_dim_lanes is set, ballot match
// otherwise. Every launch goes on `stream`.
CME_EXPORT int cme_sort_dim(const void* in, void* out_values, void* out_indices, long long outer, long long n,
                            long long inner, int dtype, int descending, void* stream) {
    if (bad_args(outer, n, inner, dtype)) return (int)hipErrorInvalidValue;
    if (outer == 0 || n == 0 || inner == 0) return 0;
    if (!in || !out_values || !out_indices) return (int)hipErrorInvalidValue;
    const SortDimPlan pl = sort_dim_plan(outer, n, inner, esize_of(dtype));
    if (pl.regime != 0 || pl.tiles > (ll)INT_MAX) return (int)hipErrorInvalidValue;
    hipStream_t s = as_stream(stream);
    bool lanes = cme::tune_get(cme::kTuneSortDimLanes) != 0;
    if (lanes) {  // lane-order ranks: only on a device that passed the check
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
        lanes = cme_radix_lane_order(capturing ? 0 : 1) != 0;
    }
    const int mode = dtype % 3 | (descending ? 4 : 0);
    if (dtype < 3) return launch<uint32_t>(in, out_values, out_indices, outer, n, inner, pl, mode, lanes, s);
    return launch<uint64_t>(in, out_values, out_indices, outer, n, inner, pl, mode, lanes, s);
}

// How sort(dim=) runs (outer, n, inner): info[0] form (0 a single line, 1
// row, 2 column), [1] regime (0 tile kernel, 1 composed), [2] the tile T in
// keys (the longest line the kernel can take), [3] lines per tile, [4] digit
// passes (the line pass included), [5] workgroups, [6] slots per lane, [7]
// lanes per workgroup. [3]-[6] are 0 in the composed regime and for an empty
// operand.
CME_EXPORT int cme_sort_dim_info(long long outer, long long n, long long inner, int dtype, long long* info) {
    if (bad_args(outer, n, inner, dtype) || !info) return (int)hipErrorInvalidValue;
    const bool empty = outer == 0 || n == 0 || inner == 0;
    const SortDimPlan pl = sort_dim_plan(outer, n, inner, esize_of(dtype));
    const bool run = !empty && pl.regime == 0;
    info[0] = pl.form;
    info[1] = pl.regime;
    info[2] = kSdTile;
    info[3] = run ? pl.lines : 0;
    info[4] = run ? pl.passes : 0;
    info[5] = run ? pl.tiles : 0;
    info[6] = run ? pl.items : 0;
    info[7] = kSdThreads;
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(sort_dim_tile_u32, 1024, sort_dim_tile_kernel<uint32_t, kRankLanes>);
CME_REGISTER_KERNEL(sort_dim_tile_u32_match, 1024, sort_dim_tile_kernel<uint32_t, kRankMatch>);
CME_REGISTER_KERNEL(sort_dim_tile_u64, 1024, sort_dim_tile_kernel<uint64_t, kRankLanes>);
CME_REGISTER_KERNEL(sort_dim_tile_u64_match, 1024, sort_dim_tile_kernel<uint64_t, kRankMatch>);
