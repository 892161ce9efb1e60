// LSD radix sort (8-bit digits) of 64-bit keys for gfx950: uint64, int64 and
// float64 keys, ascending or descending, with optional 4- or 8-byte values.
//
// The same reduce-then-scan pass as the 32-bit sort (sort.hip: upsweep ->
// one-launch count scan -> downsweep; no in-launch hand-offs, nothing waits
// on another block), over 8-byte keys:
//   K1 upsweep  : block b histograms its chunk with 16-byte loads (two keys
//                 per load, several in flight), one uniformity check per load
//   K2 scan     : radix_scan_kernel of the 32-bit sort, unchanged (counts and
//                 positions stay 32-bit: n < 2^32)
//   K3 downsweep: 8192-key tiles (1024 lanes x 8 keys), stable in-wave ranks by
//                 one returning LDS atomic per key (kRankLanes) or the ballot
//                 match, reorder by digit in LDS, contiguous digit runs out;
//                 the next tile's loads are in flight during the stores; a
//                 pass in which one digit holds every key is a straight copy.
// Keys become order codes on the first pass's loads and keys again on the last
// pass's stores: int64 flips the sign bit, float64 takes the IEEE total order
// (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN), descending complements
// the code -- equal keys then keep their input order, as in a stable
// descending sort (not the flipped ascending result).
//
// LDS layout: ONE 8-byte array per tile (keys) and one array of the value
// width, not separate low / high 4-byte planes. Per wave instruction the
// 8-byte store costs ~6 cycles against 2 x 4 for two 4-byte stores, the
// 8-byte read 2 against 2 x 2 (MI355X_MICROARCH.md, LDS table), and the
// planes double the address arithmetic of the scattered reorder; both
// layouts see the same 32-bank conflicts on scattered positions (16 lanes x 2
// banks against 32 lanes x 1 bank per group).
// Tile: 8192 keys = 1024 lanes x 8 items. 64 KiB of keys + 0 / 32 / 64 KiB of
// values + 16 KiB of per-wave counts + 3 KiB: 83 / 115 / 147 KiB, one block
// of 16 waves per CU; 8 items per lane keep keys, values and ranks (the
// prefetched tile reuses the key / value registers, dead after the reorder)
// inside the 128 VGPRs that 4 waves per SIMD allow. Measured against
// 4096-key tiles (512 lanes, two to three blocks per CU): digit runs of 32
// keys = 256 B instead of 128 B; in one A/B call int64 + int64 values 16M
// 1.43 -> 1.33 ms, 48M 4.75 -> 4.17, keys only 48M 2.58 -> 2.37, 16M 0.78 ->
// 0.83 (profiles/sort64_r7.md; run-to-run spread at 48M is about 7 %).
#include "sort_kernels.h"

namespace {

constexpr int k64Threads = 1024;
constexpr int k64Waves = k64Threads / kWave;
constexpr int k64Items = 8;
constexpr int k64Tile = k64Threads * k64Items;  // 8192 keys
constexpr int kUp64Threads = 256;
// (rx64_key_in / rx64_key_out: sort_kernels.h, shared with sort_dim.hip)
__device__ __forceinline__ uint32_t digit64(uint64_t k, int shift) { return (uint32_t)(k >> shift) & (kBins - 1); }

// Keys are 8-byte aligned; a view (keys[1:]) need not be 16-byte aligned.
// Every chunk starts an even number of keys after keys[0], so all blocks see
// the same misalignment: a misaligned chunk takes its first key alone, then
// 16-byte loads from the aligned key after it, and an odd last key alone.
template <int UNR>
__global__ __launch_bounds__(kUp64Threads) void radix64_upsweep_kernel(const uint64_t* __restrict__ keys, long long n,
                                                                       long long chunk, int shift, int nblocks,
                                                                       uint32_t* __restrict__ counts, int mode) {
    __shared__ uint32_t hist[kBins];
    for (int i = threadIdx.x; i < kBins; i += kUp64Threads) hist[i] = 0;
    __syncthreads();
    const long long b0 = (long long)blockIdx.x * chunk;
    const long long b1 = b0 + chunk < n ? b0 + chunk : n;
    const int lane = lane_id();
    // a wave whose active lanes share one digit adds once (same-address LDS
    // atomics serialise: the high digits of small keys)
    auto add = [&](uint64_t k) {
        const uint32_t d = digit64(rx64_key_in(k, mode), shift);
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
        if (__ballot(d != d0) == 0) {
            const uint64_t act = __ballot(true);
            if (lane == (int)__builtin_ctzll(act)) atomicAdd(&hist[d0], (uint32_t)__builtin_popcountll(act));
        } else {
            atomicAdd(&hist[d], 1u);
        }
    };
    // the two keys of a 16-byte load: one uniformity check for both
    auto add2 = [&](ulonglong2 v) {
        const uint32_t dx = digit64(rx64_key_in(v.x, mode), shift), dy = digit64(rx64_key_in(v.y, mode), shift);
        const uint32_t d0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)dx);
        if (__ballot((dx ^ d0) | (dy ^ d0)) == 0) {
            const uint64_t act = __ballot(true);
            if (lane == (int)__builtin_ctzll(act)) atomicAdd(&hist[d0], 2u * (uint32_t)__builtin_popcountll(act));
        } else {
            atomicAdd(&hist[dx], 1u);
            atomicAdd(&hist[dy], 1u);
        }
    };
    const long long head = (((uintptr_t)(keys + b0) & 15u) != 0 && b0 < b1) ? 1 : 0;
    const long long v0 = b0 + head;                       // first key of the 16-byte loads
    const long long npair = b1 > v0 ? (b1 - v0) / 2 : 0;  // pairs [v0 + 2p, v0 + 2p + 2)
    const ulonglong2* kv = reinterpret_cast<const ulonglong2*>(keys + v0);
    long long p = threadIdx.x;
    for (; p + (long long)(UNR - 1) * kUp64Threads < npair; p += (long long)UNR * kUp64Threads) {
        ulonglong2 v[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = kv[p + (long long)u * kUp64Threads];
#pragma unroll
        for (int u = 0; u < UNR; ++u) add2(v[u]);
    }
    for (; p < npair; p += kUp64Threads) add2(kv[p]);
    if (threadIdx.x == 0 && head) add(keys[b0]);
    if (threadIdx.x == kWave && v0 + 2 * npair < b1) add(keys[b1 - 1]);
    __syncthreads();
    for (int d = threadIdx.x; d < kBins; d += kUp64Threads) counts[(size_t)d * nblocks + blockIdx.x] = hist[d];
}

template <int VB> struct Val64 { using T = uint32_t; };
template <> struct Val64<8> { using T = uint64_t; };

// VB: bytes per value (0 none, 4, 8). RANK: kRankLanes or kRankMatch.
template <int VB, int RANK>
__global__ __launch_bounds__(k64Threads, 1) void radix64_downsweep_kernel(
    const uint64_t* __restrict__ keys_in, uint64_t* __restrict__ keys_out, const void* __restrict__ vals_in_,
    void* __restrict__ vals_out_, long long n, long long chunk, int shift, int nblocks,
    const uint32_t* __restrict__ prefix, const uint32_t* __restrict__ totals, int mode_in, int mode_out) {
    using VT = typename Val64<VB>::T;
    constexpr bool HAS_VALUES = VB != 0;
    const VT* __restrict__ vals_in = static_cast<const VT*>(vals_in_);
    VT* __restrict__ vals_out = static_cast<VT*>(vals_out_);
    const int tid = threadIdx.x;
    __shared__ uint64_t s_keys[k64Tile];
    __shared__ VT s_vals[HAS_VALUES ? k64Tile : 1];
    __shared__ uint32_t s_whist[k64Waves][kBins];  // per-wave running counts, then exclusive prefixes
    __shared__ uint32_t s_tile_off[kBins];         // exclusive prefix of tile digit counts
    __shared__ uint32_t s_base[kBins];             // global position of the next key of each digit
    __shared__ uint32_t s_gdiff[kBins];            // s_base - s_tile_off: tile index -> global position
    __shared__ uint32_t s_t[k64Waves];
    __shared__ int s_identity;
    const int lane = lane_id();
    const int wid = tid / kWave;
    const long long b0 = (long long)blockIdx.x * chunk;
    const long long b1 = b0 + chunk < n ? b0 + chunk : n;
    {  // digit bases: scan of the digit totals + this block's row prefix
        uint32_t tot;
        const uint32_t td = tid < kBins ? totals[tid] : 0u;
        if (tid == 0) s_identity = 0;
        const uint32_t db = block_exclusive_scan<k64Waves>(td, s_t, tot, OpAdd());
        if (tid < kBins) s_base[tid] = db + prefix[(size_t)tid * nblocks + blockIdx.x];
        if (tid < kBins && td == (uint32_t)n) s_identity = 1;  // every key has this digit
        lds_bcast_sync();
    }
    if (s_identity) {
        // one digit holds every key: the stable pass is the identity
        // permutation (the high bytes of index-like keys) -- a straight
        // copy, with the first / last pass's key transforms
        constexpr int U = 4;
        long long i = b0 + tid;
        for (; i + (U - 1) * k64Threads < b1; i += U * k64Threads) {
            uint64_t k[U];
            VT v[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                k[u] = keys_in[i + u * k64Threads];
                if constexpr (HAS_VALUES) v[u] = vals_in[i + u * k64Threads];
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                keys_out[i + u * k64Threads] = rx64_key_out(rx64_key_in(k[u], mode_in), mode_out);
                if constexpr (HAS_VALUES) vals_out[i + u * k64Threads] = v[u];
            }
        }
        for (; i < b1; i += k64Threads) {
            keys_out[i] = rx64_key_out(rx64_key_in(keys_in[i], mode_in), mode_out);
            if constexpr (HAS_VALUES) vals_out[i] = vals_in[i];
        }
        return;
    }

    // wave-striped: item k of lane l = key t0 + wid*512 + k*64 + l (memory order = (k, l))
    uint64_t key[k64Items];
    VT val[HAS_VALUES ? k64Items : 1];
    uint32_t rank[k64Items];
    auto items_of = [&](long long t0) {
        const long long rem = b1 - (t0 + wid * (kWave * k64Items) + lane);
        return rem <= 0 ? 0 : (rem >= (long long)kWave * k64Items ? k64Items : (int)((rem + kWave - 1) / kWave));
    };
    auto load_tile = [&](long long t0) {
        const long long base = t0 + wid * (kWave * k64Items) + lane;
        const int nk = items_of(t0);
#pragma unroll
        for (int k = 0; k < k64Items; ++k) {
            key[k] = k < nk ? keys_in[base + k * kWave] : ~0ull;
            if constexpr (HAS_VALUES) val[k] = k < nk ? vals_in[base + k * kWave] : (VT)0;
        }
    };
    if (b0 < b1) load_tile(b0);
    for (long long t0 = b0; t0 < b1; t0 += k64Tile) {
#pragma unroll
        for (int i = 0; i < k64Waves * kBins / k64Threads; ++i) (&s_whist[0][0])[i * k64Threads + tid] = 0u;
        const int nk = items_of(t0);
        __syncthreads();
        if (mode_in) {  // an invalid item's code is never ranked (outside the valid ballot)
#pragma unroll
            for (int k = 0; k < k64Items; ++k) key[k] = rx64_key_in(key[k], mode_in);
        }
        if constexpr (RANK == kRankLanes) {
#pragma unroll
            for (int k = 0; k < k64Items; ++k) {
                const bool ok = k < nk;
                const uint32_t d = digit64(key[k], shift);
                const uint64_t act = __ballot(ok);
                if (act == 0) {
                    rank[k] = 0xffffffffu;
                    continue;
                }
                const int first = (int)__builtin_ctzll(act);
                const uint32_t d0 = (uint32_t)__builtin_amdgcn_readlane((int)d, first);
                if (__ballot(ok && d != d0) == 0) {  // one digit: one atomic, ranks by lane count
                    uint32_t base = 0;
                    if (lane == first) base = atomicAdd(&s_whist[wid][d0], (uint32_t)__builtin_popcountll(act));
                    base = (uint32_t)__builtin_amdgcn_readlane((int)base, first);
                    const uint32_t below = (uint32_t)__builtin_popcountll(act & ((1ull << lane) - 1ull));
                    rank[k] = ok ? base + below : 0xffffffffu;
                } else {
                    uint32_t old = 0xffffffffu;
                    if (ok) old = atomicAdd(&s_whist[wid][d], 1u);  // same-address lanes resolve in lane order
                    rank[k] = old;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < k64Items; ++k) {
                const bool ok = k < nk;
                const uint32_t d = digit64(key[k], shift);
                const uint64_t peers = match_digit(d, ok);
                const uint32_t below = (uint32_t)__builtin_popcountll(peers & ((1ull << lane) - 1ull));
                const uint32_t prev = ok ? s_whist[wid][d] : 0u;
                rank[k] = ok ? prev + below : 0xffffffffu;
                // the lowest lane of each peer group publishes the new running count
                if (ok && below == 0) s_whist[wid][d] = prev + (uint32_t)__builtin_popcountll(peers);
                __builtin_amdgcn_sched_barrier(0);  // keep each item's ballots next to its LDS update
            }
        }
        __syncthreads();
        // per digit: exclusive prefix across waves, tile totals
        if (tid < kBins) {
            uint32_t run = 0;
#pragma unroll
            for (int w = 0; w < k64Waves; ++w) {
                const uint32_t c = s_whist[w][tid];
                s_whist[w][tid] = run;
                run += c;
            }
            s_tile_off[tid] = run;  // tile count (made exclusive below)
        }
        __syncthreads();
        {  // exclusive scan of the 256 tile counts
            uint32_t tot;
            const uint32_t c = tid < kBins ? s_tile_off[tid] : 0u;
            const uint32_t ex = block_exclusive_scan<k64Waves>(c, s_t, tot, OpAdd());
            __syncthreads();
            if (tid < kBins) {
                s_tile_off[tid] = ex;
                s_gdiff[tid] = s_base[tid] - ex;
                // fold the tile offset into every wave's prefix: one LDS read per key below
#pragma unroll
                for (int w = 0; w < k64Waves; ++w) s_whist[w][tid] += ex;
            }
        }
        __syncthreads();
        // reorder the tile by digit in LDS
#pragma unroll
        for (int k = 0; k < k64Items; ++k) {
            if (rank[k] != 0xffffffffu) {
                const uint32_t d = digit64(key[k], shift);
                const uint32_t pos = s_whist[wid][d] + rank[k];
                s_keys[pos] = key[k];
                if constexpr (HAS_VALUES) s_vals[pos] = val[k];
            }
        }
        __syncthreads();
        if (t0 + k64Tile < b1) load_tile(t0 + k64Tile);  // in flight during the stores
        const int tile_n = (int)((b1 - t0) < k64Tile ? (b1 - t0) : k64Tile);
        // the key transform only on the last pass (a uniform branch)
        auto store_tile = [&](int mo) {
#pragma unroll 4  // four independent LDS read chains in flight per lane (kv 16M 1.48 -> 1.33 ms)
            for (int i = tid; i < tile_n; i += k64Threads) {
                const uint64_t k = s_keys[i];
                const uint32_t d = digit64(k, shift);
                const uint32_t g = s_gdiff[d] + (uint32_t)i;
                keys_out[g] = mo ? rx64_key_out(k, mo) : k;
                if constexpr (HAS_VALUES) vals_out[g] = s_vals[i];
            }
        };
        if (mode_out == 0)
            store_tile(0);
        else
            store_tile(mode_out);
        __syncthreads();
        // advance the per-digit bases by this tile's counts
        if (tid < kBins) {
            const uint32_t next = tid + 1 < kBins ? s_tile_off[tid + 1] : (uint32_t)tile_n;
            s_base[tid] += next - s_tile_off[tid];
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int cme_radix_lane_order(int check);  // sort.hip

// Downsweep tile of the 64-bit sort, in keys.
CME_EXPORT int cme_radix_sort64_tile() { return k64Tile; }

// LSD radix sort of n 64-bit keys from `in` (not modified) into `out` over
// bits [bit0, bit1), ping-ponging through `tmp` so that the last pass writes
// out; values (val_bytes 4 or 8 each; 0 = none) likewise. mode: bits 0-1 key
// kind (0 uint64, 1 int64, 2 float64), bit 2 descending. ws:
// cme_radix_ws_bytes(n) bytes. Every launch goes on `stream`; no host
// synchronisation, no allocation. Honours the knobs radix_maxblocks (grid cap)
// and bit 3 of radix_ds (lane-order ranks; ballot match otherwise, and on a
// device that did not pass cme_radix_lane_order).
CME_EXPORT int cme_radix_sort64(const uint64_t* in, uint64_t* out, uint64_t* tmp, const void* vin, void* vout,
                                void* vtmp, long long n, int mode, int val_bytes, int bit0, int bit1, void* ws,
                                void* stream) {
    hipStream_t s = as_stream(stream);
    if (n <= 0) return 0;
    if (bit0 < 0 || bit1 > 64 || bit1 <= bit0 || mode < 0 || mode > 7 || (mode & 3) == 3 ||
        (val_bytes != 0 && val_bytes != 4 && val_bytes != 8) || (val_bytes != 0) != (vin != nullptr) ||
        (vin != nullptr) != (vout != nullptr) || (vin && !vtmp) || n >= (1ll << 32))
        return (int)hipErrorInvalidValue;
    bool lanes = (cme::tune_get(cme::kTuneRadixDS) & 8) != 0;
    if (lanes) {  // lane-order ranks: only on a device that passed the check
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const bool capturing = hipStreamIsCapturing(s, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone;
        lanes = cme_radix_lane_order(capturing ? 0 : 1) != 0;
    }
    const long long tiles = (n + k64Tile - 1) / k64Tile;
    long cap = cme::tune_get(cme::kTuneRadixMaxBlocks);
    cap = cap < 1 ? 1 : (cap > kMaxRadixBlocks ? kMaxRadixBlocks : cap);
    int nb = tiles < cap ? (int)tiles : (int)cap;
    const long long chunk = ((tiles + nb - 1) / nb) * k64Tile;
    nb = (int)((n + chunk - 1) / chunk);
    uint32_t* counts = (uint32_t*)ws;
    uint32_t* totals = counts + (size_t)nb * kBins;
    const int npass = (bit1 - bit0 + kRadixBits - 1) / kRadixBits;
    const uint64_t* ki = in;
    const void* vi = vin;
    for (int p = 0; p < npass; ++p) {
        const bool to_out = ((npass - 1 - p) & 1) == 0;  // the last pass lands in out
        uint64_t* ko = to_out ? out : tmp;
        void* vo = vin ? (to_out ? vout : vtmp) : nullptr;
        const int shift = bit0 + kRadixBits * p;
        const int mi = p == 0 ? mode : 0, mo = p == npass - 1 ? mode : 0;
        hipLaunchKernelGGL(radix64_upsweep_kernel<4>, dim3(nb), dim3(kUp64Threads), 0, s, ki, n, chunk, shift, nb,
                           counts, mi);
        hipLaunchKernelGGL(radix_scan_kernel, dim3(kBins), dim3(1024), 0, s, counts, nb, totals);
#define CME_DS64(VB, R)                                                                                            \
    hipLaunchKernelGGL((radix64_downsweep_kernel<VB, R>), dim3(nb), dim3(k64Threads), 0, s, ki, ko, vi, vo, n, chunk, \
                       shift, nb, counts, totals, mi, mo)
        if (val_bytes == 0) {
            if (lanes) CME_DS64(0, kRankLanes);
            else CME_DS64(0, kRankMatch);
        } else if (val_bytes == 4) {
            if (lanes) CME_DS64(4, kRankLanes);
            else CME_DS64(4, kRankMatch);
        } else {
            if (lanes) CME_DS64(8, kRankLanes);
            else CME_DS64(8, kRankMatch);
        }
#undef CME_DS64
        CME_TRY(hipGetLastError());
        ki = ko;
        vi = vo;
    }
    return 0;
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(radix64_upsweep, 256, radix64_upsweep_kernel<4>);
CME_REGISTER_KERNEL(radix64_downsweep, 1024, radix64_downsweep_kernel<0, kRankLanes>);
CME_REGISTER_KERNEL(radix64_downsweep_v4, 1024, radix64_downsweep_kernel<4, kRankLanes>);
CME_REGISTER_KERNEL(radix64_downsweep_v8, 1024, radix64_downsweep_kernel<8, kRankLanes>);
CME_REGISTER_KERNEL(radix64_downsweep_v8_match, 1024, radix64_downsweep_kernel<8, kRankMatch>);
