// Tuning arms of the wave-pipelined heat pass (kernel: heat_pipe.h):
// rows per phase, prefetch depth, steps per pass, waves per role, wide lanes.
#include "../hip/heat_pipe.h"

// Tuning entry for the wave-pipelined ns-step pass (fp32, order 8): ns 3..6,
// rows per phase rb, arm number pd, explicit chunk or tasks per CU.
namespace {
struct TuneCall {
    const float* p;
    float* c;
    int pitch, gy;
    Region g;
    float xcfl, ycfl;
    int chunk, per_cu;
    hipStream_t s;
};

// one arm: config C at (NS, RB) where the arm takes that combination
template <int NS, int RB, PipeCfg C, bool OK>
int arm(const TuneCall& a) {
    if constexpr (OK)
        return launch_pipe_multi<float, with(C, NS, RB)>(a.p, a.c, a.pitch, a.gy, &a.g, 1, a.g, a.xcfl, a.ycfl, a.chunk,
                                                         a.per_cu, a.s);
    else
        return (int)hipErrorInvalidValue;
}

// The arms, by number: what it is, then its config and the (NS, RB) it
// takes. Fields not named: order 8, kFma, prefetch depth 1, temporal stores,
// one wave per role, 4 columns per lane; ns and rb come from the call. 81..98
// are wide lanes (8 columns per lane) with non-temporal stores.
template <int NS, int RB>
int tunep_pd(const TuneCall& a, int pd) {
    // clang-format off
    switch (pd) {
        case 1: return arm<NS, RB, PipeCfg{}, true>(a);
        // prefetch depth 2
        case 2: return arm<NS, RB, PipeCfg{.pd = 2}, true>(a);
        // non-temporal output stores
        case 11: return arm<NS, RB, PipeCfg{.nt = true}, RB == 4>(a);
        // 11, reassociated ("fast") arithmetic
        case 12: return arm<NS, RB, PipeCfg{.arith = kFast, .nt = true}, RB == 4>(a);
        // 12, registers capped for 4 waves per SIMD
        case 13: return arm<NS, RB, PipeCfg{.arith = kFast, .nt = true, .occ = 4}, RB == 4>(a);
        // 11 + two waves per role (seams through LDS)
        case 21: return arm<NS, RB, PipeCfg{.nt = true, .wpr = 2}, RB == 4>(a);
        // 11 + four waves per role
        case 41: return arm<NS, RB, PipeCfg{.nt = true, .wpr = 4}, RB == 4 && NS <= 4>(a);
        // wide lanes
        case 81: return arm<NS, RB, PipeCfg{.nt = true, .vw = 8}, RB <= 4 && NS <= 5>(a);
        // 81, registers capped for 3 waves per SIMD
        case 83: return arm<NS, RB, PipeCfg{.nt = true, .vw = 8, .occ = 3}, RB == 2 && NS == 4>(a);
        // 81, capped for 4
        case 84: return arm<NS, RB, PipeCfg{.nt = true, .vw = 8, .occ = 4}, RB == 2 && NS == 4>(a);
        // FMA chains interleaved across the lane's points (bitwise = 81)
        case 85: return arm<NS, RB, PipeCfg{.arith = kFmaTermMajor, .nt = true, .vw = 8}, RB <= 4 && NS <= 5>(a);
        // 85, roles 1.. read x-neighbours from the LDS ring
        case 86: return arm<NS, RB, PipeCfg{.arith = kFmaTermMajor, .nt = true, .vw = 8, .lx = true}, RB <= 4 && NS <= 4>(a);
        // 85, prefetch depth 2 (RB 1: 151 VGPRs; RB 2: 175 = 2 waves/SIMD)
        case 87: return arm<NS, RB, PipeCfg{.arith = kFmaTermMajor, .pd = 2, .nt = true, .vw = 8}, RB <= 2 && NS == 4>(a);
        // 85, RB 1 capped at 4 waves per SIMD (128 VGPRs, 15 spilled)
        case 88: return arm<NS, RB, PipeCfg{.arith = kFmaTermMajor, .nt = true, .vw = 8, .occ = 4}, RB == 1 && NS == 4>(a);
        // 85, RB 1, prefetch depth 3
        case 89: return arm<NS, RB, PipeCfg{.arith = kFmaTermMajor, .pd = 3, .nt = true, .vw = 8}, RB == 1 && NS == 4>(a);
        // reassociated ("fast"): 17 instead of 20 flop-instructions per point
        case 91: return arm<NS, RB, PipeCfg{.arith = kFast, .nt = true, .vw = 8}, RB == 2 && NS <= 4>(a);
        // 91, capped for 3 waves per SIMD
        case 92: return arm<NS, RB, PipeCfg{.arith = kFast, .nt = true, .vw = 8, .occ = 3}, RB == 2 && NS <= 4>(a);
        // 91, terms interleaved across the lane's points (bitwise = 91)
        case 95: return arm<NS, RB, PipeCfg{.arith = kFastTermMajor, .nt = true, .vw = 8}, RB == 2 && NS <= 4>(a);
        // 95, capped for 3 waves per SIMD
        case 96: return arm<NS, RB, PipeCfg{.arith = kFastTermMajor, .nt = true, .vw = 8, .occ = 3}, RB == 2 && NS <= 4>(a);
        // 96 at ONE row per phase (168 VGPRs, no spill)
        case 97: return arm<NS, RB, PipeCfg{.arith = kFastTermMajor, .nt = true, .vw = 8, .occ = 3}, RB == 1 && NS == 4>(a);
        // 96 on explicit float pairs, role 0 loads into its window (bitwise = 91; production)
        case 98: return arm<NS, RB, PipeCfg{.arith = kFastPacked, .nt = true, .vw = 8, .occ = 3}, RB == 2 && NS <= 4>(a);
        default: return (int)hipErrorInvalidValue;
    }
    // clang-format on
}
template <int NS>
int tunep_rb(const TuneCall& a, int rb, int pd) {
    if (rb == 4) return tunep_pd<NS, 4>(a, pd);
    if constexpr (NS == 4) {
        if (rb == 1 && pd >= 85) return tunep_pd<NS, 1>(a, pd);
    }
    if constexpr (NS <= 4) {
        if (rb == 2) return tunep_pd<NS, 2>(a, pd);
        if (rb == 8) return tunep_pd<NS, 8>(a, pd);
    }
    return (int)hipErrorInvalidValue;
}
}  // namespace

CME_EXPORT int cme_heat_pipe_tune(const float* prev, float* curr, int pitch, int gy, int xb, int xe, int yb, int ye,
                                  float xcfl, float ycfl, int chunk, int rb, int ns, int pd, int per_cu,
                                  void* stream) {
    const TuneCall a{prev, curr, pitch, gy, Region{xb, xe, yb, ye}, xcfl, ycfl, chunk, per_cu, as_stream(stream)};
    switch (ns) {
        case 3: return tunep_rb<3>(a, rb, pd);
        case 4: return tunep_rb<4>(a, rb, pd);
        case 5: return tunep_rb<5>(a, rb, pd);
        case 6: return tunep_rb<6>(a, rb, pd);
        default: return (int)hipErrorInvalidValue;
    }
}

// Profiling entry (benchmarks/trace_pipe_tasks.py): the production fp32
// wide-lane pass (kFmaTermMajor, rb 2) over `nout` regions as the fused
// distributed schedule launches them (deep interior first, then the border
// strips), with every workgroup recording {start, end} wall-clock ticks and
// {region << 40 | XCC_ID << 32 | HW_ID} into trace (3 x u64 per workgroup;
// the caller sizes it for the grid and zeroes it). chunk / per_cu: the chunk
// rule's overrides (0 = production rule).
CME_EXPORT int cme_heat_pipe_trace(const float* prev, float* curr, int pitch, int gy, const int* out, int nout,
                                   const int* ext, int ns, float xcfl, float ycfl, int chunk, int per_cu,
                                   unsigned long long* trace, void* stream) {
    Region gs[kMaxS2Regions];
    if (!regions_from(out, nout, gs) || !trace) return (int)hipErrorInvalidValue;
    const Region e{ext[0], ext[1], ext[2], ext[3]};
    PipeGate gate;
    gate.trace = trace;
    hipStream_t s = as_stream(stream);
    constexpr PipeCfg kProd = pipe_prod_cfg<float>(8, true, true);
    switch (ns) {
        case 3: return launch_pipe_multi<float, with(kProd, 3)>(prev, curr, pitch, gy, gs, nout, e, xcfl, ycfl, chunk, per_cu, s, gate);
        case 4: return launch_pipe_multi<float, with(kProd, 4)>(prev, curr, pitch, gy, gs, nout, e, xcfl, ycfl, chunk, per_cu, s, gate);
        default: return (int)hipErrorInvalidValue;
    }
}
