// The compile-time configuration of the wave-pipelined heat pass
// (csrc/hip/heat_pipe.h): one value names a kernel, so a launch, a registry
// entry and a tuning arm that mean the same kernel say so with the same
// constant.
#pragma once

#include "cme213/heat_stencil.h"

namespace cme {

// Arithmetic of the row update. The numbers are the `fma` / arith codes of
// the C entry points (3 was "kFast capped at 4 waves per SIMD": now occ = 4).
enum PipeArith {
    kExact = 0,          // the reference's expression, contraction off
    kFma = 1,            // FMA-contracted (the reference's nvcc -fmad code)
    kFast = 2,           // reassociated, CFL numbers folded into the weights (heat_update_fast)
    kFmaTermMajor = 4,   // kFma with the chains of a lane's points interleaved term by term (bitwise kFma)
    kFastTermMajor = 5,  // kFast with its terms interleaved across the lane's points (bitwise kFast)
    kFastPacked = 6,     // kFastTermMajor's operations on explicit float pairs (wide lanes; bitwise kFast)
};

struct PipeCfg {
    int order = 8;    // stencil order: 2, 4, 8
    int ns = 4;       // timesteps per pass = roles per workgroup (2..6)
    int arith = kFma;
    int rb = 4;       // rows per phase
    int pd = 1;       // phases of input loads role 0 keeps in flight
    bool nt = false;  // non-temporal output stores
    int wpr = 1;      // waves per role, side by side
    int vw = 4;       // columns per lane (8: wide lanes, fp32)
    int occ = 0;      // waves per SIMD the registers are capped for; 0 = uncapped
    bool lx = false;  // roles 1.. read their x-neighbours from the LDS ring, not through DPP
    int ost = 0;      // output stores of the dataflow launch (heat_flow.hip): 1 / 2 = all / band-edge rows write-through
};

// `c` at ns steps per pass (and rb rows per phase), for dispatchers whose
// enclosing template or switch supplies them
constexpr PipeCfg with(PipeCfg c, int ns, int rb = 0) {
    c.ns = ns;
    if (rb > 0) c.rb = rb;
    return c;
}

// `c` without its register cap. occ only sets a kernel's launch bounds, so the
// kernel hands the body (pipe_task, PipeN) this value: kernels that differ in
// occ alone share one instantiation of the body.
constexpr PipeCfg uncapped(PipeCfg c) {
    c.occ = 0;
    return c;
}

// Output columns of one strip of the wave-pipelined pass: wpr waves side by
// side per timestep role (64*wpr lanes of vw columns). vw = 4: ns lanes lost
// per side (one lane per step, exact at order 8). vw = 8 (wide lanes): the
// whole lanes covering the ns*B columns each side loses over ns steps.
template <PipeCfg C>
struct PipeOut {
    static constexpr int B = HeatOrder<C.order>::B;
    static constexpr int kMargin = C.vw == 4 ? C.ns : (C.ns * B + C.vw - 1) / C.vw;
    static constexpr int kOut = (64 * C.wpr - 2 * kMargin) * C.vw;
};

}  // namespace cme
