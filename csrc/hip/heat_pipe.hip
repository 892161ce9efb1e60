// C entry points of the wave-pipelined heat pass (kernel: heat_pipe.h).
#include "heat_pipe.h"

// Production entry: ns (3..6) timesteps in one pass, like cme_heat_stepn_f32
// (intermediate steps over `ext`, the last writes `out`, nout <= 4 regions).
// The kernel of each (type, order, arithmetic, width) is pipe_prod_cfg's
// (heat_pipe.h).
namespace {
// CME_PIPE_VW: unset = the measured default (8 columns per lane at order 8,
// 4 at orders 2 / 4), 4 / 8 = that width at every order (fp32)
int pipe_vw_env() {
    const long x = cme::tune_get(cme::kTunePipeVW);
    return (x == 4 || x == 8) ? (int)x : 0;
}

template <typename T, PipeCfg C>
int pipe_steps(const T* p, T* c, int pitch, int gy, const Region* gs, int n, Region e, int ns, T xcfl, T ycfl,
               int chunk, hipStream_t s, PipeGate gate) {
    switch (ns) {
        case 3: return launch_pipe_multi<T, with(C, 3)>(p, c, pitch, gy, gs, n, e, xcfl, ycfl, chunk, 0, s, gate);
        case 4: return launch_pipe_multi<T, with(C, 4)>(p, c, pitch, gy, gs, n, e, xcfl, ycfl, chunk, 0, s, gate);
    }
    // 5 / 6 steps per pass, fp32: orders 2 / 4 are HBM-bound at 4 (profiles/heat_pipe_wide_r3.md)
    if constexpr (sizeof(T) == 4) {
        switch (ns) {
            case 5: return launch_pipe_multi<T, with(C, 5)>(p, c, pitch, gy, gs, n, e, xcfl, ycfl, chunk, 0, s, gate);
            case 6: return launch_pipe_multi<T, with(C, 6)>(p, c, pitch, gy, gs, n, e, xcfl, ycfl, chunk, 0, s, gate);
        }
    }
    return (int)hipErrorInvalidValue;
}

template <typename T, int ORDER, bool FMA>
int pipe_ns(const T* p, T* c, int pitch, int gy, const Region* gs, int n, Region e, int ns, T xcfl, T ycfl, int chunk,
            hipStream_t s, PipeGate gate) {
    if constexpr (sizeof(T) == 4) {
        const int env = pipe_vw_env();
        if (env == 8 || (env == 0 && ORDER == 8))
            return pipe_steps<T, pipe_prod_cfg<T>(ORDER, FMA, true)>(p, c, pitch, gy, gs, n, e, ns, xcfl, ycfl, chunk, s,
                                                                gate);
    }
    return pipe_steps<T, pipe_prod_cfg<T>(ORDER, FMA)>(p, c, pitch, gy, gs, n, e, ns, xcfl, ycfl, chunk, s, gate);
}

template <typename T, bool FMA>
int pipe_order(int order, const T* p, T* c, int pitch, int gy, const Region* gs, int n, Region e, int ns, T xcfl,
               T ycfl, int chunk, hipStream_t s, PipeGate gate) {
    switch (order) {
        case 2: return pipe_ns<T, 2, FMA>(p, c, pitch, gy, gs, n, e, ns, xcfl, ycfl, chunk, s, gate);
        case 4: return pipe_ns<T, 4, FMA>(p, c, pitch, gy, gs, n, e, ns, xcfl, ycfl, chunk, s, gate);
        case 8: return pipe_ns<T, 8, FMA>(p, c, pitch, gy, gs, n, e, ns, xcfl, ycfl, chunk, s, gate);
        default: return (int)hipErrorInvalidValue;
    }
}

// every cme_heat_pipe[_gated]_f32/f64: regions from ints, the arithmetic, the gate
template <typename T>
int pipe_entry(const T* prev, T* curr, int pitch, int gy, const int* out, int nout, const int* ext, int order,
               int nsteps, T xcfl, T ycfl, int chunk, int fma, int wait_from, const unsigned* flag, unsigned value,
               unsigned* timeout, void* stream) {
    Region gs[kMaxS2Regions];
    if (!regions_from(out, nout, gs) || (flag && !timeout)) return (int)hipErrorInvalidValue;
    const Region e{ext[0], ext[1], ext[2], ext[3]};
    const PipeGate gate = make_gate(flag, value, wait_from, timeout);
    return fma ? pipe_order<T, true>(order, prev, curr, pitch, gy, gs, nout, e, nsteps, xcfl, ycfl, chunk,
                                     as_stream(stream), gate)
               : pipe_order<T, false>(order, prev, curr, pitch, gy, gs, nout, e, nsteps, xcfl, ycfl, chunk,
                                      as_stream(stream), gate);
}
}  // namespace

CME_EXPORT int cme_heat_pipe_f32(const float* prev, float* curr, int pitch, int gy, const int* out, int nout,
                                 const int* ext, int order, int nsteps, float xcfl, float ycfl, int chunk, int fma,
                                 void* stream) {
    return pipe_entry<float>(prev, curr, pitch, gy, out, nout, ext, order, nsteps, xcfl, ycfl, chunk, fma, 0, nullptr,
                             0u, nullptr, stream);
}

CME_EXPORT int cme_heat_pipe_f64(const double* prev, double* curr, int pitch, int gy, const int* out, int nout,
                                 const int* ext, int order, int nsteps, double xcfl, double ycfl, int chunk, int fma,
                                 void* stream) {
    return pipe_entry<double>(prev, curr, pitch, gy, out, nout, ext, order, nsteps, xcfl, ycfl, chunk, fma, 0,
                              nullptr, 0u, nullptr, stream);
}

// The same pass with regions [wait_from, nout) gated on *flag >= value (the
// fused distributed schedule: deep interior and border strips in ONE launch,
// the border workgroups waiting for the previous halo exchange).
CME_EXPORT int cme_heat_pipe_gated_f32(const float* prev, float* curr, int pitch, int gy, const int* out, int nout,
                                       const int* ext, int order, int nsteps, float xcfl, float ycfl, int fma,
                                       int wait_from, const unsigned* flag, unsigned value, unsigned* timeout,
                                       void* stream) {
    return pipe_entry<float>(prev, curr, pitch, gy, out, nout, ext, order, nsteps, xcfl, ycfl, 0, fma, wait_from, flag,
                             value, timeout, stream);
}

// fp64 twin of cme_heat_pipe_gated_f32 (the fused schedule on the hw5
// workload's doubles, hw/hw5/2dHeat_solution.cpp:63-84).
CME_EXPORT int cme_heat_pipe_gated_f64(const double* prev, double* curr, int pitch, int gy, const int* out, int nout,
                                       const int* ext, int order, int nsteps, double xcfl, double ycfl, int fma,
                                       int wait_from, const unsigned* flag, unsigned value, unsigned* timeout,
                                       void* stream) {
    return pipe_entry<double>(prev, curr, pitch, gy, out, nout, ext, order, nsteps, xcfl, ycfl, 0, fma, wait_from,
                              flag, value, timeout, stream);
}

// kernels in the occupancy / resource report (cme_kernel_query)
CME_REGISTER_KERNEL(heat_pipe3_fma_f32_o8, 192, heat_pipe_kernel<float, with(pipe_prod_cfg<float>(8, true), 3)>);
CME_REGISTER_KERNEL(heat_pipe4_fma_f32_o8, 256, heat_pipe_kernel<float, with(pipe_prod_cfg<float>(8, true), 4)>);
CME_REGISTER_KERNEL(heat_pipe3w_fma_f32_o8, 192, heat_pipe_kernel<float, with(pipe_prod_cfg<float>(8, true, true), 3)>);
CME_REGISTER_KERNEL(heat_pipe4w_fma_f32_o8, 256, heat_pipe_kernel<float, with(pipe_prod_cfg<float>(8, true, true), 4)>);
CME_REGISTER_KERNEL(heat_pipe4w_f32_o8, 256, heat_pipe_kernel<float, with(pipe_prod_cfg<float>(8, false, true), 4)>);
