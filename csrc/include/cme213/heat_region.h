// Compute-region descriptors shared by the multi-step heat kernels
// (heat2d.hip: stream2 / streamN; heat_pipe.hip: the wave-pipelined pass).
#pragma once

namespace cme {

constexpr int cgcd(int a, int b) { return b == 0 ? a : cgcd(b, a % b); }

// A rectangle of cells [xb, xe) x [yb, ye) of a device grid.
struct Region {
    int xb, xe, yb, ye;
};

// Up to eight output regions per launch (a distributed subdomain's border
// strips go out as ONE launch, or its deep interior AND border strips in the
// fused schedule); every region shares the intermediate-step region passed
// next to it.
constexpr int kMaxS2Regions = 8;
struct S2Regions {
    int n;
    int xb[kMaxS2Regions], xe[kMaxS2Regions], yb[kMaxS2Regions], ye[kMaxS2Regions];
    int strips[kMaxS2Regions], chunk[kMaxS2Regions];
    int wave_end[kMaxS2Regions];  // cumulative wave (or workgroup-task) counts
};

// The nout regions {xb, xe, yb, ye} a C entry point receives as ints, into
// gs[kMaxS2Regions]; false if there are none or too many.
inline bool regions_from(const int* out, int nout, Region* gs) {
    if (nout < 1 || nout > kMaxS2Regions) return false;
    for (int i = 0; i < nout; ++i) gs[i] = Region{out[4 * i], out[4 * i + 1], out[4 * i + 2], out[4 * i + 3]};
    return true;
}

// Output columns of one 64-lane strip of an NS-step pass (4 columns per lane;
// step k is valid on lanes k..63-k, x-neighbours arrive through DPP).
template <int NS>
struct StripN {
    static constexpr int kOut = (64 - 2 * NS) * 4;
};

// Fused-schedule gate of the pipelined pass: workgroups of regions
// [from, n) wait until *flag >= val (wrap-safe) before reading their input
// -- the halo exchange of the previous pass signals the flag from the comm
// stream (dist_heat.hip). Bounded: a wait past the spin limit sets *timeout
// (pinned host word) and proceeds. flag == nullptr: no gate. `spins`: polls
// before giving up (~2^24: tens of seconds; CME_DIST_GATE_SPINS lowers it so
// a test can force the timeout path).
struct PipeGate {
    const unsigned* flag = nullptr;
    unsigned val = 0;
    int from = 0;
    unsigned* timeout = nullptr;
    unsigned spins = 1u << 24;
    // profiling only (hip_tune/heat_pipe_tune.hip cme_heat_pipe_trace): per
    // task {start, end} wall clock (100 MHz) and {HW_ID, XCC_ID, region}
    unsigned long long* trace = nullptr;
};

}  // namespace cme
