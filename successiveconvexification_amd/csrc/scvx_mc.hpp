// Shared by the two translation units of the sampled closed-loop dispersion (scvx_mc.hip, scvx_mc_nav.hip): the layout of a partial row,
// the kernel-argument constants and the wavefront reductions.  Not part of the ABI.
#pragma once
#include "scvx_internal.hpp"

namespace scvx {

// one partial row: 16 maxima, 16 sums, the counts of P_MASS .. P_FIN, P_ANY, OUT_LO, OUT_HI, N_BAD (as doubles: exact below 2^53),
// the sum of the landing deviation e [14] and of the upper triangle of e e' [105]
constexpr int MC_MAX = 0, MC_SUM = 16, MC_CNT = 32, MC_ANY = 41, MC_LO = 42, MC_HI = 43, MC_BAD = 44, MC_E = 45, MC_EE = 59, MC_NP = 164;
// ... and behind it, in the row of scvx_track_mc_nav_f64: the sum of the navigation error eps_K [14], of the upper triangle of
// [e; eps_K][e; eps_K]' [406] (its 14 x 14 corner is MC_EE again, the same sums), and the largest |eps+_k|_inf fed to the law
constexpr int MCN_EPS = MC_NP, MCN_JJ = MCN_EPS + 14, MCN_FED = MCN_JJ + 406, MCN_NP = MCN_FED + 1;

struct McK {
    double sw[14];   // sqrt(w): the size of the impulse per state component
    double tol;
};

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ double wave_nan_max(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = nan_max(v, __shfl_xor(v, o));
    return v;
}

// the context's workspace of partial rows, grown on demand (scvx_mc.hip)
hipError_t mc_workspace(scvx_ctx* ctx, size_t doubles);

}  // namespace scvx
