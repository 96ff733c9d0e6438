// Shared by the two translation units of the sampled closed-loop dispersion (scvx_mc.hip, scvx_mc_nav.hip): the layout of a partial row,
// the kernel-argument constants and the wavefront reductions.  Not part of the ABI.
#pragma once
#include "scvx_internal.hpp"
#include "scvx_rng.hpp"

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

// The four state path functions of one node of one flight into pathv (the flying kernels with PV set): MASS = x[0], GLIDE =
// tan(gammaGs) |r[2:3]| - r[1], TILT = |q[3:4]|, RATE = |w| -- the audit's own expressions, the constants of tilt (sqcm) and rate
// (omMax) NOT subtracted.  p points at (b, k, MASS, s); consecutive functions are S apart.  Plain vector stores.
__device__ __forceinline__ void mc_path_store(double* __restrict__ p, int S, double tggs, const double* xs) {
    p[(size_t)SCVX_PSIG_MASS * S] = xs[0];
    p[(size_t)SCVX_PSIG_GLIDE * S] = tggs * sqrt(xs[2] * xs[2] + xs[3] * xs[3]) - xs[1];
    p[(size_t)SCVX_PSIG_TILT * S] = sqrt(xs[9] * xs[9] + xs[10] * xs[10]);
    p[(size_t)SCVX_PSIG_RATE * S] = sqrt(xs[11] * xs[11] + xs[12] * xs[12] + xs[13] * xs[13]);
}

// the context's workspace of partial rows, grown on demand (scvx_mc.hip)
hipError_t mc_workspace(scvx_ctx* ctx, size_t doubles);
// ... and, beside it, the workspace of the dense values whose order statistics are asked for without the dense output itself
// (flights [B][S][16] and pathv [B][K+1][5][S]), under the same rule: no two calls on one context overlapping on different streams
hipError_t mc_q_workspace(scvx_ctx* ctx, size_t doubles);

// What the _q forms add to a sampled call (scvx_quantile.hip, scvx_mc.hip): nq ranks (host), flightq [B][16][nq], pathq
// [B][K+1][5][nq], pathv [B][K+1][5][S], each a device pointer or nullptr.
struct McQ {
    int nq = 0;
    const int* ranks = nullptr;
    double *flightq = nullptr, *pathq = nullptr, *pathv = nullptr;
};
// The _rng forms: the draws are made by the lanes (scvx_rng.hpp) and the pointers xi0 / eta / xin / nud of the launch are not read;
// noise: whether the truth receives the impulses sqrt(w) eta (the role of eta != nullptr in the calls on uploaded draws).
struct McRng {
    const scvx_mc_rng* r = nullptr;
    int noise = 0;
};
inline McRngK mc_rng_k(const McRng& g, bool noise) {
    return McRngK{g.r->seed, g.r->s_lo, g.r->b_lo, g.r->independent, noise ? 1 : 0};
}
// The _veh forms: per-flight vehicle errors theta = mu + sp * zeta (include/scvx.h).  zeta [S][6] and theta [B][S][6] are device
// pointers or nullptr (zeta is not read when the lanes make the draws); McVehK is what the ACT instantiations take as their last
// kernel argument.
struct McVeh {
    const scvx_mc_vehicle* v = nullptr;
    const double* zeta = nullptr;
    double* theta = nullptr;
};
struct McVehK {
    double mu[SCVX_VEH_N], sp[SCVX_VEH_N];
    const double* zeta;
    double* theta;
};
inline McVehK mc_veh_k(const McVeh& h) {
    McVehK k{};
    for (int i = 0; i < SCVX_VEH_N; i++) k.mu[i] = h.v->mu[i], k.sp[i] = h.v->sp[i];
    k.zeta = h.zeta, k.theta = h.theta;
    return k;
}
// veh may be nullptr (then zeta and theta must be); rng: whether the lanes make the draws
int check_mc_vehicle(scvx_ctx* ctx, const scvx_mc_vehicle* veh, const void* zeta, const void* theta, bool rng);
// what the _veh entry points ask of the draws before they become a _q or an _rng call: with rng every uploaded draw must be NULL,
// without it noise must be 0
int check_mc_veh_draws(scvx_ctx* ctx, const scvx_mc_rng* rng, int noise, const void* xi0, const void* eta, const void* xin,
                       const void* nud, const void* zeta);
int check_mc_rng(scvx_ctx* ctx, const scvx_mc_rng* rng);
int check_mc_q(scvx_ctx* ctx, int S, int nq, const int* ranks, const void* flightq, const void* pathq);
int check_ranks(scvx_ctx* ctx, int S, int nq, const int* ranks);
// rows: row r starts at v[(r / inner) * ld_outer + (r % inner) * ld_inner], its S values inc apart; out [R][nq]
hipError_t launch_order_stats(int R, int S, const double* v, size_t ld_outer, int inner, size_t ld_inner, size_t inc, int nq,
                              const int* ranks, double* out, hipStream_t st);
// where the flying kernel writes flights / pathv (the caller's buffer, the workspace, or nullptr), then after it: the order statistics
hipError_t mc_q_buffers(scvx_ctx* ctx, int B, int K, int S, const McQ& q, double*& flights, double*& pathv);
hipError_t mc_q_finish(int B, int K, int S, const McQ& q, const double* flights, const double* pathv, hipStream_t st);

}  // namespace scvx
