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

// What the _q forms add to a sampled call (scvx_quantile.hip, scvx_mc.hip): nq ranks (host), flightq [B][16][nq], pathq
// [B][K+1][5][nq], pathv [B][K+1][5][S], each a device pointer or nullptr.
struct McQ {
    int nq = 0;
    const int* ranks = nullptr;
    double *flightq = nullptr, *pathq = nullptr, *pathv = nullptr;
};
inline McRngK mc_rng_k(const scvx_mc_rng& r, bool noise) { return McRngK{r.seed, r.s_lo, r.b_lo, r.independent, noise ? 1 : 0}; }
// The _veh forms: per-flight vehicle errors theta = mu + sp * zeta (include/scvx.h).  v == nullptr: the nominal vehicle, the
// instantiations without ACT.  zeta [S][6] and theta [B][S][6] or nullptr (zeta is not read when the lanes make the draws); McVehK is
// what the ACT instantiations take as their last kernel argument.
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

// One sampled call, whichever of the 24 entry points it came through: everything such a call can carry, under the names of
// include/scvx.h.  What a form does not take stays nullptr / 0.  The arrays are the caller's -- host arrays at the _host and the
// batch-level forms -- or, behind stage_mc, their device copies; w, H, rm, q.ranks, rng and veh.v are always host memory.
struct McCall {
    int B = 0, K = 0, S = 0;
    const double *x = nullptr, *u = nullptr, *sigma = nullptr, *gain = nullptr, *C0 = nullptr;   // the plan, its gains, the dispersion
    const double *xi0 = nullptr, *eta = nullptr;                                                  // uploaded draws
    const double* w = nullptr;   // sw14 (flown on the truth: the impulse's size) or w14 (nav: its VARIANCE)
    const void* reserved = nullptr;
    int nsub = 0, flags = 0;
    double tol = 0.0;
    double *mcrep = nullptr, *xmean = nullptr, *xcov = nullptr, *flights = nullptr, *xland = nullptr, *dx0 = nullptr;
    McQ q;
    // drawn: the lanes make the draws (the _rng forms, the _veh forms with rng) from rng, no draw is uploaded, and noise says whether
    // the truth receives the impulses -- the role of eta != nullptr in a call on uploaded draws
    bool drawn = false;
    const scvx_mc_rng* rng = nullptr;
    int noise = 0;
    McVeh veh;
    bool nav = false;   // flown on a navigation estimate (scvx_mc_nav.hip): everything below applies
    Tiles deriv;
    const double *kf = nullptr, *CN = nullptr, *xin = nullptr, *nud = nullptr;
    int m = 0;
    const double *H = nullptr, *rm = nullptr;
    double *jmean = nullptr, *jcov = nullptr, *mcnav = nullptr, *navfed = nullptr, *navK = nullptr;
};
// what a batch-level form checks besides: the tracking weights and, with nav, N0 (host arrays).  The plan, the gains, the tiles and
// kf are then the batch's own and the reduced outputs optional: check_mc_call does not ask for them.
struct McBatch {
    const double *q14, *rNU, *qf14, *N0;
};
class Staging;
struct Dims;

// every refusal of a sampled call, in one order for all the forms (tests/golden/mc_refusals.txt, mc_batch_refusals.txt)
int check_mc_call(scvx_ctx* ctx, const McCall& c, const McBatch* batch = nullptr);
// the device copy of a record of host arrays: the inputs uploaded, the outputs asked for downloaded by s.finish();
// reduced_always: mcrep, xmean, xcov (jmean, jcov, mcnav) are allocated also where the caller does not want them
McCall stage_mc(Staging& s, const Dims& d, const McCall& host, bool reduced_always);
// the whole call on device arrays: workspaces, noise, the flights, the reduction, the order statistics (scvx_mc.hip; the flight on an
// estimate and its reduction are launch_mc_nav's, in scvx_mc_nav.hip beside their kernels)
hipError_t launch_mc(scvx_ctx* ctx, const McCall& dev, hipStream_t st);
hipError_t launch_mc_nav(scvx_ctx* ctx, const McCall& dev, const McK& m, const McRngK& rg, hipStream_t st);
// the two context-level shapes of an entry point: check and launch on the caller's device arrays; check, stage, launch, finish
int mc_call_dev(scvx_ctx* ctx, const McCall& c);
int mc_call_host(scvx_ctx* ctx, const McCall& c, const char* entry);

// veh may be nullptr (then zeta and theta must be); rng: whether the lanes make the draws
int check_mc_vehicle(scvx_ctx* ctx, const scvx_mc_vehicle* veh, const void* zeta, const void* theta, bool rng);
int check_mc_rng(scvx_ctx* ctx, const scvx_mc_rng* rng);
int check_ranks(scvx_ctx* ctx, int S, int nq, const int* ranks);
// rows: row r starts at v[(r / inner) * ld_outer + (r % inner) * ld_inner], its S values inc apart; out [R][nq]
hipError_t launch_order_stats(int R, int S, const double* v, size_t ld_outer, int inner, size_t ld_inner, size_t inc, int nq,
                              const int* ranks, double* out, hipStream_t st);

}  // namespace scvx
