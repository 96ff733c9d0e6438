// Sampled closed-loop dispersion (scvx_track_mc_f64, include/scvx.h): S flights per plan under the tracking law of scvx_track.hip, with
// an optional impulse of process noise at every node, reduced on the device to one row of statistics per plan.  No counterpart in the
// reference.
//
// The flights are mc_fly_kernel's (scvx_mc_fly.hpp: the kernel, its reduction and its launch, shared with the flight on a navigation
// estimate in scvx_mc_nav.hip).  This translation unit instantiates it with NAV = false (mm = 0 and null pointers for the estimate, none
// of them read): 24 kernels over (model) x (PV) x (RNG), no LDS, no barrier.  mc_finish_kernel (one block per plan) combines the
// ceil(S / 64) partial rows [MC_NP] of its plan in block order.
//
// The entry points without _q launch the instantiations with PV off; the _q forms (scvx_track_mc_q_f64, include/scvx.h) follow the
// flight with order statistics of the flight columns and of the rows of pathv; flights and pathv live in a second workspace of the
// context when only their order statistics are asked for.  The entry points without _rng launch the instantiations with RNG off;
// mc_draws_kernel writes out the draws the RNG instantiations consume.
#include "scvx_stage.hpp"
#include "scvx_mc_fly.hpp"   // the flying kernel, mc_finish_front, the noise and the launch, shared with scvx_mc_nav.hip

namespace scvx {

// The draws the RNG instantiations consume, written out (scvx_mc_draws_f64): one lane per (plan, s), grid (ceil(S / 64), P); xi0 / xin
// [P][S][14], eta / nud [P][S][K][14] (all 14 columns of a group: nud[.., 0:m] is what a call with m rows reads), each or nullptr.
__global__ __launch_bounds__(64) void mc_draws_kernel(McRngK rg, int S, int K, double* __restrict__ xi0, double* __restrict__ eta,
                                                      double* __restrict__ xin, double* __restrict__ nud) {
    const int p = blockIdx.y;
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= S) return;
    const uint64_t rc2 = mc_rng_c2(rg, p), rc3 = mc_rng_c3(rg, s);
    const size_t fl = (size_t)p * S + s;
    for (int st = 0; st < 2; st++) {
        double* z0 = st == 0 ? xi0 : xin;
        double* zk = st == 0 ? eta : nud;
        const uint64_t c1 = st == 0 ? MC_STREAM_TRUTH : MC_STREAM_NAV;
        if (z0) {
            double z[16];
            mc_draw_group(rg.seed, c1, rc2, rc3, 0, 14, z);
#pragma unroll
            for (int i = 0; i < 14; i++) z0[fl * 14 + i] = z[i];
        }
        if (zk)
            for (int k = 0; k < K; k++) {
                double z[16];
                mc_draw_group(rg.seed, c1, rc2, rc3, 1 + k, 14, z);
#pragma unroll
                for (int i = 0; i < 14; i++) zk[(fl * K + k) * 14 + i] = z[i];
            }
    }
}

// one block per plan: the partial rows of the plan combined in block order, then the report, the mean and the covariance
__global__ __launch_bounds__(256) void mc_finish_kernel(int S, int K, int nblk, const double* __restrict__ part,
                                                        double* __restrict__ mcrep, double* __restrict__ xmean,
                                                        double* __restrict__ xcov) {
    __shared__ double sh[MC_NP];
    mc_finish_front<MC_NP>(S, K, nblk, part, sh, mcrep, xmean, xcov);
}

// the context's workspace of partial rows, grown on demand (hipFree waits for whatever still reads the old one)
hipError_t mc_workspace(scvx_ctx* ctx, size_t doubles) {
    if (ctx->mc_ws_doubles >= doubles) return hipSuccess;
    if (ctx->mc_ws) (void)hipFree(ctx->mc_ws);
    ctx->mc_ws = nullptr;
    ctx->mc_ws_doubles = 0;
    hipError_t e = hipMalloc((void**)&ctx->mc_ws, doubles * 8);
    if (e == hipSuccess) ctx->mc_ws_doubles = doubles;
    return e;
}

hipError_t mc_q_workspace(scvx_ctx* ctx, size_t doubles) {
    if (ctx->mcq_ws_doubles >= doubles) return hipSuccess;
    if (ctx->mcq_ws) (void)hipFree(ctx->mcq_ws);
    ctx->mcq_ws = nullptr;
    ctx->mcq_ws_doubles = 0;
    hipError_t e = hipMalloc((void**)&ctx->mcq_ws, doubles * 8);
    if (e == hipSuccess) ctx->mcq_ws_doubles = doubles;
    return e;
}

void mc_workspace_free(scvx_ctx* ctx) {
    if (ctx->mc_ws) (void)hipFree(ctx->mc_ws);
    ctx->mc_ws = nullptr;
    ctx->mc_ws_doubles = 0;
    if (ctx->mcq_ws) (void)hipFree(ctx->mcq_ws);
    ctx->mcq_ws = nullptr;
    ctx->mcq_ws_doubles = 0;
}

// flights: the caller's dense buffer or nullptr on entry; on return where the flying kernel writes the flights (the workspace when
// only their order statistics are asked for), and pathv likewise (nullptr: the instantiations without per-node samples)
hipError_t mc_q_buffers(scvx_ctx* ctx, int B, int K, int S, const McQ& q, double*& flights, double*& pathv) {
    pathv = q.pathv;
    const size_t nf = (q.flightq && !flights) ? (size_t)B * S * SCVX_FLIGHT_NREP : 0;
    const size_t np = (q.pathq && !q.pathv) ? (size_t)B * (K + 1) * SCVX_PSIG_N * S : 0;
    if (nf + np == 0) return hipSuccess;
    hipError_t e = mc_q_workspace(ctx, nf + np);
    if (e != hipSuccess) return e;
    if (nf) flights = ctx->mcq_ws;
    if (np) pathv = ctx->mcq_ws + nf;
    return hipSuccess;
}

// the order statistics of the sixteen flight columns (rows of S values 16 apart) and of every (b, k, f) row of pathv (contiguous)
hipError_t mc_q_finish(int B, int K, int S, const McQ& q, const double* flights, const double* pathv, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (q.flightq)
        e = launch_order_stats(B * SCVX_FLIGHT_NREP, S, flights, (size_t)S * SCVX_FLIGHT_NREP, SCVX_FLIGHT_NREP, 1, SCVX_FLIGHT_NREP, q.nq,
                               q.ranks, q.flightq, st);
    if (e == hipSuccess && q.pathq)
        e = launch_order_stats(B * (K + 1) * SCVX_PSIG_N, S, pathv, (size_t)S, 1, 0, 1, q.nq, q.ranks, q.pathq, st);
    return e;
}

int check_mc_rng(scvx_ctx* ctx, const scvx_mc_rng* rng) {
    if (!ctx) return SCVX_ERR_ARG;
    if (!rng) return fail(ctx, SCVX_ERR_ARG, "mc rng: null rng");
    if (rng->reserved != 0) return fail(ctx, SCVX_ERR_ARG, "mc rng: reserved must be 0");
    if (rng->independent != 0 && rng->independent != 1) return fail(ctx, SCVX_ERR_ARG, "mc rng: independent must be 0 or 1");
    return SCVX_OK;
}

int check_mc_q(scvx_ctx* ctx, int S, int nq, const int* ranks, const void* flightq, const void* pathq) {
    if (nq == 0 && !flightq && !pathq) return SCVX_OK;   // nothing asked for: the call it extends
    return check_ranks(ctx, S, nq, ranks);
}

hipError_t launch_track_mc(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw, int nsub, int flags, double tol,
                           double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0, hipStream_t st,
                           const McQ* q, const McRng* rng, const McVeh* veh) {
    const int nblk = (S + 63) / 64;
    hipError_t e = mc_workspace(ctx, (size_t)B * nblk * MC_NP);
    if (e != hipSuccess) return e;
    double* pv = nullptr;
    if (q && (e = mc_q_buffers(ctx, B, K, S, *q, flights, pv)) != hipSuccess) return e;
    McK m{};
    m.tol = tol;
    const McRngK rg = mc_noise(m, sw, false, eta, rng);
    double* part = ctx->mc_ws;
    e = launch_mc_fly<false>(ctx, m, B, K, S, x, u, sigma, gain, C0, xi0, eta, nsub, flags, part, flights, xland, dx0, pv, rng, rg, st,
                             McNavA<double>{}, veh);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, S, K, nblk, part, mcrep, xmean, xcov);
    e = hipGetLastError();
    if (e != hipSuccess || !q) return e;
    return mc_q_finish(B, K, S, *q, flights, pv, st);
}

int check_track_mc(scvx_ctx* ctx, int B, int K, int S, const void* x, const void* u, const void* sigma, const void* gain, const void* C0,
                   const void* xi0, const void* eta, const double* sw, const void* reserved, int nsub, int flags, double tol,
                   const void* mcrep, const void* xmean, const void* xcov) {
    if (!ctx) return SCVX_ERR_ARG;
    if (B < 1 || B > 65535) return fail(ctx, SCVX_ERR_ARG, "track mc: 1 <= B <= 65535 required");
    if (S < 1) return fail(ctx, SCVX_ERR_ARG, "track mc: S >= 1 required");
    if (K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "track mc: K must equal the problem's K");
    if (nsub < 1 || nsub > 1000) return fail(ctx, SCVX_ERR_ARG, "track mc: nsub must be in [1,1000]");
    if (flags & ~SCVX_TRACK_CLAMP) return fail(ctx, SCVX_ERR_ARG, "track mc: unknown flags (SCVX_TRACK_CLAMP)");
    if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(ctx, SCVX_ERR_ARG, "track mc: tol must be finite and >= 0");
    if (sw)
        for (int i = 0; i < 14; i++)
            if (!(sw[i] >= 0.0) || !std::isfinite(sw[i])) return fail(ctx, SCVX_ERR_ARG, "track mc: sw must be finite and >= 0");
    if (eta && !sw) return fail(ctx, SCVX_ERR_ARG, "track mc: eta without sw");
    if (reserved) return fail(ctx, SCVX_ERR_ARG, "track mc: the reserved argument must be NULL");
    if (!x || !u || !sigma || !gain || !C0 || !xi0 || !mcrep || !xmean || !xcov) return fail(ctx, SCVX_ERR_ARG, "track mc: null buffer");
    if (ctx->prob.aero_kind == 1 && !ctx->dyn.aero)
        return fail(ctx, SCVX_ERR_STATE, "AtmosphericData problem: call scvx_set_aero_table first");
    return SCVX_OK;
}

// scvx_track_mc_q_f64 and, with rg (then xi0_dev and eta_dev are placeholders that are never read), scvx_track_mc_rng_f64
static int track_mc_q_dev(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev, const McRng* rg, const McVeh* vh = nullptr) {
    int rc = scvx::check_track_mc(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags,
                                  tol, mcrep_dev, xmean_dev, xcov_dev);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq_dev, pathq_dev))) return rc;
    if (vh && (rc = scvx::check_mc_vehicle(ctx, vh->v, vh->zeta, vh->theta, rg != nullptr))) return rc;
    if (vh && !vh->v) vh = nullptr;   // veh == NULL: the call without vehicle errors
    scvx::McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = flightq_dev, q.pathq = pathq_dev, q.pathv = pathv_dev;
    const bool any = flightq_dev || pathq_dev || pathv_dev;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_mc(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, rg ? nullptr : xi0_dev,
                                        rg ? nullptr : eta_dev, sw14, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, flights_dev,
                                        xland_dev, dx0_dev, ctx->stream, any ? &q : nullptr, rg, vh));
    return SCVX_OK;
}

// scvx_track_mc_q_f64_host and, with rg (xi0 and eta placeholders, nothing of them uploaded), scvx_track_mc_rng_f64_host
static int track_mc_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0,
                           int nq, const int* ranks, double* flightq, double* pathq, double* pathv, const McRng* rg,
                           const McVeh* vh = nullptr, const char* entry = "scvx_track_mc_q_f64_host");

// one lane per (plan, s): the draws the _rng forms consume (mc_draws_kernel); any of the four outputs may be nullptr
hipError_t launch_mc_draws(const scvx_mc_rng& r, int P, int S, int K, double* xi0, double* eta, double* xin, double* nud, hipStream_t st) {
    const McRng g{&r, 0};
    hipLaunchKernelGGL(mc_draws_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)P), dim3(64), 0, st, mc_rng_k(g, false), S, K, xi0, eta,
                       xin, nud);
    return hipGetLastError();
}

int check_mc_draws(scvx_ctx* ctx, const scvx_mc_rng* rng, int P, int S, int K) {
    int rc = check_mc_rng(ctx, rng);
    if (rc) return rc;
    if (P < 1 || P > 65535) return fail(ctx, SCVX_ERR_ARG, "mc draws: 1 <= P <= 65535 required");
    if (S < 1) return fail(ctx, SCVX_ERR_ARG, "mc draws: S >= 1 required");
    if (K < 1) return fail(ctx, SCVX_ERR_ARG, "mc draws: K >= 1 required");
    return SCVX_OK;
}

}  // namespace scvx

extern "C" {

int scvx_mc_draws_f64(scvx_ctx* ctx, const scvx_mc_rng* rng, int P, int S, int K, double* xi0_dev, double* eta_dev, double* xin_dev,
                      double* nud_dev) {
    int rc = scvx::check_mc_draws(ctx, rng, P, S, K);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_mc_draws(*rng, P, S, K, xi0_dev, eta_dev, xin_dev, nud_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_mc_draws_f64_host(scvx_ctx* ctx, const scvx_mc_rng* rng, int P, int S, int K, double* xi0, double* eta, double* xin, double* nud) {
    int rc = scvx::check_mc_draws(ctx, rng, P, S, K);
    if (rc) return rc;
    const size_t n0 = (size_t)P * S * 14, nk = n0 * K;
    scvx::Staging s(ctx);
    double *d0 = s.out(xi0, n0), *d1 = s.out(eta, nk), *d2 = s.out(xin, n0), *d3 = s.out(nud, nk);
    s.launch([&] { return scvx::launch_mc_draws(*rng, P, S, K, d0, d1, d2, d3, s.st); });
    return s.finish("scvx_mc_draws_f64_host");
}

int scvx_track_mc_q_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                        const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                        const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                        double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                        double* pathq_dev, double* pathv_dev) {
    return scvx::track_mc_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags, tol,
                                mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, nq, ranks, flightq_dev, pathq_dev,
                                pathv_dev, nullptr);
}

// the placeholders: xi0 any non-null pointer, eta non-null exactly when the truth receives impulses (check_track_mc's rules for them)
int scvx_track_mc_rng_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const scvx_mc_rng* rng, int noise, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev) {
    const scvx::McRng rg{rng, noise};
    return scvx::track_mc_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, x_dev, noise ? x_dev : nullptr, sw14, reserved,
                                nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, nq, ranks, flightq_dev,
                                pathq_dev, pathv_dev, &rg);
}

int scvx_track_mc_rng_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const scvx_mc_rng* rng, int noise, const double* sw14,
                               const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                               double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                               double* pathv) {
    const scvx::McRng rg{rng, noise};
    return scvx::track_mc_q_host(ctx, B, K, S, x, u, sigma, gain, C0, x, noise ? x : nullptr, sw14, reserved, nsub, flags, tol, mcrep,
                                 xmean, xcov, flights, xland, dx0, nq, ranks, flightq, pathq, pathv, &rg);
}

// the _veh forms: the _q call (rng == NULL) or the _rng call (its placeholders as above) with the vehicle errors behind it
int scvx_track_mc_veh_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev, const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh,
                          const double* zeta_dev, double* theta_dev) {
    int rc = scvx::check_mc_veh_draws(ctx, rng, noise, xi0_dev, eta_dev, nullptr, nullptr, zeta_dev);
    if (rc) return rc;
    const scvx::McRng rg{rng, noise};
    const scvx::McVeh vh{veh, zeta_dev, theta_dev};
    if (rng) xi0_dev = x_dev, eta_dev = noise ? x_dev : nullptr;
    return scvx::track_mc_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags, tol,
                                mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, nq, ranks, flightq_dev, pathq_dev,
                                pathv_dev, rng ? &rg : nullptr, &vh);
}

int scvx_track_mc_veh_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* sw14,
                               const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                               double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                               double* pathv, const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh, const double* zeta,
                               double* theta) {
    int rc = scvx::check_mc_veh_draws(ctx, rng, noise, xi0, eta, nullptr, nullptr, zeta);
    if (rc) return rc;
    const scvx::McRng rg{rng, noise};
    const scvx::McVeh vh{veh, zeta, theta};
    if (rng) xi0 = x, eta = noise ? x : nullptr;
    return scvx::track_mc_q_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov,
                                 flights, xland, dx0, nq, ranks, flightq, pathq, pathv, rng ? &rg : nullptr, &vh,
                                 "scvx_track_mc_veh_f64_host");
}

int scvx_track_mc_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                      const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                      const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                      double* flights_dev, double* xland_dev, double* dx0_dev) {
    return scvx_track_mc_q_f64(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags, tol,
                               mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, 0, nullptr, nullptr, nullptr, nullptr);
}

int scvx_track_mc_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland,
                           double* dx0) {
    return scvx_track_mc_q_f64_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov,
                                    flights, xland, dx0, 0, nullptr, nullptr, nullptr, nullptr);
}

int scvx_track_mc_q_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                             const double* gain, const double* C0, const double* xi0, const double* eta, const double* sw14,
                             const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                             double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                             double* pathv) {
    return scvx::track_mc_q_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov,
                                 flights, xland, dx0, nq, ranks, flightq, pathq, pathv, nullptr);
}

}  // extern "C"

namespace scvx {

static int track_mc_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0,
                           int nq, const int* ranks, double* flightq, double* pathq, double* pathv, const McRng* rg, const McVeh* vh,
                           const char* entry) {
    int rc = scvx::check_track_mc(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if (rg) xi0 = eta = nullptr;   // placeholders until here: the lanes make the draws
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq, pathq))) return rc;
    if (vh && (rc = scvx::check_mc_vehicle(ctx, vh->v, vh->zeta, vh->theta, rg != nullptr))) return rc;
    if (vh && !vh->v) vh = nullptr;   // veh == NULL: the call without vehicle errors
    const Dims d(B, K, scvx_control_dim(ctx), S, 0, nq);
    Staging s(ctx);
    McVeh dvh;   // the vehicle errors with zeta and theta on the device
    if (vh) dvh.v = vh->v, dvh.zeta = s.in(rg ? nullptr : vh->zeta, d.zeta), dvh.theta = s.out(vh->theta, d.theta);
    McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = s.out(flightq, d.flightq), q.pathq = s.out(pathq, d.pathq), q.pathv = s.out(pathv, d.pathv);
    const double *dx = s.in(x, d.x), *du = s.in(u, d.u), *ds = s.in(sigma, d.b), *dg = s.in(gain, d.gain), *dc = s.in(C0, d.c14),
                 *di = s.in(xi0, d.xi), *de = s.in(eta, d.eta);
    double *dr = s.out(mcrep, d.mcrep), *dm = s.out(xmean, d.b14), *dv = s.out(xcov, d.c14), *df = s.out(flights, d.flights),
           *dl = s.out(xland, d.s14), *d0 = s.out(dx0, d.s14);
    s.launch([&] {
        return launch_track_mc(ctx, B, K, S, dx, du, ds, dg, dc, di, de, sw14, nsub, flags, tol, dr, dm, dv, df, dl, d0, s.st,
                               (flightq || pathq || pathv) ? &q : nullptr, rg, vh ? &dvh : nullptr);
    });
    return s.finish(entry);
}

}  // namespace scvx
