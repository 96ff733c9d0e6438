// Sampled closed-loop dispersion flown on a navigation ESTIMATE (scvx_track_mc_nav_f64, include/scvx.h): scvx_track_mc_f64's S flights
// per plan with the law fed x_fly - eps+_k, the error eps of the estimate generated per flight on the device from the filter gains of
// the navigation analysis (scvx_nav.hip), with measurement noise and with the process noise that hits the truth.  No counterpart in the
// reference.
//
// The flights are mc_fly_kernel's (scvx_mc_fly.hpp: the one body scvx_mc.hip instantiates too), here with NAV = true:
// 48 kernels over (model) x (PV) x (RNG) x (DS, the tiles' storage type).  What the estimate adds -- the error's recursion, its 12 KB of
// LDS (19 KB with RNG), the two barriers per node -- is described there.  With eps = 0 a flight is bitwise the flight with
// NAV = false, and with the eps+ the kernel wrote fed to scvx_track_fly_nav_f64 as `nav` a flight's 16 columns are bitwise that flyer's
// (tests/test_gpu_mc_nav.py).  The instantiations stay in a translation unit of their own: the two are the slowest to compile and are
// compiled side by side.
//
// H and sqrt(rm) are copied by a small launch (mc_nav_model_kernel) into the context's workspace behind the partial rows: from the
// kernel argument they would be kept in scalar registers for the whole flight, several hundred of them spilled.
//
// mc_nav_finish_kernel (one block per plan) combines the partial rows [MCN_NP] in block order.  The row is the plain one, then the sums
// of eps_K [14] and of the upper triangle of [e; eps_K][e; eps_K]' [406], and the largest |eps+_k|_inf fed; mcrep, xmean and xcov come
// from mc_finish_front, the expressions mc_finish_kernel uses.
#include "scvx_stage.hpp"
#include "scvx_mc_fly.hpp"

namespace scvx {

struct McNavK {
    double H[196];    // [m][14]
    double srm[14];   // sqrt(rm)
};

// the measurement model from the kernel argument of this small launch into the workspace, in stream order behind whatever still reads it
__global__ __launch_bounds__(256) void mc_nav_model_kernel(McNavK nv, double* __restrict__ dst) {
    const int t = threadIdx.x;
    if (t < MCN_SRM) dst[t] = nv.H[t];
    else if (t < MCN_MODEL) dst[t] = nv.srm[t - MCN_SRM];
}

// square root of a variance (a rounded variance of -1e-40 is 0, a NaN stays a NaN)
__device__ __forceinline__ double mcn_sd(double v) { return v > 0.0 ? sqrt(v) : (v != v ? v : 0.0); }

// one block per plan: the partial rows of the plan combined in block order and mc_finish_kernel's three outputs (mc_finish_front), then
// the joint mean and covariance of [e; eps_K], and the navigation report read off them
__global__ __launch_bounds__(256) void mc_nav_finish_kernel(int S, int K, int nblk, const double* __restrict__ part,
                                                            double* __restrict__ mcrep, double* __restrict__ xmean,
                                                            double* __restrict__ xcov, double* __restrict__ jmean,
                                                            double* __restrict__ jcov, double* __restrict__ mcnav) {
    __shared__ double sh[MCN_NP], jc[784];
    mc_finish_front<MCN_NP>(S, K, nblk, part, sh, mcrep, xmean, xcov);
    const int b = blockIdx.x, t = threadIdx.x;
    const double dS = double(S);
    // the sum of component i of [e; eps_K]: MC_E and MCN_EPS are not adjacent in the row
    auto vsum = [&](int i) { return i < 14 ? sh[MC_E + i] : sh[MCN_EPS + i - 14]; };
    if (t < 28) jmean[(size_t)b * 28 + t] = vsum(t) / dS;
    for (int e = t; e < 784; e += 256) {
        const int i = e / 28, j = e % 28;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const int idx = lo * 28 - (lo * (lo - 1)) / 2 + (hi - lo);
        double v = 0.0;
        if (S > 1) {
            const double mm = vsum(lo) * vsum(hi) / dS;
            v = (sh[MCN_JJ + idx] - mm) / (dS - 1.0);
        }
        jc[e] = v;
        jcov[(size_t)b * 784 + e] = v;
    }
    __syncthreads();
    if (t < SCVX_NAV_NREP) {
        // block traces of the eps block P (NAV_M .. NAV_W) and of Sigma_xx - C - C' + P (EST_R, EST_V), as nav_cov_kernel reads them
        const int i0 = t == SCVX_NAV_M ? 0 : (t == SCVX_NAV_R || t == SCVX_NAV_EST_R) ? 1 : (t == SCVX_NAV_V || t == SCVX_NAV_EST_V) ? 4
                       : t == SCVX_NAV_Q ? 7 : 11;
        const int i1 = t == SCVX_NAV_M ? 1 : (t == SCVX_NAV_R || t == SCVX_NAV_EST_R) ? 4 : (t == SCVX_NAV_V || t == SCVX_NAV_EST_V) ? 7
                       : t == SCVX_NAV_Q ? 11 : 14;
        double v;
        if (t == SCVX_NAV_PEAK) {
            v = sh[MCN_FED];   // MAX_FED: the sampled row has no per-node sums
        } else {
            double tr = 0.0;
            for (int i = i0; i < i1; i++) {
                if (t >= SCVX_NAV_EST_R) tr += jc[i * 28 + i] - jc[i * 28 + 14 + i] - jc[(14 + i) * 28 + i] + jc[(14 + i) * 28 + 14 + i];
                else tr += jc[(14 + i) * 28 + 14 + i];
            }
            v = mcn_sd(tr);
        }
        mcnav[(size_t)b * SCVX_NAV_NREP + t] = v;
    }
}

template <typename DS>
static hipError_t launch_track_mc_nav_t(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                        const double* gain, const double* C0, const double* xi0, const double* eta, const double* w,
                                        const DS* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int mm,
                                        const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                                        double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland,
                                        double* dx0, double* navfed, double* navK, hipStream_t st, const McQ* q, const McRng* rng,
                                        const McVeh* veh) {
    const int nblk = (S + 63) / 64;
    const size_t nrows = (size_t)B * nblk * MCN_NP;
    hipError_t e = mc_workspace(ctx, nrows + MCN_MODEL);
    if (e != hipSuccess) return e;
    double* pv = nullptr;
    if (q && (e = mc_q_buffers(ctx, B, K, S, *q, flights, pv)) != hipSuccess) return e;
    McK m{};
    m.tol = tol;
    const McRngK rg = mc_noise(m, w, true, eta, rng);
    McNavK nv{};
    for (int i = 0; i < mm; i++) nv.srm[i] = std::sqrt(rm[i]);
    for (int i = 0; i < mm * 14; i++) nv.H[i] = H[i];
    double* part = ctx->mc_ws;
    double* hm = ctx->mc_ws + nrows;
    hipLaunchKernelGGL(mc_nav_model_kernel, dim3(1), dim3(256), 0, st, nv, hm);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const McNavA<DS> na{mm, hm, deriv, kf, CN, xin, nud, navfed, navK};
    e = launch_mc_fly<true>(ctx, m, B, K, S, x, u, sigma, gain, C0, xi0, eta, nsub, flags, part, flights, xland, dx0, pv, rng, rg, st, na,
                            veh);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mc_nav_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, S, K, nblk, part, mcrep, xmean, xcov, jmean, jcov, mcnav);
    e = hipGetLastError();
    if (e != hipSuccess || !q) return e;
    return mc_q_finish(B, K, S, *q, flights, pv, st);
}

hipError_t launch_track_mc_nav(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w, Tiles deriv,
                               const double* kf, const double* CN, const double* xin, const double* nud, int m, const double* H,
                               const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                               double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0, double* navfed,
                               double* navK, hipStream_t st, const McQ* q, const McRng* rng, const McVeh* veh) {
    return deriv.d ? launch_track_mc_nav_t<double>(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w, deriv.d, kf, CN, xin, nud, m, H, rm, nsub,
                                                   flags, tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, st,
                                                   q, rng, veh)
                   : launch_track_mc_nav_t<float>(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w, deriv.f, kf, CN, xin, nud, m, H, rm, nsub,
                                                  flags, tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, st, q,
                                                  rng, veh);
}

int check_track_mc_nav(scvx_ctx* ctx, int B, int K, int S, const void* x, const void* u, const void* sigma, const void* gain,
                       const void* C0, const void* xi0, const void* eta, const double* w, const void* deriv, const void* kf,
                       const void* CN, const void* xin, const void* nud, int m, const double* H, const double* rm, int nsub, int flags,
                       double tol, const void* mcrep, const void* xmean, const void* xcov, const void* jmean, const void* jcov,
                       const void* mcnav) {
    if (!ctx) return SCVX_ERR_ARG;
    // everything scvx_track_mc_f64 refuses (its sw is checked below, as the variance w), in its words
    int rc = check_track_mc(ctx, B, K, S, x, u, sigma, gain, C0, xi0, nullptr, nullptr, nullptr, nsub, flags, tol, mcrep, xmean, xcov);
    if (rc) return rc;
    if (w)
        for (int i = 0; i < 14; i++)
            if (!(w[i] >= 0.0) || !std::isfinite(w[i])) return fail(ctx, SCVX_ERR_ARG, "track mc nav: w must be finite and >= 0");
    if (eta && !w) return fail(ctx, SCVX_ERR_ARG, "track mc nav: eta without w14");
    if ((rc = check_nav_model(ctx, m, H, rm))) return rc;
    if (!deriv || !CN || !xin || !jmean || !jcov || !mcnav)
        return fail(ctx, SCVX_ERR_ARG, "track mc nav: null buffer (deriv, CN, xin, jmean, jcov, mcnav)");
    if (m > 0 && (!kf || !nud)) return fail(ctx, SCVX_ERR_ARG, "track mc nav: m > 0 needs kf[B][K][14][m] and nud[S][K][m]");
    return SCVX_OK;
}

// scvx_track_mc_nav_q_f64 and, with rg (then xi0, eta, xin and nud are placeholders that are never read), scvx_track_mc_nav_rng_f64
static int track_mc_nav_q_dev(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                              const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* w14,
                              const double* deriv_dev, const double* kf_dev, const double* CN_dev, const double* xin_dev,
                              const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags, double tol,
                              double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev,
                              double* mcnav_dev, double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev,
                              double* navK_dev, int nq, const int* ranks, double* flightq_dev, double* pathq_dev, double* pathv_dev,
                              const McRng* rg, const McVeh* vh = nullptr) {
    int rc = scvx::check_track_mc_nav(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev, kf_dev,
                                      CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev,
                                      jcov_dev, mcnav_dev);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq_dev, pathq_dev))) return rc;
    if (vh && (rc = scvx::check_mc_vehicle(ctx, vh->v, vh->zeta, vh->theta, rg != nullptr))) return rc;
    if (vh && !vh->v) vh = nullptr;   // veh == NULL: the call without vehicle errors
    if (rg) xi0_dev = eta_dev = xin_dev = nud_dev = nullptr;   // placeholders until here: the lanes make the draws
    scvx::McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = flightq_dev, q.pathq = pathq_dev, q.pathv = pathv_dev;
    const bool any = flightq_dev || pathq_dev || pathv_dev;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_mc_nav(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14,
                                            scvx::Tiles{deriv_dev, nullptr}, kf_dev, CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol,
                                            mcrep_dev, xmean_dev, xcov_dev, jmean_dev, jcov_dev, mcnav_dev, flights_dev, xland_dev, dx0_dev,
                                            navfed_dev, navK_dev, ctx->stream, any ? &q : nullptr, rg, vh));
    return SCVX_OK;
}

static int track_mc_nav_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                               const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                               const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                               double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                               double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv,
                               const McRng* rg, const McVeh* vh = nullptr, const char* entry = "scvx_track_mc_nav_q_f64_host");

}  // namespace scvx

extern "C" {

int scvx_track_mc_nav_q_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                            const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* w14,
                            const double* deriv_dev, const double* kf_dev, const double* CN_dev, const double* xin_dev,
                            const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags, double tol,
                            double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev,
                            double* mcnav_dev, double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev,
                            double* navK_dev, int nq, const int* ranks, double* flightq_dev, double* pathq_dev, double* pathv_dev) {
    return scvx::track_mc_nav_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev, kf_dev,
                                    CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev,
                                    jcov_dev, mcnav_dev, flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, nq, ranks, flightq_dev,
                                    pathq_dev, pathv_dev, nullptr);
}

// the placeholders: xi0, xin and (with m > 0) nud any non-null pointer, eta non-null exactly when the truth receives impulses
// (check_track_mc_nav's rules for them)
int scvx_track_mc_nav_rng_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                              const double* gain_dev, const double* C0_dev, const scvx_mc_rng* rng, int noise, const double* w14,
                              const double* deriv_dev, const double* kf_dev, const double* CN_dev, int m, const double* H,
                              const double* rm, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev,
                              double* xcov_dev, double* jmean_dev, double* jcov_dev, double* mcnav_dev, double* flights_dev,
                              double* xland_dev, double* dx0_dev, double* navfed_dev, double* navK_dev, int nq, const int* ranks,
                              double* flightq_dev, double* pathq_dev, double* pathv_dev) {
    const scvx::McRng rg{rng, noise};
    return scvx::track_mc_nav_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, x_dev, noise ? x_dev : nullptr, w14, deriv_dev,
                                    kf_dev, CN_dev, x_dev, x_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev,
                                    jcov_dev, mcnav_dev, flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, nq, ranks, flightq_dev,
                                    pathq_dev, pathv_dev, &rg);
}

int scvx_track_mc_nav_rng_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                   const double* gain, const double* C0, const scvx_mc_rng* rng, int noise, const double* w14,
                                   const double* deriv, const double* kf, const double* CN, int m, const double* H, const double* rm,
                                   int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov, double* jmean,
                                   double* jcov, double* mcnav, double* flights, double* xland, double* dx0, double* navfed,
                                   double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv) {
    const scvx::McRng rg{rng, noise};
    return scvx::track_mc_nav_q_host(ctx, B, K, S, x, u, sigma, gain, C0, x, noise ? x : nullptr, w14, deriv, kf, CN, x, x, m, H, rm, nsub,
                                     flags, tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, nq, ranks,
                                     flightq, pathq, pathv, &rg);
}

// the _veh forms: the _q call (rng == NULL) or the _rng call (its placeholders as above) with the vehicle errors behind it
int scvx_track_mc_nav_veh_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                              const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev,
                              const double* w14, const double* deriv_dev, const double* kf_dev, const double* CN_dev,
                              const double* xin_dev, const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags,
                              double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev,
                              double* mcnav_dev, double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev,
                              double* navK_dev, int nq, const int* ranks, double* flightq_dev, double* pathq_dev, double* pathv_dev,
                              const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh, const double* zeta_dev, double* theta_dev) {
    int rc = scvx::check_mc_veh_draws(ctx, rng, noise, xi0_dev, eta_dev, xin_dev, nud_dev, zeta_dev);
    if (rc) return rc;
    const scvx::McRng rg{rng, noise};
    const scvx::McVeh vh{veh, zeta_dev, theta_dev};
    if (rng) xi0_dev = xin_dev = nud_dev = x_dev, eta_dev = noise ? x_dev : nullptr;
    return scvx::track_mc_nav_q_dev(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev, kf_dev,
                                    CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev,
                                    jcov_dev, mcnav_dev, flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, nq, ranks, flightq_dev,
                                    pathq_dev, pathv_dev, rng ? &rg : nullptr, &vh);
}

int scvx_track_mc_nav_veh_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                   const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                                   const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                                   const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                                   double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                                   double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv,
                                   const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh, const double* zeta, double* theta) {
    int rc = scvx::check_mc_veh_draws(ctx, rng, noise, xi0, eta, xin, nud, zeta);
    if (rc) return rc;
    const scvx::McRng rg{rng, noise};
    const scvx::McVeh vh{veh, zeta, theta};
    if (rng) xi0 = xin = nud = x, eta = noise ? x : nullptr;
    return scvx::track_mc_nav_q_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w14, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags, tol,
                                     mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, nq, ranks, flightq, pathq,
                                     pathv, rng ? &rg : nullptr, &vh, "scvx_track_mc_nav_veh_f64_host");
}

int scvx_track_mc_nav_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* w14,
                          const double* deriv_dev, const double* kf_dev, const double* CN_dev, const double* xin_dev,
                          const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags, double tol,
                          double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev, double* mcnav_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev, double* navK_dev) {
    return scvx_track_mc_nav_q_f64(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev, kf_dev, CN_dev,
                                   xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev, jcov_dev,
                                   mcnav_dev, flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, 0, nullptr, nullptr, nullptr, nullptr);
}

int scvx_track_mc_nav_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                               const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                               const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                               double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                               double* navfed, double* navK) {
    return scvx_track_mc_nav_q_f64_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w14, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags,
                                        tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, 0, nullptr, nullptr,
                                        nullptr, nullptr);
}

int scvx_track_mc_nav_q_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                 const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                                 const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                                 const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                                 double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                                 double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv) {
    return scvx::track_mc_nav_q_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w14, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags, tol,
                                     mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, nq, ranks, flightq, pathq,
                                     pathv, nullptr);
}

}  // extern "C"

namespace scvx {

static int track_mc_nav_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                               const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                               const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                               double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                               double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv,
                               const McRng* rg, const McVeh* vh, const char* entry) {
    int rc = scvx::check_track_mc_nav(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w14, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags,
                                      tol, mcrep, xmean, xcov, jmean, jcov, mcnav);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if (rg) xi0 = eta = xin = nud = nullptr;   // placeholders until here: the lanes make the draws
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq, pathq))) return rc;
    if (vh && (rc = scvx::check_mc_vehicle(ctx, vh->v, vh->zeta, vh->theta, rg != nullptr))) return rc;
    if (vh && !vh->v) vh = nullptr;   // veh == NULL: the call without vehicle errors
    const Dims d(B, K, scvx_control_dim(ctx), S, m, nq);
    Staging s(ctx);
    McVeh dvh;   // the vehicle errors with zeta and theta on the device
    if (vh) dvh.v = vh->v, dvh.zeta = s.in(rg ? nullptr : vh->zeta, d.zeta), dvh.theta = s.out(vh->theta, d.theta);
    const double *dx = s.in(x, d.x), *du = s.in(u, d.u), *ds = s.in(sigma, d.b), *dg = s.in(gain, d.gain), *dc = s.in(C0, d.c14),
                 *di = s.in(xi0, d.xi), *de = s.in(eta, d.eta), *dd = s.in(deriv, d.deriv), *dk = s.in(m > 0 ? kf : nullptr, d.kf),
                 *dcn = s.in(CN, d.c14), *dxi = s.in(xin, d.xi), *dnu = s.in(m > 0 ? nud : nullptr, d.nud);
    double *dr = s.out(mcrep, d.mcrep), *dm = s.out(xmean, d.b14), *dv = s.out(xcov, d.c14), *djm = s.out(jmean, d.jmean),
           *djc = s.out(jcov, d.jcov), *dnv = s.out(mcnav, d.nrep), *df = s.out(flights, d.flights), *dl = s.out(xland, d.s14),
           *d0 = s.out(dx0, d.s14), *dfe = s.out(navfed, d.fed), *dnk = s.out(navK, d.s14);
    McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = s.out(flightq, d.flightq), q.pathq = s.out(pathq, d.pathq), q.pathv = s.out(pathv, d.pathv);
    s.launch([&] {
        return launch_track_mc_nav(ctx, B, K, S, dx, du, ds, dg, dc, di, de, w14, Tiles{dd, nullptr}, dk, dcn, dxi, dnu, m, H, rm, nsub, flags,
                                   tol, dr, dm, dv, djm, djc, dnv, df, dl, d0, dfe, dnk, s.st, (flightq || pathq || pathv) ? &q : nullptr, rg,
                                   vh ? &dvh : nullptr);
    });
    return s.finish(entry);
}

}  // namespace scvx
