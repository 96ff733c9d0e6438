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

// The flight on an estimate and its reduction, for launch_mc (scvx_mc.hip), which has grown the workspace and prepared the record: the
// measurement model into the workspace, the flights with the tiles as they are stored -- deriv.d ? <double> : <float>, in that order
// (profiles/host_staging.md) -- and the finish kernel.
hipError_t launch_mc_nav(scvx_ctx* ctx, const McCall& c, const McK& m, const McRngK& rg, hipStream_t st) {
    McNavK nv{};
    for (int i = 0; i < c.m; i++) nv.srm[i] = std::sqrt(c.rm[i]);
    for (int i = 0; i < c.m * 14; i++) nv.H[i] = c.H[i];
    hipLaunchKernelGGL(mc_nav_model_kernel, dim3(1), dim3(256), 0, st, nv, mc_nav_model(ctx, c));
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = c.deriv.d ? launch_mc_fly<true, double>(ctx, c, m, rg, st) : launch_mc_fly<true, float>(ctx, c, m, rg, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mc_nav_finish_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.S, c.K, (c.S + 63) / 64, ctx->mc_ws, c.mcrep, c.xmean,
                       c.xcov, c.jmean, c.jcov, c.mcnav);
    return hipGetLastError();
}

}  // namespace scvx

extern "C" {

// Every entry point below fills one record from its arguments, as those of scvx_mc.hip do, with nav set and the estimate's group.
int scvx_track_mc_nav_q_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                            const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* w14,
                            const double* deriv_dev, const double* kf_dev, const double* CN_dev, const double* xin_dev,
                            const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags, double tol,
                            double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev, double* mcnav_dev,
                            double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev, double* navK_dev, int nq,
                            const int* ranks, double* flightq_dev, double* pathq_dev, double* pathv_dev) {
    scvx::McCall c;
    c.nav = true, c.B = B, c.K = K, c.S = S, c.x = x_dev, c.u = u_dev, c.sigma = sigma_dev, c.gain = gain_dev, c.C0 = C0_dev, c.w = w14;
    c.deriv.d = deriv_dev, c.kf = kf_dev, c.CN = CN_dev, c.m = m, c.H = H, c.rm = rm, c.nsub = nsub, c.flags = flags, c.tol = tol;
    c.mcrep = mcrep_dev, c.xmean = xmean_dev, c.xcov = xcov_dev, c.jmean = jmean_dev, c.jcov = jcov_dev, c.mcnav = mcnav_dev;
    c.flights = flights_dev, c.xland = xland_dev, c.dx0 = dx0_dev, c.navfed = navfed_dev, c.navK = navK_dev;
    c.q = {nq, ranks, flightq_dev, pathq_dev, pathv_dev}, c.xi0 = xi0_dev, c.eta = eta_dev, c.xin = xin_dev, c.nud = nud_dev;
    return scvx::mc_call_dev(ctx, c);
}

int scvx_track_mc_nav_rng_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                              const double* gain_dev, const double* C0_dev, const scvx_mc_rng* rng, int noise, const double* w14,
                              const double* deriv_dev, const double* kf_dev, const double* CN_dev, int m, const double* H,
                              const double* rm, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                              double* jmean_dev, double* jcov_dev, double* mcnav_dev, double* flights_dev, double* xland_dev,
                              double* dx0_dev, double* navfed_dev, double* navK_dev, int nq, const int* ranks, double* flightq_dev,
                              double* pathq_dev, double* pathv_dev) {
    scvx::McCall c;
    c.nav = true, c.B = B, c.K = K, c.S = S, c.x = x_dev, c.u = u_dev, c.sigma = sigma_dev, c.gain = gain_dev, c.C0 = C0_dev, c.w = w14;
    c.deriv.d = deriv_dev, c.kf = kf_dev, c.CN = CN_dev, c.m = m, c.H = H, c.rm = rm, c.nsub = nsub, c.flags = flags, c.tol = tol;
    c.mcrep = mcrep_dev, c.xmean = xmean_dev, c.xcov = xcov_dev, c.jmean = jmean_dev, c.jcov = jcov_dev, c.mcnav = mcnav_dev;
    c.flights = flights_dev, c.xland = xland_dev, c.dx0 = dx0_dev, c.navfed = navfed_dev, c.navK = navK_dev;
    c.q = {nq, ranks, flightq_dev, pathq_dev, pathv_dev}, c.drawn = true, c.rng = rng, c.noise = noise;
    return scvx::mc_call_dev(ctx, c);
}

int scvx_track_mc_nav_veh_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                              const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev,
                              const double* w14, const double* deriv_dev, const double* kf_dev, const double* CN_dev,
                              const double* xin_dev, const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags,
                              double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev,
                              double* mcnav_dev, double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev,
                              double* navK_dev, int nq, const int* ranks, double* flightq_dev, double* pathq_dev, double* pathv_dev,
                              const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh, const double* zeta_dev, double* theta_dev) {
    scvx::McCall c;
    c.nav = true, c.B = B, c.K = K, c.S = S, c.x = x_dev, c.u = u_dev, c.sigma = sigma_dev, c.gain = gain_dev, c.C0 = C0_dev, c.w = w14;
    c.deriv.d = deriv_dev, c.kf = kf_dev, c.CN = CN_dev, c.m = m, c.H = H, c.rm = rm, c.nsub = nsub, c.flags = flags, c.tol = tol;
    c.mcrep = mcrep_dev, c.xmean = xmean_dev, c.xcov = xcov_dev, c.jmean = jmean_dev, c.jcov = jcov_dev, c.mcnav = mcnav_dev;
    c.flights = flights_dev, c.xland = xland_dev, c.dx0 = dx0_dev, c.navfed = navfed_dev, c.navK = navK_dev;
    c.q = {nq, ranks, flightq_dev, pathq_dev, pathv_dev}, c.xi0 = xi0_dev, c.eta = eta_dev, c.xin = xin_dev, c.nud = nud_dev;
    c.drawn = rng != nullptr, c.rng = rng, c.noise = noise, c.veh = {veh, zeta_dev, theta_dev};
    return scvx::mc_call_dev(ctx, c);
}

int scvx_track_mc_nav_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* w14,
                          const double* deriv_dev, const double* kf_dev, const double* CN_dev, const double* xin_dev,
                          const double* nud_dev, int m, const double* H, const double* rm, int nsub, int flags, double tol,
                          double* mcrep_dev, double* xmean_dev, double* xcov_dev, double* jmean_dev, double* jcov_dev, double* mcnav_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, double* navfed_dev, double* navK_dev) {
    return scvx_track_mc_nav_q_f64(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev, kf_dev,
                                   CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev,
                                   jcov_dev, mcnav_dev, flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev, 0, nullptr, nullptr,
                                   nullptr, nullptr);
}

int scvx_track_mc_nav_q_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                 const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                                 const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                                 const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                                 double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                                 double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv) {
    scvx::McCall c;
    c.nav = true, c.B = B, c.K = K, c.S = S, c.x = x, c.u = u, c.sigma = sigma, c.gain = gain, c.C0 = C0, c.w = w14, c.deriv.d = deriv;
    c.kf = kf, c.CN = CN, c.m = m, c.H = H, c.rm = rm, c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep, c.xmean = xmean;
    c.xcov = xcov, c.jmean = jmean, c.jcov = jcov, c.mcnav = mcnav, c.flights = flights, c.xland = xland, c.dx0 = dx0, c.navfed = navfed;
    c.navK = navK, c.q = {nq, ranks, flightq, pathq, pathv}, c.xi0 = xi0, c.eta = eta, c.xin = xin, c.nud = nud;
    return scvx::mc_call_host(ctx, c, "scvx_track_mc_nav_q_f64_host");
}

int scvx_track_mc_nav_rng_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                   const double* gain, const double* C0, const scvx_mc_rng* rng, int noise, const double* w14,
                                   const double* deriv, const double* kf, const double* CN, int m, const double* H, const double* rm,
                                   int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov, double* jmean,
                                   double* jcov, double* mcnav, double* flights, double* xland, double* dx0, double* navfed, double* navK,
                                   int nq, const int* ranks, double* flightq, double* pathq, double* pathv) {
    scvx::McCall c;
    c.nav = true, c.B = B, c.K = K, c.S = S, c.x = x, c.u = u, c.sigma = sigma, c.gain = gain, c.C0 = C0, c.w = w14, c.deriv.d = deriv;
    c.kf = kf, c.CN = CN, c.m = m, c.H = H, c.rm = rm, c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep, c.xmean = xmean;
    c.xcov = xcov, c.jmean = jmean, c.jcov = jcov, c.mcnav = mcnav, c.flights = flights, c.xland = xland, c.dx0 = dx0, c.navfed = navfed;
    c.navK = navK, c.q = {nq, ranks, flightq, pathq, pathv}, c.drawn = true, c.rng = rng, c.noise = noise;
    return scvx::mc_call_host(ctx, c, "scvx_track_mc_nav_rng_f64_host");
}

int scvx_track_mc_nav_veh_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                   const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                                   const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                                   const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                                   double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                                   double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv,
                                   const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh, const double* zeta, double* theta) {
    scvx::McCall c;
    c.nav = true, c.B = B, c.K = K, c.S = S, c.x = x, c.u = u, c.sigma = sigma, c.gain = gain, c.C0 = C0, c.w = w14, c.deriv.d = deriv;
    c.kf = kf, c.CN = CN, c.m = m, c.H = H, c.rm = rm, c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep, c.xmean = xmean;
    c.xcov = xcov, c.jmean = jmean, c.jcov = jcov, c.mcnav = mcnav, c.flights = flights, c.xland = xland, c.dx0 = dx0, c.navfed = navfed;
    c.navK = navK, c.q = {nq, ranks, flightq, pathq, pathv}, c.xi0 = xi0, c.eta = eta, c.xin = xin, c.nud = nud, c.drawn = rng != nullptr;
    c.rng = rng, c.noise = noise, c.veh = {veh, zeta, theta};
    return scvx::mc_call_host(ctx, c, "scvx_track_mc_nav_veh_f64_host");
}

int scvx_track_mc_nav_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                               const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                               const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                               double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                               double* navfed, double* navK) {
    return scvx_track_mc_nav_q_f64_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w14, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags,
                                        tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, 0, nullptr,
                                        nullptr, nullptr, nullptr);
}

}  // extern "C"
