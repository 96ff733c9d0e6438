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

// a workspace of the context (the partial rows; the dense values of a _q call), grown on demand: hipFree waits for whatever still reads
// the old one.  No two calls on one context may overlap on different streams.
static hipError_t mc_grow(double*& ws, size_t& have, size_t doubles) {
    if (have >= doubles) return hipSuccess;
    if (ws) (void)hipFree(ws);
    ws = nullptr;
    have = 0;
    hipError_t e = hipMalloc((void**)&ws, doubles * 8);
    if (e == hipSuccess) have = doubles;
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

// flights and q.pathv: the caller's dense buffers or nullptr on entry; on return where the flying kernel writes them -- the second
// workspace when only their order statistics are asked for (q.pathv == nullptr: the instantiations without per-node samples)
static hipError_t mc_q_buffers(scvx_ctx* ctx, McCall& c) {
    const size_t nf = (c.q.flightq && !c.flights) ? (size_t)c.B * c.S * SCVX_FLIGHT_NREP : 0;
    const size_t np = (c.q.pathq && !c.q.pathv) ? (size_t)c.B * (c.K + 1) * SCVX_PSIG_N * c.S : 0;
    if (nf + np == 0) return hipSuccess;
    hipError_t e = mc_grow(ctx->mcq_ws, ctx->mcq_ws_doubles, nf + np);
    if (e != hipSuccess) return e;
    if (nf) c.flights = ctx->mcq_ws;
    if (np) c.q.pathv = ctx->mcq_ws + nf;
    return hipSuccess;
}

// the order statistics of the sixteen flight columns (rows of S values 16 apart) and of every (b, k, f) row of pathv (contiguous)
static hipError_t mc_q_finish(const McCall& c, hipStream_t st) {
    hipError_t e = hipSuccess;
    if (c.q.flightq)
        e = launch_order_stats(c.B * SCVX_FLIGHT_NREP, c.S, c.flights, (size_t)c.S * SCVX_FLIGHT_NREP, SCVX_FLIGHT_NREP, 1,
                               SCVX_FLIGHT_NREP, c.q.nq, c.q.ranks, c.q.flightq, st);
    if (e == hipSuccess && c.q.pathq)
        e = launch_order_stats(c.B * (c.K + 1) * SCVX_PSIG_N, c.S, c.q.pathv, (size_t)c.S, 1, 0, 1, c.q.nq, c.q.ranks, c.q.pathq, st);
    return e;
}

hipError_t launch_mc(scvx_ctx* ctx, const McCall& dev, hipStream_t st) {
    McCall c = dev;   // flights, q.pathv and eta become what the flying kernel is given
    const int nblk = (c.S + 63) / 64;
    hipError_t e = mc_grow(ctx->mc_ws, ctx->mc_ws_doubles, (size_t)c.B * nblk * (c.nav ? MCN_NP : MC_NP) + (c.nav ? MCN_MODEL : 0));
    if (e != hipSuccess || (e = mc_q_buffers(ctx, c)) != hipSuccess) return e;
    McK m{};
    m.tol = c.tol;
    const McRngK rg = mc_noise(m, c);
    if (c.nav) {
        e = launch_mc_nav(ctx, c, m, rg, st);
    } else {
        e = launch_mc_fly<false, double>(ctx, c, m, rg, st);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(mc_finish_kernel, dim3((unsigned)c.B), dim3(256), 0, st, c.S, c.K, nblk, ctx->mc_ws, c.mcrep, c.xmean, c.xcov);
        e = hipGetLastError();
    }
    return e != hipSuccess ? e : mc_q_finish(c, st);
}

int check_mc_rng(scvx_ctx* ctx, const scvx_mc_rng* rng) {
    if (!ctx) return SCVX_ERR_ARG;
    if (!rng) return fail(ctx, SCVX_ERR_ARG, "mc rng: null rng");
    if (rng->reserved != 0) return fail(ctx, SCVX_ERR_ARG, "mc rng: reserved must be 0");
    if (rng->independent != 0 && rng->independent != 1) return fail(ctx, SCVX_ERR_ARG, "mc rng: independent must be 0 or 1");
    return SCVX_OK;
}

int check_mc_vehicle(scvx_ctx* ctx, const scvx_mc_vehicle* veh, const void* zeta, const void* theta, bool rng) {
    if (!ctx) return SCVX_ERR_ARG;
    if (!veh) {
        if (zeta || theta) return fail(ctx, SCVX_ERR_ARG, "vehicle: zeta / theta without veh");
        return SCVX_OK;
    }
    if (veh->reserved[0] != 0 || veh->reserved[1] != 0) return fail(ctx, SCVX_ERR_ARG, "vehicle: reserved must be 0");
    bool drawn = false;
    for (int i = 0; i < SCVX_VEH_N; i++) {
        if (!std::isfinite(veh->mu[i])) return fail(ctx, SCVX_ERR_ARG, "vehicle: mu must be finite");
        if (!(veh->sp[i] >= 0.0) || !std::isfinite(veh->sp[i])) return fail(ctx, SCVX_ERR_ARG, "vehicle: sp must be finite and >= 0");
        drawn = drawn || veh->sp[i] > 0.0;
    }
    if (!ctx->dyn.aero && (veh->mu[SCVX_VEH_AERO] != 0.0 || veh->sp[SCVX_VEH_AERO] != 0.0))
        return fail(ctx, SCVX_ERR_ARG, "vehicle: AERO on a model without aerodynamics");
    if (!ctx->dyn.fin && (veh->mu[SCVX_VEH_FIN] != 0.0 || veh->sp[SCVX_VEH_FIN] != 0.0))
        return fail(ctx, SCVX_ERR_ARG, "vehicle: FIN on a model without fins");
    if (!rng && drawn && !zeta) return fail(ctx, SCVX_ERR_ARG, "vehicle: sp > 0 needs zeta[S][6] (or rng)");
    return SCVX_OK;
}

// The order is the contract: a call with two faults is refused for the one that comes first here.  The words say "track mc" for what
// every form shares and "track mc nav" for what the flight on an estimate adds; the noise is checked where each family had it.
int check_mc_call(scvx_ctx* ctx, const McCall& c, const McBatch* batch) {
    if (!ctx) return SCVX_ERR_ARG;
    int rc;
    // the _veh forms' rule for the draws (no other form can break it): with rng nothing uploaded, without it no noise flag
    if (c.drawn && (c.xi0 || c.eta || c.xin || c.nud || c.veh.zeta))
        return fail(ctx, SCVX_ERR_ARG, "vehicle: with rng the uploaded draws (xi0, eta, xin, nud, zeta) must be NULL");
    if (!c.drawn && c.noise != 0) return fail(ctx, SCVX_ERR_ARG, "vehicle: noise without rng (pass eta)");
    if (batch && (rc = check_track_weights(ctx, batch->q14, batch->rNU, batch->qf14))) return rc;
    if (c.B < 1 || c.B > 65535) return fail(ctx, SCVX_ERR_ARG, "track mc: 1 <= B <= 65535 required");
    if (c.S < 1) return fail(ctx, SCVX_ERR_ARG, "track mc: S >= 1 required");
    if (c.K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "track mc: K must equal the problem's K");
    if (c.nsub < 1 || c.nsub > 1000) return fail(ctx, SCVX_ERR_ARG, "track mc: nsub must be in [1,1000]");
    if (c.flags & ~SCVX_TRACK_CLAMP) return fail(ctx, SCVX_ERR_ARG, "track mc: unknown flags (SCVX_TRACK_CLAMP)");
    if (!(c.tol >= 0.0) || !std::isfinite(c.tol)) return fail(ctx, SCVX_ERR_ARG, "track mc: tol must be finite and >= 0");
    const bool impulses = c.drawn ? c.noise != 0 : c.eta != nullptr;
    auto check_w = [&](const char* bad, const char* missing) {
        if (c.w)
            for (int i = 0; i < 14; i++)
                if (!(c.w[i] >= 0.0) || !std::isfinite(c.w[i])) return fail(ctx, SCVX_ERR_ARG, bad);
        return impulses && !c.w ? fail(ctx, SCVX_ERR_ARG, missing) : (int)SCVX_OK;
    };
    if (!c.nav && (rc = check_w("track mc: sw must be finite and >= 0", "track mc: eta without sw"))) return rc;
    if (c.reserved) return fail(ctx, SCVX_ERR_ARG, "track mc: the reserved argument must be NULL");
    const bool own = batch != nullptr;   // the plan, the gains, the tiles and kf are the batch's, the reduced outputs optional
    if (!(own || (c.x && c.u && c.sigma && c.gain && c.mcrep && c.xmean && c.xcov)) || !c.C0 || !(c.drawn || c.xi0))
        return fail(ctx, SCVX_ERR_ARG, "track mc: null buffer");
    if (ctx->prob.aero_kind == 1 && !ctx->dyn.aero)
        return fail(ctx, SCVX_ERR_STATE, "AtmosphericData problem: call scvx_set_aero_table first");
    if (c.nav) {
        if ((rc = check_w("track mc nav: w must be finite and >= 0", "track mc nav: eta without w14"))) return rc;
        if ((rc = check_nav_model(ctx, c.m, c.H, c.rm))) return rc;
        if (!(own || ((c.deriv.d || c.deriv.f) && c.jmean && c.jcov && c.mcnav)) || !c.CN || !(c.drawn || c.xin))
            return fail(ctx, SCVX_ERR_ARG, "track mc nav: null buffer (deriv, CN, xin, jmean, jcov, mcnav)");
        if (c.m > 0 && (!(own || c.kf) || !(c.drawn || c.nud)))
            return fail(ctx, SCVX_ERR_ARG, "track mc nav: m > 0 needs kf[B][K][14][m] and nud[S][K][m]");
        if (own && !batch->N0) return fail(ctx, SCVX_ERR_ARG, "track mc nav: null buffer (N0)");
    }
    if (c.drawn && (rc = check_mc_rng(ctx, c.rng))) return rc;
    // the _q arguments: with nothing of them asked for, the call they extend
    if ((c.q.nq != 0 || c.q.flightq || c.q.pathq) && (rc = check_ranks(ctx, c.S, c.q.nq, c.q.ranks))) return rc;
    return check_mc_vehicle(ctx, c.veh.v, c.veh.zeta, c.veh.theta, c.drawn);
}

// the buffers in the order the hand-written sequences declared them: the vehicle's, the inputs, the outputs, the order statistics
McCall stage_mc(Staging& s, const Dims& d, const McCall& host, bool reduced_always) {
    McCall v = host;
    auto reduced = [&](double* p, size_t n) { return reduced_always ? s.out_always(p, n) : s.out(p, n); };
    v.veh.zeta = s.in(host.veh.zeta, d.zeta), v.veh.theta = s.out(host.veh.theta, d.theta);
    v.x = s.in(host.x, d.x), v.u = s.in(host.u, d.u), v.sigma = s.in(host.sigma, d.b), v.gain = s.in(host.gain, d.gain);
    v.C0 = s.in(host.C0, d.c14), v.xi0 = s.in(host.xi0, d.xi), v.eta = s.in(host.eta, d.eta);
    if (host.nav) {   // kf and nud are read with m > 0 only
        v.deriv.d = s.in(host.deriv.d, d.deriv), v.kf = s.in(host.m > 0 ? host.kf : nullptr, d.kf), v.CN = s.in(host.CN, d.c14);
        v.xin = s.in(host.xin, d.xi), v.nud = s.in(host.m > 0 ? host.nud : nullptr, d.nud);
    }
    v.mcrep = reduced(host.mcrep, d.mcrep), v.xmean = reduced(host.xmean, d.b14), v.xcov = reduced(host.xcov, d.c14);
    if (host.nav) v.jmean = reduced(host.jmean, d.jmean), v.jcov = reduced(host.jcov, d.jcov), v.mcnav = reduced(host.mcnav, d.nrep);
    v.flights = s.out(host.flights, d.flights), v.xland = s.out(host.xland, d.s14), v.dx0 = s.out(host.dx0, d.s14);
    v.navfed = s.out(host.navfed, d.fed), v.navK = s.out(host.navK, d.s14);
    v.q.flightq = s.out(host.q.flightq, d.flightq), v.q.pathq = s.out(host.q.pathq, d.pathq), v.q.pathv = s.out(host.q.pathv, d.pathv);
    return v;
}

int mc_call_dev(scvx_ctx* ctx, const McCall& c) {
    int rc = check_mc_call(ctx, c);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, launch_mc(ctx, c, ctx->stream));
    return SCVX_OK;
}

int mc_call_host(scvx_ctx* ctx, const McCall& c, const char* entry) {
    int rc = check_mc_call(ctx, c);
    if (rc) return rc;
    const Dims d(c.B, c.K, scvx_control_dim(ctx), c.S, c.m, c.q.nq);
    Staging s(ctx);
    const McCall dev = stage_mc(s, d, c, false);
    s.launch([&] { return launch_mc(ctx, dev, s.st); });
    return s.finish(entry);
}

// one lane per (plan, s): the draws the _rng forms consume (mc_draws_kernel); any of the four outputs may be nullptr
hipError_t launch_mc_draws(const scvx_mc_rng& r, int P, int S, int K, double* xi0, double* eta, double* xin, double* nud, hipStream_t st) {
    hipLaunchKernelGGL(mc_draws_kernel, dim3((unsigned)((S + 63) / 64), (unsigned)P), dim3(64), 0, st, mc_rng_k(r, false), S, K, xi0, eta,
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

// Every entry point below fills one record from its arguments.  The _q forms take the uploaded draws; the _rng forms have the lanes make
// them; the _veh forms are either, by rng, with the vehicle errors; the forms without a suffix are the _q forms with nothing of q.
int scvx_track_mc_q_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                        const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                        const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                        double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                        double* pathq_dev, double* pathv_dev) {
    scvx::McCall c;
    c.B = B, c.K = K, c.S = S, c.x = x_dev, c.u = u_dev, c.sigma = sigma_dev, c.gain = gain_dev, c.C0 = C0_dev, c.w = sw14;
    c.reserved = reserved, c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep_dev, c.xmean = xmean_dev, c.xcov = xcov_dev;
    c.flights = flights_dev, c.xland = xland_dev, c.dx0 = dx0_dev, c.q = {nq, ranks, flightq_dev, pathq_dev, pathv_dev}, c.xi0 = xi0_dev;
    c.eta = eta_dev;
    return scvx::mc_call_dev(ctx, c);
}

int scvx_track_mc_rng_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const scvx_mc_rng* rng, int noise, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev) {
    scvx::McCall c;
    c.B = B, c.K = K, c.S = S, c.x = x_dev, c.u = u_dev, c.sigma = sigma_dev, c.gain = gain_dev, c.C0 = C0_dev, c.w = sw14;
    c.reserved = reserved, c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep_dev, c.xmean = xmean_dev, c.xcov = xcov_dev;
    c.flights = flights_dev, c.xland = xland_dev, c.dx0 = dx0_dev, c.q = {nq, ranks, flightq_dev, pathq_dev, pathv_dev}, c.drawn = true;
    c.rng = rng, c.noise = noise;
    return scvx::mc_call_dev(ctx, c);
}

int scvx_track_mc_veh_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                          const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                          const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                          double* flights_dev, double* xland_dev, double* dx0_dev, int nq, const int* ranks, double* flightq_dev,
                          double* pathq_dev, double* pathv_dev, const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh,
                          const double* zeta_dev, double* theta_dev) {
    scvx::McCall c;
    c.B = B, c.K = K, c.S = S, c.x = x_dev, c.u = u_dev, c.sigma = sigma_dev, c.gain = gain_dev, c.C0 = C0_dev, c.w = sw14;
    c.reserved = reserved, c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep_dev, c.xmean = xmean_dev, c.xcov = xcov_dev;
    c.flights = flights_dev, c.xland = xland_dev, c.dx0 = dx0_dev, c.q = {nq, ranks, flightq_dev, pathq_dev, pathv_dev}, c.xi0 = xi0_dev;
    c.eta = eta_dev, c.drawn = rng != nullptr, c.rng = rng, c.noise = noise, c.veh = {veh, zeta_dev, theta_dev};
    return scvx::mc_call_dev(ctx, c);
}

int scvx_track_mc_f64(scvx_ctx* ctx, int B, int K, int S, const double* x_dev, const double* u_dev, const double* sigma_dev,
                      const double* gain_dev, const double* C0_dev, const double* xi0_dev, const double* eta_dev, const double* sw14,
                      const void* reserved, int nsub, int flags, double tol, double* mcrep_dev, double* xmean_dev, double* xcov_dev,
                      double* flights_dev, double* xland_dev, double* dx0_dev) {
    return scvx_track_mc_q_f64(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, sw14, reserved, nsub, flags, tol,
                               mcrep_dev, xmean_dev, xcov_dev, flights_dev, xland_dev, dx0_dev, 0, nullptr, nullptr, nullptr, nullptr);
}

int scvx_track_mc_q_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                             const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                             int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland,
                             double* dx0, int nq, const int* ranks, double* flightq, double* pathq, double* pathv) {
    scvx::McCall c;
    c.B = B, c.K = K, c.S = S, c.x = x, c.u = u, c.sigma = sigma, c.gain = gain, c.C0 = C0, c.w = sw14, c.reserved = reserved;
    c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep, c.xmean = xmean, c.xcov = xcov, c.flights = flights, c.xland = xland;
    c.dx0 = dx0, c.q = {nq, ranks, flightq, pathq, pathv}, c.xi0 = xi0, c.eta = eta;
    return scvx::mc_call_host(ctx, c, "scvx_track_mc_q_f64_host");
}

int scvx_track_mc_rng_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const scvx_mc_rng* rng, int noise, const double* sw14,
                               const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                               double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                               double* pathv) {
    scvx::McCall c;
    c.B = B, c.K = K, c.S = S, c.x = x, c.u = u, c.sigma = sigma, c.gain = gain, c.C0 = C0, c.w = sw14, c.reserved = reserved;
    c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep, c.xmean = xmean, c.xcov = xcov, c.flights = flights, c.xland = xland;
    c.dx0 = dx0, c.q = {nq, ranks, flightq, pathq, pathv}, c.drawn = true, c.rng = rng, c.noise = noise;
    return scvx::mc_call_host(ctx, c, "scvx_track_mc_rng_f64_host");
}

int scvx_track_mc_veh_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* sw14,
                               const void* reserved, int nsub, int flags, double tol, double* mcrep, double* xmean, double* xcov,
                               double* flights, double* xland, double* dx0, int nq, const int* ranks, double* flightq, double* pathq,
                               double* pathv, const scvx_mc_rng* rng, int noise, const scvx_mc_vehicle* veh, const double* zeta,
                               double* theta) {
    scvx::McCall c;
    c.B = B, c.K = K, c.S = S, c.x = x, c.u = u, c.sigma = sigma, c.gain = gain, c.C0 = C0, c.w = sw14, c.reserved = reserved;
    c.nsub = nsub, c.flags = flags, c.tol = tol, c.mcrep = mcrep, c.xmean = xmean, c.xcov = xcov, c.flights = flights, c.xland = xland;
    c.dx0 = dx0, c.q = {nq, ranks, flightq, pathq, pathv}, c.xi0 = xi0, c.eta = eta, c.drawn = rng != nullptr, c.rng = rng;
    c.noise = noise, c.veh = {veh, zeta, theta};
    return scvx::mc_call_host(ctx, c, "scvx_track_mc_veh_f64_host");
}

int scvx_track_mc_f64_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma, const double* gain,
                           const double* C0, const double* xi0, const double* eta, const double* sw14, const void* reserved, int nsub,
                           int flags, double tol, double* mcrep, double* xmean, double* xcov, double* flights, double* xland, double* dx0) {
    return scvx_track_mc_q_f64_host(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, sw14, reserved, nsub, flags, tol, mcrep, xmean, xcov,
                                    flights, xland, dx0, 0, nullptr, nullptr, nullptr, nullptr);
}

}  // extern "C"
