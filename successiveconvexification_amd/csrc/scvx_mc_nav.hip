// Sampled closed-loop dispersion flown on a navigation ESTIMATE (scvx_track_mc_nav_f64, include/scvx.h): scvx_track_mc_f64's S flights
// per plan with the law fed x_fly - eps+_k, the error eps of the estimate generated per flight on the device from the filter gains of
// the navigation analysis (scvx_nav.hip), with measurement noise and with the process noise that hits the truth.  No counterpart in the
// reference.
//
// mc_nav_fly_kernel keeps mc_fly_kernel's shape (scvx_mc.hip): ONE LANE PER FLIGHT, a wavefront = 64 consecutive samples of one plan,
// grid (ceil(S / 64), B).  The plan, its gains, the state block A_k of its derivative tile and the filter gains Kf_k are one address per
// wavefront (blockIdx.y and the loop counters only): scalar loads -- except the three matrices of the error's recursion.  A_k (196
// doubles), Kf_k (14 m) and H (14 m) read element by element through scalar loads cost about 36 cycles per element on the MI355X (the
// strided loads do not merge; 1.31 x scvx_track_mc_f64 at m = 0, 1.49 x at m = 6 on the exo model), and H from the kernel argument is
// kept in scalar registers for the whole flight, several hundred of them spilled.  So the wave fetches A_k and Kf_k with one coalesced
// load per 64 elements -- node k + 1's while segment k is integrated -- and parks them in LDS, where every lane reads them at one address
// (a broadcast); H and sqrt(rm) are copied by a small launch into the context's workspace behind the partial rows and from there into LDS
// once.  Only the draws xi0, eta, xin, nud are per lane.  eps [14] is in registers at the node: the innovation H eps + sqrt(rm) nud (m
// values, formed before eps is touched), eps+ = eps - Kf innovation, the feedback on (x_fly - eps+) - xbar, and eps_{k+1} = A_k eps+
// (+ sqrt(w) eta_k) BEFORE the segment's RK4 loop; while the segment is integrated eps rests in LDS as well (a column per lane; 12 KB of
// LDS per block in all).  The flight arithmetic is mc_fly_kernel's statement for statement: with eps = 0 a flight is bitwise that
// kernel's, and with the eps+ this kernel wrote fed to scvx_track_fly_nav_f64 as `nav` a flight's 16 columns are bitwise that flyer's
// (tests/test_gpu_mc_nav.py).  It is a kernel of its own, in a translation unit of its own, so that mc_fly_kernel and fly_kernel keep
// their code exactly (profiles/mc_nav.md).  A non-finite eps poisons its flight through `bad`, whichever node it appears at.  DS is the
// tiles' storage type (double, or float with scvx_batch_set_linearization_f32: widened on load, as nav_cov_kernel does).
//
// Reduction as in scvx_mc.hip: a fixed xor butterfly per wavefront, one partial row [MCN_NP] per block in the context's workspace,
// mc_nav_finish_kernel (one block per plan) combining the blocks in order.  The row is mc_fly_kernel's, then the sums of eps_K [14] and
// of the upper triangle of [e; eps_K][e; eps_K]' [406], and the largest |eps+_k|_inf fed.  The 14 x 14 corner of the triangle is written
// to MC_EE as well and every landing statistic is formed by one expression, so xcov is bitwise jcov[:, :14, :14].
//
// RNG (the last template parameter, as in scvx_mc.hip): the four loads of draws become calls of mc_draw_group (scvx_rng.hpp).  eta_k is
// formed once, at the error's time step, and rests in LDS (a column per lane, 7 KB per block) until the truth's impulse behind the
// segment; of nud_k only the blocks that hold its first m draws are formed.  With RNG off the instantiations keep the parent's registers,
// LDS and scratch (profiles/mc_rng.md).
#include <cmath>
#include <limits>
#include "scvx_mc.hpp"

namespace scvx {

struct McNavK {
    double H[196];    // [m][14]
    double srm[14];   // sqrt(rm)
};
constexpr int MCN_SRM = 196, MCN_MODEL = 210;

// the measurement model from the kernel argument of this small launch into the workspace, in stream order behind whatever still reads it
__global__ __launch_bounds__(256) void mc_nav_model_kernel(McNavK nv, double* __restrict__ dst) {
    const int t = threadIdx.x;
    if (t < MCN_SRM) dst[t] = nv.H[t];
    else if (t < MCN_MODEL) dst[t] = nv.srm[t - MCN_SRM];
}

// square root of a variance (a rounded variance of -1e-40 is 0, a NaN stays a NaN)
__device__ __forceinline__ double mcn_sd(double v) { return v > 0.0 ? sqrt(v) : (v != v ? v : 0.0); }

template <bool AERO, bool FIN, bool TRQ, typename DS, bool PV, bool RNG>
__global__ __launch_bounds__(64) void mc_nav_fly_kernel(DynPK<double, TRQ> p, PathK c, McK m, int mm, const double* __restrict__ hm, int S, int K,
                                                        const double* __restrict__ x, const double* __restrict__ u,
                                                        const double* __restrict__ sigma, const double* __restrict__ gain,
                                                        const double* __restrict__ C0, const double* __restrict__ xi0,
                                                        const double* __restrict__ eta, const DS* __restrict__ deriv,
                                                        const double* __restrict__ kf, const double* __restrict__ CN,
                                                        const double* __restrict__ xin, const double* __restrict__ nud, double dt,
                                                        int nsub, int opt, double* __restrict__ part, double* __restrict__ flights,
                                                        double* __restrict__ xland, double* __restrict__ dx0o,
                                                        double* __restrict__ navfed, double* __restrict__ navK,
                                                        double* __restrict__ pathv, McRngK rg) {
    // hm: H [m][14] then sqrt(rm) at MCN_SRM, in the workspace behind the partial rows
    typedef double R;
    __shared__ R epl[14][64];   // eps rests here while the segment is integrated: one column per lane, no lane reads another's
    __shared__ R Al[196], Kl[196], Hl[MCN_MODEL];   // A_k, Kf_k and the model: written by the wave, read by every lane at one address
    __shared__ R etl[RNG ? 14 : 1][64];   // RNG: eta_k rests here between the error's time step and the truth's impulse, a column per lane
    const int ln = threadIdx.x;
    const int b = blockIdx.y;
    const int sl = blockIdx.x * 64 + threadIdx.x;
    const bool live = sl < S;
    const int s_ = live ? sl : S - 1;
    constexpr int NU = FIN ? 5 : 3;
    constexpr int n = 14 + NU;
    constexpr int DSZ = 14 * (14 + 2 * NU + 1);   // one derivative tile, column-major [14 + 2 NU + 1][14]: A_k is its first 14 columns
    const R* xb = x + (size_t)b * (K + 1) * 14;
    const R* ub = u + (size_t)b * (K + 1) * NU;
    const R* gb = gain + (size_t)b * K * NU * n;
    const R* cb = C0 + (size_t)b * 196;
    const R* cnb = CN + (size_t)b * 196;
    const DS* tb = deriv + (size_t)b * K * DSZ;
    const R* kb = mm > 0 ? kf + (size_t)b * K * 14 * mm : nullptr;
    const R* xi = RNG ? nullptr : xi0 + (size_t)s_ * 14;
    const R* et = (!RNG && eta) ? eta + (size_t)s_ * K * 14 : nullptr;
    const R* xn_ = RNG ? nullptr : xin + (size_t)s_ * 14;
    const R* nd = (!RNG && mm > 0) ? nud + (size_t)s_ * K * mm : nullptr;
    const uint64_t rc2 = RNG ? mc_rng_c2(rg, b) : 0, rc3 = RNG ? mc_rng_c3(rg, s_) : 0;   // RNG: the flight's streams, scvx_rng.hpp
    const size_t fl = (size_t)b * S + s_;
    const R sig = sigma[b];
    const R h = dt / R(nsub);
    const R inv_n = R(1.0) / R(nsub);
    const R ninf = -std::numeric_limits<double>::infinity();
    const bool clamp = (opt & SCVX_TRACK_CLAMP) != 0;
    R xs[14], ukv[NU], upv[NU], eps[14];
    // ---- the start: dx0 = C0 xi0 and eps_0 = CN xin, summed with fma in ascending j ----
    {
        R xv[16];
        if (RNG) {
            mc_draw_group(rg.seed, MC_STREAM_TRUTH, rc2, rc3, 0, 14, xv);
        } else {
#pragma unroll
            for (int j = 0; j < 14; j++) xv[j] = xi[j];
        }
#pragma unroll
        for (int i = 0; i < 14; i++) {
            R a = R(0.0);
#pragma unroll
            for (int j = 0; j < 14; j++) a = fma(cb[i * 14 + j], xv[j], a);
            if (dx0o && live) dx0o[fl * 14 + i] = a;
            xs[i] = a;
        }
        if (RNG) {
            mc_draw_group(rg.seed, MC_STREAM_NAV, rc2, rc3, 0, 14, xv);
        } else {
#pragma unroll
            for (int j = 0; j < 14; j++) xv[j] = xn_[j];
        }
#pragma unroll
        for (int i = 0; i < 14; i++) {
            R a = R(0.0);
#pragma unroll
            for (int j = 0; j < 14; j++) a = fma(cnb[i * 14 + j], xv[j], a);
            eps[i] = a;
        }
    }
#pragma unroll
    for (int i = 0; i < 14; i++) epl[i][ln] = eps[i];
#pragma unroll
    for (int i = 0; i < 14; i++) xs[i] = xb[i] + xs[i];
#pragma unroll
    for (int j = 0; j < NU; j++) upv[j] = ub[j];
    R gap = R(0.0), bad = R(0.0);   // bad: 0 while every sampled state, node difference and eps is finite, else NaN
    R g_mass = ninf, g_glide = ninf, g_tilt = ninf, g_rate = ninf, g_tmax = ninf, g_tmin = ninf, g_gimbal = ninf, g_dp = ninf,
      g_fin = ninf, qn = R(0.0), fedmax = R(0.0);
    int n_lo = 0, n_hi = 0;         // commanded node controls k = 1..K outside the thrust band by more than tol, before the clamp
#pragma unroll
    for (int i = 0; i < 14; i++) bad = fma(eps[i], R(0.0), bad);
    // A_k and Kf_k of node 0 (a lane fetches elements ln, ln + 64, ..), and the model
    DS pre[4];
    R prk[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int e = ln + 64 * q;
        pre[q] = e < 196 ? tb[e] : DS(0);
        prk[q] = (mm > 0 && e < 14 * mm) ? kb[e] : R(0.0);
    }
    if (mm > 0)
        for (int e = ln; e < MCN_MODEL; e += 64) Hl[e] = hm[e];
    // PV: the five path functions at every node, as mc_fly_kernel stores them: of the TRUTH xs (the constraints bind the vehicle), the
    // thrust norm of the command formed from the estimate
    R* pvb = PV ? pathv + (size_t)b * (K + 1) * SCVX_PSIG_N * S + s_ : nullptr;
    if (PV && live) pvb[(size_t)SCVX_PSIG_THRUST * S] = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
    for (int k = 0; k < K; k++) {
        if (PV && live) mc_path_store(pvb + (size_t)k * SCVX_PSIG_N * S, S, c.tggs, xs);
        __syncthreads();   // the readers of the previous node's A and Kf are done
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = ln + 64 * q;
            if (e < 196) {
                Al[e] = (R)pre[q];
                Kl[e] = prk[q];
            }
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < 14; i++) eps[i] = epl[i][ln];
        // ---- node k: the measurement update of the estimate's error, eps+ = eps - Kf (H eps + sqrt(rm) nud) ----
        if (mm > 0) {
            R inn[14];
            R zn[16];   // RNG: nud_k, the first mm draws of group 1 + k of the navigation stream
            if (RNG) mc_draw_group(rg.seed, MC_STREAM_NAV, rc2, rc3, 1 + k, mm, zn);
#pragma unroll
            for (int r = 0; r < 14; r++) {
                inn[r] = R(0.0);
                if (r < mm) {
                    R a = Hl[MCN_SRM + r] * (RNG ? zn[r] : nd[(size_t)k * mm + r]);
#pragma unroll
                    for (int j = 0; j < 14; j++) a = fma(Hl[r * 14 + j], eps[j], a);
                    inn[r] = a;
                }
            }
#pragma unroll
            for (int r = 0; r < 14; r++) {
                if (r < mm) {
#pragma unroll
                    for (int i = 0; i < 14; i++) eps[i] = fma(-Kl[i * mm + r], inn[r], eps[i]);
                }
            }
        }
        // eps holds eps+_k
#pragma unroll
        for (int i = 0; i < 14; i++) {
            fedmax = nan_max(fedmax, fabs(eps[i]));
            if (navfed && live) navfed[(fl * K + k) * 14 + i] = eps[i];
        }
        // ---- node k: the next node's control from the ESTIMATE of the flown state and the applied control ----
        {
            R z[n];
#pragma unroll
            for (int i = 0; i < 14; i++) z[i] = (xs[i] - eps[i]) - xb[(size_t)k * 14 + i];
#pragma unroll
            for (int j = 0; j < NU; j++) {
                z[14 + j] = upv[j] - ub[(size_t)k * NU + j];
                ukv[j] = upv[j];
            }
            const R* g = gb + (size_t)k * NU * n;
#pragma unroll
            for (int j = 0; j < NU; j++) {
                R a = ub[(size_t)(k + 1) * NU + j];
#pragma unroll
                for (int i = 0; i < n; i++) a = fma(g[j * n + i], z[i], a);
                upv[j] = a;
            }
            {
                const R un = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
                n_lo += (c.Tmin - un > m.tol) ? 1 : 0;
                n_hi += (un - c.Tmax > m.tol) ? 1 : 0;
                if (PV && live) pvb[((size_t)(k + 1) * SCVX_PSIG_N + SCVX_PSIG_THRUST) * S] = un;
            }
            if (clamp) {
                const R un = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
                R f = R(1.0);
                if (un > c.Tmax) f = c.Tmax / un;
                else if (un < c.Tmin && un > R(0.0)) f = c.Tmin / un;
#pragma unroll
                for (int j = 0; j < 3; j++) upv[j] *= f;
                if (FIN) {
                    const R fn = sqrt(upv[3] * upv[3] + upv[4] * upv[4]);
                    const R ff = fn > c.finmxf ? c.finmxf / fn : R(1.0);
                    upv[3] *= ff;
                    upv[4] *= ff;
                }
            }
        }
        // ---- the time step of the error: eps_{k+1} = A_k eps+_k (+ sqrt(w) eta_k, the impulse the truth receives below) ----
        {
            R ep[14];
#pragma unroll
            for (int i = 0; i < 14; i++) ep[i] = eps[i];
            R ev[16];   // RNG: eta_k, group 1 + k of the truth's stream, formed here once
            if (RNG && rg.noise) {
                mc_draw_group(rg.seed, MC_STREAM_TRUTH, rc2, rc3, 1 + k, 14, ev);
#pragma unroll
                for (int i = 0; i < 14; i++) etl[i][ln] = ev[i];
            }
#pragma unroll
            for (int i = 0; i < 14; i++) {
                R a = R(0.0);
#pragma unroll
                for (int j = 0; j < 14; j++) a = fma(Al[j * 14 + i], ep[j], a);
                if (RNG) {
                    if (rg.noise) a = fma(m.sw[i], ev[i], a);
                } else if (et) a = fma(m.sw[i], et[(size_t)k * 14 + i], a);
                epl[i][ln] = a;
                bad = fma(a, R(0.0), bad);
            }
        }
        // A and Kf of node k + 1, in flight while the segment is integrated
        if (k + 1 < K) {
            const DS* t = tb + (size_t)(k + 1) * DSZ;
#pragma unroll
            for (int q = 0; q < 4; q++) {
                const int e = ln + 64 * q;
                pre[q] = e < 196 ? t[e] : DS(0);
                prk[q] = (mm > 0 && e < 14 * mm) ? kb[(size_t)(k + 1) * 14 * mm + e] : R(0.0);
            }
        }
        for (int s = 0; s <= nsub; s++) {
            // ---- sample: state xs, control of the hold at s / nsub (the stage-0 control of substep s) ----
            const R lk0 = R(s) * inv_n;
            R us[NU];
#pragma unroll
            for (int j = 0; j < NU; j++) us[j] = fma(ukv[j], R(1.0) - lk0, upv[j] * lk0);
            const R un = sqrt(us[0] * us[0] + us[1] * us[1] + us[2] * us[2]);
            g_tmax = nan_max(g_tmax, un - c.Tmax);
            g_tmin = nan_max(g_tmin, c.Tmin - un);
            g_gimbal = nan_max(g_gimbal, un - us[0] * c.inv_cosd);
            if (FIN) g_fin = nan_max(g_fin, sqrt(us[3] * us[3] + us[4] * us[4]) - c.finmxf);
            g_mass = nan_max(g_mass, c.mdry - xs[0]);
            g_glide = nan_max(g_glide, c.tggs * sqrt(xs[2] * xs[2] + xs[3] * xs[3]) - xs[1]);
            g_tilt = nan_max(g_tilt, sqrt(xs[9] * xs[9] + xs[10] * xs[10]) - c.sqcm);
            g_rate = nan_max(g_rate, sqrt(xs[11] * xs[11] + xs[12] * xs[12] + xs[13] * xs[13]) - c.omMax);
            if (c.dp) g_dp = nan_max(g_dp, sqrt(xs[4] * xs[4] + xs[5] * xs[5] + xs[6] * xs[6]) - c.vmax);
            qn = nan_max(qn, fabs(sqrt(xs[7] * xs[7] + xs[8] * xs[8] + xs[9] * xs[9] + xs[10] * xs[10]) - R(1.0)));
#pragma unroll
            for (int i = 0; i < 14; i++) bad = fma(xs[i], R(0.0), bad);
            if (s == nsub) break;
            // ---- one RK4 substep, as propagate_kernel takes it ----
            R xa[14], xt[14];
#pragma unroll
            for (int i = 0; i < 14; i++) {
                xa[i] = xs[i];
                xt[i] = xs[i];
            }
#pragma unroll
            for (int stg = 0; stg < 4; stg++) {
                const R lkp = (R(s) + (stg == 0 ? R(0.0) : (stg == 3 ? R(1.0) : R(0.5)))) * inv_n;
                const R lkm = R(1.0) - lkp;
                R uu[NU];
#pragma unroll
                for (int j = 0; j < NU; j++) uu[j] = fma(ukv[j], lkm, upv[j] * lkp);
                R g[14];
                rhs_only<AERO, FIN, TRQ>(p, xt, uu, g);
                const R wacc = h * ((stg == 0 || stg == 3) ? (R(1.0) / R(6.0)) : (R(1.0) / R(3.0)));
                const R wnext = h * (stg == 2 ? R(1.0) : R(0.5));
#pragma unroll
                for (int i = 0; i < 14; i++) {
                    const R dx = sig * g[i];
                    xa[i] = fma(wacc, dx, xa[i]);
                    if (stg < 3) xt[i] = fma(wnext, dx, xs[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 14; i++) xs[i] = xa[i];
        }
        // ---- the impulse of segment k: after its last sample, before node k + 1's gap, dense row and feedback ----
        if (RNG) {
            if (rg.noise) {
#pragma unroll
                for (int i = 0; i < 14; i++) xs[i] = fma(m.sw[i], etl[i][ln], xs[i]);
            }
        } else if (et) {
#pragma unroll
            for (int i = 0; i < 14; i++) xs[i] = fma(m.sw[i], et[(size_t)k * 14 + i], xs[i]);
        }
        // ---- node k + 1: the flown state against the planned one ----
        const R* xn = xb + (size_t)(k + 1) * 14;
#pragma unroll
        for (int i = 0; i < 14; i++) {
            const R d = xs[i] - xn[i];
            gap = nan_max(gap, fabs(d));
            bad = fma(d, R(0.0), bad);
        }
    }
    // xs is the flown final node, eps the error eps_K of the estimate there (no measurement at node K)
    if (PV && live) mc_path_store(pvb + (size_t)K * SCVX_PSIG_N * S, S, c.tggs, xs);
#pragma unroll
    for (int i = 0; i < 14; i++) eps[i] = epl[i][ln];
    R mr = R(0.0), mv = R(0.0), mq = R(0.0), mw = R(0.0);
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const R dr = xs[1 + i] - c.rIf[i], dv = xs[4 + i] - c.vIf[i], dw = xs[11 + i] - c.wBf[i];
        mr = fma(dr, dr, mr); mv = fma(dv, dv, mv); mw = fma(dw, dw, mw);
    }
#pragma unroll
    for (int i = 0; i < 4; i++) { const R dq = xs[7 + i] - c.qBIf[i]; mq = fma(dq, dq, mq); }
    R o[SCVX_FLIGHT_NREP];
    o[SCVX_FLIGHT_GAP] = gap + bad;
    o[SCVX_FLIGHT_MISS_R] = sqrt(mr) + bad;
    o[SCVX_FLIGHT_MISS_V] = sqrt(mv) + bad;
    o[SCVX_FLIGHT_MISS_Q] = sqrt(mq) + bad;
    o[SCVX_FLIGHT_MISS_W] = sqrt(mw) + bad;
    o[SCVX_FLIGHT_MASS_END] = xs[0];
    o[SCVX_FLIGHT_G_MASS] = g_mass + bad;
    o[SCVX_FLIGHT_G_GLIDE] = g_glide + bad;
    o[SCVX_FLIGHT_G_TILT] = g_tilt + bad;
    o[SCVX_FLIGHT_G_RATE] = g_rate + bad;
    o[SCVX_FLIGHT_G_TMAX] = g_tmax;
    o[SCVX_FLIGHT_G_TMIN] = g_tmin;
    o[SCVX_FLIGHT_G_GIMBAL] = g_gimbal;
    o[SCVX_FLIGHT_G_DP] = c.dp ? g_dp + bad : ninf;
    o[SCVX_FLIGHT_G_FIN] = g_fin;
    o[SCVX_FLIGHT_QNORM] = qn + bad;
    if (live) {
        if (flights) {
#pragma unroll
            for (int i = 0; i < SCVX_FLIGHT_NREP; i++) flights[fl * SCVX_FLIGHT_NREP + i] = o[i];
        }
        if (xland) {
#pragma unroll
            for (int i = 0; i < 14; i++) xland[fl * 14 + i] = xs[i];
        }
        if (navK) {
#pragma unroll
            for (int i = 0; i < 14; i++) navK[fl * 14 + i] = eps[i];
        }
    }
    // ---- the wavefront's partial row ----
    R* pr = part + ((size_t)b * gridDim.x + blockIdx.x) * MCN_NP;
    const bool l0 = threadIdx.x == 0;
#pragma unroll
    for (int i = 0; i < SCVX_FLIGHT_NREP; i++) {
        const R mx = wave_nan_max(live ? o[i] : ninf);
        const R sm = wave_sum(live ? o[i] : R(0.0));
        if (l0) {
            pr[MC_MAX + i] = mx;
            pr[MC_SUM + i] = sm;
        }
    }
    bool any = false;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        const bool over = live && o[SCVX_FLIGHT_G_MASS + i] > m.tol;   // a comparison with NaN is false
        any = any || over;
        const int cnt = __popcll(__ballot(over));
        if (l0) pr[MC_CNT + i] = R(cnt);
    }
    {
        const int ca = __popcll(__ballot(any));
        const int cbad = __popcll(__ballot(live && !isfinite(o[SCVX_FLIGHT_GAP])));
        const R lo = wave_sum(live ? R(n_lo) : R(0.0)), hi = wave_sum(live ? R(n_hi) : R(0.0));   // integers below 2^53: exact
        const R fm = wave_nan_max(live ? fedmax : ninf);
        if (l0) {
            pr[MC_ANY] = R(ca);
            pr[MC_BAD] = R(cbad);
            pr[MC_LO] = lo;
            pr[MC_HI] = hi;
            pr[MCN_FED] = fm;
        }
    }
    R v[28];   // [e; eps_K]; + bad (0, or NaN): a flight poisoned through its error alone has a finite e, and its plan's rows are NaN
    const R* xK = xb + (size_t)K * 14;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        v[i] = (xs[i] - xK[i]) + bad;
        v[14 + i] = eps[i] + bad;
    }
#pragma unroll
    for (int i = 0; i < 28; i++) {
        const R sm = wave_sum(live ? v[i] : R(0.0));
        if (l0) pr[(i < 14 ? MC_E : MCN_EPS - 14) + i] = sm;
    }
    int t = 0, t14 = 0;
#pragma unroll
    for (int i = 0; i < 28; i++) {
#pragma unroll
        for (int j = i; j < 28; j++) {
            const R sm = wave_sum(live ? v[i] * v[j] : R(0.0));
            if (l0) {
                pr[MCN_JJ + t] = sm;
                if (j < 14) pr[MC_EE + t14] = sm;
            }
            t++;
            if (j < 14) t14++;
        }
    }
}

// one block per plan: the partial rows of the plan combined in block order, then mc_finish_kernel's three outputs by its expressions,
// the joint mean and covariance of [e; eps_K], and the navigation report read off them
__global__ __launch_bounds__(256) void mc_nav_finish_kernel(int S, int K, int nblk, const double* __restrict__ part,
                                                            double* __restrict__ mcrep, double* __restrict__ xmean,
                                                            double* __restrict__ xcov, double* __restrict__ jmean,
                                                            double* __restrict__ jcov, double* __restrict__ mcnav) {
    __shared__ double sh[MCN_NP], jc[784];
    const int b = blockIdx.x, t = threadIdx.x;
    const double* pb = part + (size_t)b * nblk * MCN_NP;
    for (int e = t; e < MCN_NP; e += 256) {
        double a = pb[e];
        const bool mx = e < MC_SUM || e == MCN_FED;
        for (int q = 1; q < nblk; q++) {
            const double v = pb[(size_t)q * MCN_NP + e];
            a = mx ? nan_max(a, v) : a + v;
        }
        sh[e] = a;
    }
    __syncthreads();
    const double dS = double(S);
    if (t < SCVX_MC_NREP) {
        double v = 0.0;
        if (t < MC_SUM) v = sh[t];
        else if (t <= MC_ANY) v = sh[t] / dS;
        else if (t == MC_LO || t == MC_HI) v = sh[t] / (dS * double(K));
        else if (t == MC_BAD) v = sh[t];
        else if (t == SCVX_MC_S) v = dS;
        mcrep[(size_t)b * SCVX_MC_NREP + t] = v;
    }
    if (t < 14) xmean[(size_t)b * 14 + t] = sh[MC_E + t] / dS;
    if (t < 196) {
        const int i = t / 14, j = t % 14;
        const int lo = i < j ? i : j, hi = i < j ? j : i;
        const int idx = lo * 14 - (lo * (lo - 1)) / 2 + (hi - lo);
        double v = 0.0;
        if (S > 1) {
            const double mm = sh[MC_E + lo] * sh[MC_E + hi] / dS;
            v = (sh[MC_EE + idx] - mm) / (dS - 1.0);
        }
        xcov[(size_t)b * 196 + t] = v;
    }
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
                                        double* dx0, double* navfed, double* navK, hipStream_t st, const McQ* q, const McRng* rng) {
    const PathK c = path_constants(ctx->prob);
    const double dt = 1.0 / (K + 1);
    const int nblk = (S + 63) / 64;
    const size_t nrows = (size_t)B * nblk * MCN_NP;
    hipError_t e = mc_workspace(ctx, nrows + MCN_MODEL);
    if (e != hipSuccess) return e;
    double* pv = nullptr;
    if (q && (e = mc_q_buffers(ctx, B, K, S, *q, flights, pv)) != hipSuccess) return e;
    McK m{};
    m.tol = tol;
    bool noise = false;
    if ((rng ? rng->noise != 0 : eta != nullptr) && w)
        for (int i = 0; i < 14; i++) {
            m.sw[i] = std::sqrt(w[i]);
            noise = noise || w[i] > 0.0;
        }
    if (!noise) eta = nullptr;   // w all zero: the undisturbed kernel path, bit for bit
    const McRngK rg = rng ? mc_rng_k(*rng, noise) : McRngK{};
    McNavK nv{};
    for (int i = 0; i < mm; i++) nv.srm[i] = std::sqrt(rm[i]);
    for (int i = 0; i < mm * 14; i++) nv.H[i] = H[i];
    const dim3 g((unsigned)nblk, (unsigned)B), blk(64);
    double* part = ctx->mc_ws;
    double* hm = ctx->mc_ws + nrows;
    hipLaunchKernelGGL(mc_nav_model_kernel, dim3(1), dim3(256), 0, st, nv, hm);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    const DynP<double> dp(ctx->dyn);
#define SCVX_MCN_RG(A, F, T, P, G, par)                                                                                                          \
    hipLaunchKernelGGL((mc_nav_fly_kernel<A, F, T, DS, P, G>), g, blk, 0, st, par, c, m, mm, hm, S, K, x, u, sigma, gain, C0, xi0, eta, deriv, kf, \
                       CN, xin, nud, dt, nsub, flags, part, flights, xland, dx0, navfed, navK, pv, rg)
#define SCVX_MCN_PV(A, F, T, P, par)                 \
    do {                                             \
        if (rng) SCVX_MCN_RG(A, F, T, P, true, par); \
        else SCVX_MCN_RG(A, F, T, P, false, par);    \
    } while (0)
#define SCVX_MCN(A, F, T, par)                  \
    do {                                        \
        if (pv) SCVX_MCN_PV(A, F, T, true, par); \
        else SCVX_MCN_PV(A, F, T, false, par);  \
    } while (0)
    if (ctx->dyn.trq) {
        const DynPT<double> dpt(ctx->dyn);
        if (ctx->dyn.fin) SCVX_MCN(true, true, true, dpt);
        else SCVX_MCN(true, false, true, dpt);
    } else if (ctx->dyn.fin) {
        if (ctx->dyn.aero) SCVX_MCN(true, true, false, dp);
        else SCVX_MCN(false, true, false, dp);
    } else if (ctx->dyn.aero)
        SCVX_MCN(true, false, false, dp);
    else
        SCVX_MCN(false, false, false, dp);
#undef SCVX_MCN
#undef SCVX_MCN_PV
#undef SCVX_MCN_RG
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(mc_nav_finish_kernel, dim3((unsigned)B), dim3(256), 0, st, S, K, nblk, part, mcrep, xmean, xcov, jmean, jcov, mcnav);
    e = hipGetLastError();
    if (e != hipSuccess || !q) return e;
    return mc_q_finish(B, K, S, *q, flights, pv, st);
}

hipError_t launch_track_mc_nav(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w,
                               const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                               const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                               double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                               double* navfed, double* navK, hipStream_t st, const McQ* q, const McRng* rng) {
    return launch_track_mc_nav_t<double>(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags,
                                         tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, st, q, rng);
}

hipError_t launch_track_mc_nav_f32(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                                   const double* gain, const double* C0, const double* xi0, const double* eta, const double* w,
                                   const float* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                                   const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                                   double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                                   double* navfed, double* navK, hipStream_t st, const McQ* q, const McRng* rng) {
    return launch_track_mc_nav_t<float>(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags,
                                        tol, mcrep, xmean, xcov, jmean, jcov, mcnav, flights, xland, dx0, navfed, navK, st, q, rng);
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
                              const McRng* rg) {
    int rc = scvx::check_track_mc_nav(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev, kf_dev,
                                      CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev, jmean_dev,
                                      jcov_dev, mcnav_dev);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq_dev, pathq_dev))) return rc;
    if (rg) xi0_dev = eta_dev = xin_dev = nud_dev = nullptr;   // placeholders until here: the lanes make the draws
    scvx::McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = flightq_dev, q.pathq = pathq_dev, q.pathv = pathv_dev;
    const bool any = flightq_dev || pathq_dev || pathv_dev;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_mc_nav(ctx, B, K, S, x_dev, u_dev, sigma_dev, gain_dev, C0_dev, xi0_dev, eta_dev, w14, deriv_dev,
                                            kf_dev, CN_dev, xin_dev, nud_dev, m, H, rm, nsub, flags, tol, mcrep_dev, xmean_dev, xcov_dev,
                                            jmean_dev, jcov_dev, mcnav_dev, flights_dev, xland_dev, dx0_dev, navfed_dev, navK_dev,
                                            ctx->stream, any ? &q : nullptr, rg));
    return SCVX_OK;
}

static int track_mc_nav_q_host(scvx_ctx* ctx, int B, int K, int S, const double* x, const double* u, const double* sigma,
                               const double* gain, const double* C0, const double* xi0, const double* eta, const double* w14,
                               const double* deriv, const double* kf, const double* CN, const double* xin, const double* nud, int m,
                               const double* H, const double* rm, int nsub, int flags, double tol, double* mcrep, double* xmean,
                               double* xcov, double* jmean, double* jcov, double* mcnav, double* flights, double* xland, double* dx0,
                               double* navfed, double* navK, int nq, const int* ranks, double* flightq, double* pathq, double* pathv,
                               const McRng* rg);

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
                               const McRng* rg) {
    int rc = scvx::check_track_mc_nav(ctx, B, K, S, x, u, sigma, gain, C0, xi0, eta, w14, deriv, kf, CN, xin, nud, m, H, rm, nsub, flags,
                                      tol, mcrep, xmean, xcov, jmean, jcov, mcnav);
    if (rc) return rc;
    if (rg && (rc = scvx::check_mc_rng(ctx, rg->r))) return rc;
    if (rg) xi0 = eta = xin = nud = nullptr;   // placeholders until here: the lanes make the draws
    if ((rc = scvx::check_mc_q(ctx, S, nq, ranks, flightq, pathq))) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    scvx::DevBuf<double> dfq, dpq, dpv;
    const size_t nfq = (size_t)B * SCVX_FLIGHT_NREP * nq, npq = (size_t)B * (K + 1) * SCVX_PSIG_N * nq,
                 npv = (size_t)B * (K + 1) * SCVX_PSIG_N * S;
    const int NU = scvx_control_dim(ctx), n = 14 + NU;
    const size_t nx = (size_t)B * (K + 1) * 14, nu = (size_t)B * (K + 1) * NU, ng = (size_t)B * K * NU * n, nc = (size_t)B * 196,
                 ni = (size_t)S * 14, ne = (size_t)S * K * 14, nr = (size_t)B * SCVX_MC_NREP, nm = (size_t)B * 14,
                 nf = (size_t)B * S * SCVX_FLIGHT_NREP, nl = (size_t)B * S * 14, nd = (size_t)B * K * 14 * (14 + 2 * NU + 1),
                 nk = (size_t)B * K * 14 * m, nn = (size_t)S * K * m, nj = (size_t)B * 28, njc = (size_t)B * 784,
                 nv = (size_t)B * SCVX_NAV_NREP, nfed = (size_t)B * S * K * 14;
    scvx::DevBuf<double> dx, du, ds, dg, dc, di, de, dd, dk, dcn, dxi, dnu, dr, dm, dv, djm, djc, dnv, df, dl, d0, dfe, dnk;
    const struct { scvx::DevBuf<double>* b; const double* h; size_t n; bool want; } in[] = {
        {&dx, x, nx, true},   {&du, u, nu, true},       {&ds, sigma, (size_t)B, true}, {&dg, gain, ng, true}, {&dc, C0, nc, true},
        {&di, xi0, ni, xi0 != nullptr}, {&de, eta, ne, eta != nullptr}, {&dd, deriv, nd, true},  {&dk, kf, nk, m > 0},  {&dcn, CN, nc, true},
        {&dxi, xin, ni, xin != nullptr}, {&dnu, nud, nn, m > 0 && nud != nullptr}};
    const struct { scvx::DevBuf<double>* b; double* h; size_t n; bool want; } out[] = {
        {&dr, mcrep, nr, true},  {&dm, xmean, nm, true},  {&dv, xcov, nc, true},  {&djm, jmean, nj, true},
        {&djc, jcov, njc, true}, {&dnv, mcnav, nv, true}, {&df, flights, nf, flights != nullptr}, {&dl, xland, nl, xland != nullptr},
        {&d0, dx0, nl, dx0 != nullptr}, {&dfe, navfed, nfed, navfed != nullptr}, {&dnk, navK, nl, navK != nullptr},
        {&dfq, flightq, nfq, flightq != nullptr}, {&dpq, pathq, npq, pathq != nullptr}, {&dpv, pathv, npv, pathv != nullptr}};
    hipStream_t st = ctx->stream;
    for (const auto& a : in)
        if (a.want) {
            SCVX_HIP(ctx, hipMalloc((void**)&a.b->p, a.n * 8));
            SCVX_HIP(ctx, hipMemcpyAsync(a.b->p, a.h, a.n * 8, hipMemcpyHostToDevice, st));
        }
    for (const auto& a : out)
        if (a.want) SCVX_HIP(ctx, hipMalloc((void**)&a.b->p, a.n * 8));
    scvx::McQ q;
    q.nq = nq, q.ranks = ranks, q.flightq = dfq.p, q.pathq = dpq.p, q.pathv = dpv.p;
    hipError_t e = scvx::launch_track_mc_nav(ctx, B, K, S, dx.p, du.p, ds.p, dg.p, dc.p, di.p, de.p, w14, dd.p, dk.p, dcn.p, dxi.p, dnu.p, m,
                                             H, rm, nsub, flags, tol, dr.p, dm.p, dv.p, djm.p, djc.p, dnv.p, df.p, dl.p, d0.p, dfe.p,
                                             dnk.p, st, (flightq || pathq || pathv) ? &q : nullptr, rg);
    for (const auto& a : out)
        if (e == hipSuccess && a.want) e = hipMemcpyAsync(a.h, a.b->p, a.n * 8, hipMemcpyDeviceToHost, st);
    hipError_t e2 = hipStreamSynchronize(st);   // also on an error: the buffers are freed behind whatever was enqueued
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return scvx::fail(ctx, SCVX_ERR_HIP, std::string("scvx_track_mc_nav_q_f64_host: ") + hipGetErrorString(e));
    return SCVX_OK;
}

}  // namespace scvx
