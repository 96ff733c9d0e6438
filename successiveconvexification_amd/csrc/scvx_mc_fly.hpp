// The flying kernel of the sampled closed-loop dispersion, its launch and the front of its finish: ONE body for the flight on the true
// state (scvx_mc.hip instantiates it with NAV = false) and for the flight on a navigation estimate (scvx_mc_nav.hip: NAV = true), and
// for both with per-flight vehicle errors (ACT = true: scvx_mc_veh.hip and scvx_mc_nav_veh.hip).  Not part of the ABI.
//
// mc_fly_kernel: ONE LANE PER FLIGHT (plan b, sample s); the 64 lanes of a wavefront are 64 consecutive samples of the SAME plan, blocks
// of one wavefront, grid (ceil(S / 64), B).  Every read of the plan -- x, u, sigma, the gains -- is then one address for the whole
// wavefront (blockIdx.y and the loop counters only), which the compiler serves with scalar loads; only the draws are per lane.
// scvx_track_fly_f64 spends its batch dimension on samples instead: every lane reads its own copy of the same 20 KB of gains.
//
// The flight arithmetic is fly_kernel<.., TRACK = true>'s (scvx_flight.hip), statement for statement: the feedback's fma order, the
// clamp, the first-order hold, the RK4 substep, the samples at s = 0..nsub, nan_max and the `bad` poison; without noise a flight's 16
// columns are bitwise scvx_track_fly_f64's for the same plan and the same dx0 (tests/test_gpu_mc.py).  The substep and the sampling
// block stay in the body: lifted into a __device__ function they take other registers and another fma contraction
// (profiles/fly_kernel_merge.md).
//
// NAV: the law is fed x_fly - eps+_k, the error eps of the estimate generated per flight from the filter gains of the navigation
// analysis.  Every statement of it is under `if constexpr (NAV)`; an instantiation without it has no LDS and no barrier and compiles to
// what a kernel without those statements compiles to, and with eps = 0 the two are bitwise the same flight (tests/test_gpu_mc_nav.py).
// The argument list and the order of the declarations at the top are the ones the NAV instantiations had when they were a kernel of
// their own: a trailing pack for the estimate's arguments, or the pointer set-up in another order, changes their SGPR spills and
// address arithmetic (profiles/mc_kernel_merge.md).  A_k (196 doubles), Kf_k (14 m) and H (14 m) read element by element through
// scalar loads cost about 36 cycles per element on the MI355X, so the wave fetches A_k and Kf_k with one coalesced load per 64 elements
// -- node k + 1's while segment k is integrated -- and parks them in LDS, where every lane reads them at one address (a broadcast); H and
// sqrt(rm) come from the context's workspace into LDS once.  eps [14] is in registers at the node: the innovation H eps + sqrt(rm) nud
// (m values, formed before eps is touched), eps+ = eps - Kf innovation, the feedback on (x_fly - eps+) - xbar, and eps_{k+1} = A_k eps+
// (+ sqrt(w) eta_k) BEFORE the segment's RK4 loop; while the segment is integrated eps rests in LDS as well (a column per lane; 12 KB of
// LDS per block in all).  A non-finite eps poisons its flight through `bad`, whichever node it appears at.
//
// Reduction, deterministic and without floating-point atomics: the wavefront reduces every statistic over its lanes with a fixed
// xor butterfly (32, 16, .., 1; lanes past S carry the neutral element) and lane 0 writes one partial row per block into the context's
// workspace ([MC_NP], with NAV [MCN_NP]); the finish kernels (one block per plan) combine the ceil(S / 64) partial rows of their plan in
// block order through mc_finish_front.  A lane past S flies sample S - 1 again, so that all 64 lanes reach the barriers and the
// butterfly, and contributes nothing; there is no early return.  With NAV the 14 x 14 corner of the joint triangle is written to MC_EE
// as well and every landing statistic is formed by one expression, so xcov is bitwise jcov[:, :14, :14].
//
// PV: every live lane also stores the five path functions of psig at every node into pathv [B][K+1][5][S] -- the sample is the fastest
// index, so a wavefront's 64 samples store one contiguous line per value and each (b, k, f) row is contiguous for the order-statistics
// kernel (scvx_quantile.hip): of the TRUTH xs (the constraints bind the vehicle), the thrust norm of the command as the law formed it.
//
// RNG: the loads of the draws become calls of mc_draw_group (scvx_rng.hpp) -- every lane makes its own from Philox4x64-10, the four
// blocks of a group formed at the node and dead after it; everything else is statement for statement, so a flight is bitwise the flight
// of the RNG-off kernel fed the draws mc_draws_kernel dumps (tests/test_gpu_mc_rng.py).  With NAV eta_k is formed once, at the error's
// time step, and rests in LDS (a column per lane, 7 KB per block) until the truth's impulse behind the segment; of nud_k only the blocks
// that hold its first m draws are formed.
//
// ACT: per-flight vehicle errors theta = fma(sp, zeta, mu) (include/scvx.h "vehicle errors"), six per lane in registers, formed before
// the start -- from zeta [S][6], or with RNG from the first six normals of group 0 of stream 8.  Every statement of it is under
// `if constexpr (ACT)`, and its kernel argument (McVehK) is a trailing pack that is empty without it: an instantiation without ACT has
// the argument block and the body it had.  The error lies BEHIND the command: the law, the clamp, the counters, the samples of the
// thrust band and pathv see the commanded hold uu; only the control handed to rhs_only at the four RK stages is the applied one,
//     ua[0:3] = (1 + th0) (uu[0:3] + d x uu[0:3]),  d = (0, th1, th2);      ua[3:5] = (1 + th5) uu[3:5]
// and rhs_only reads alpha (1 + th3), force_scalar (1 + th4) and trq_scalar (1 + th4) from a per-lane copy of the parameter block,
// of which only these three fields leave the scalar registers.  With NAV the recursion of eps is untouched.  The ACT instantiations
// live in translation units of their own (scvx_mc_veh.hip, scvx_mc_nav_veh.hip), compiled beside the others.
#pragma once
#include <cmath>
#include <limits>
#include <type_traits>
#include "scvx_mc.hpp"

namespace scvx {

// the measurement model in the workspace behind the partial rows: H [m][14], then sqrt(rm) at MCN_SRM
constexpr int MCN_SRM = 196, MCN_MODEL = 210;

// The argument list is the same with and without NAV (without it mm = 0 and hm, deriv .. nud, navfed, navK are nullptr and never read).
// DS is the tiles' storage type (double, or float with scvx_batch_set_linearization_f32: widened on load, as nav_cov_kernel does);
// without NAV only DS = double is instantiated.
template <typename T>
__device__ __forceinline__ const T& mc_first(const T& t) { return t; }
struct McNone {};

template <bool AERO, bool FIN, bool TRQ, bool PV, bool RNG, bool NAV, typename DS = double, bool ACT = false, typename... VA>
__global__ __launch_bounds__(64) void mc_fly_kernel(DynPK<double, TRQ> p, PathK c, McK m, int mm, const double* __restrict__ hm, int S, int K,
                                                    const double* __restrict__ x, const double* __restrict__ u,
                                                    const double* __restrict__ sigma, const double* __restrict__ gain,
                                                    const double* __restrict__ C0, const double* __restrict__ xi0,
                                                    const double* __restrict__ eta, const DS* __restrict__ deriv,
                                                    const double* __restrict__ kf, const double* __restrict__ CN,
                                                    const double* __restrict__ xin, const double* __restrict__ nud, double dt,
                                                    int nsub, int opt, double* __restrict__ part, double* __restrict__ flights,
                                                    double* __restrict__ xland, double* __restrict__ dx0o,
                                                    double* __restrict__ navfed, double* __restrict__ navK,
                                                    double* __restrict__ pathv, McRngK rg, VA... va) {
    static_assert(sizeof...(VA) == (ACT ? 1 : 0), "the ACT instantiations take one McVehK behind rg, the others nothing");
    typedef double R;
    // NAV only (without it none of these is referenced and none remains: LDS 0).  epl: eps rests here while the segment is integrated,
    // one column per lane, no lane reads another's; Al, Kl, Hl: A_k, Kf_k and the model (hm), written by the wave, read by every lane at
    // one address; etl (RNG): eta_k rests here between the error's time step and the truth's impulse, a column per lane
    __shared__ R epl[NAV ? 14 : 1][64];
    __shared__ R Al[NAV ? 196 : 1], Kl[NAV ? 196 : 1], Hl[NAV ? MCN_MODEL : 1];
    __shared__ R etl[(NAV && RNG) ? 14 : 1][64];
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
    const R* cnb = CN + (size_t)b * 196;   // NAV: cnb, tb, kb, xn_ and nd
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
    R xs[14], ukv[NU], upv[NU], eps[NAV ? 14 : 1];
    R th[ACT ? SCVX_VEH_N : 1];       // ACT: the vehicle errors of this flight
    // ACT: the parameter block with this flight's alpha, force_scalar and trq_scalar (without ACT: nothing)
    auto pl = [&] {
        if constexpr (ACT) return p;
        else return McNone{};
    }();
    if constexpr (ACT) {
        const McVehK& vk = mc_first(va...);
        R zv[16];
        if (RNG) {
            mc_draw_group(rg.seed, MC_STREAM_VEH, rc2, rc3, 0, SCVX_VEH_N, zv);
        } else {
#pragma unroll
            for (int i = 0; i < SCVX_VEH_N; i++) zv[i] = vk.zeta ? vk.zeta[(size_t)s_ * SCVX_VEH_N + i] : R(0.0);
        }
#pragma unroll
        for (int i = 0; i < SCVX_VEH_N; i++) {
            th[i] = fma(vk.sp[i], zv[i], vk.mu[i]);
            if (vk.theta && live) vk.theta[fl * SCVX_VEH_N + i] = th[i];
        }
        pl.alpha = p.alpha * (R(1.0) + th[SCVX_VEH_ISP]);
        if constexpr (AERO) pl.force_scalar = p.force_scalar * (R(1.0) + th[SCVX_VEH_AERO]);
        if constexpr (TRQ) pl.trq_scalar = p.trq_scalar * (R(1.0) + th[SCVX_VEH_AERO]);
    }
    // ---- the start: dx0 = C0 xi0 (and eps_0 = CN xin), summed with fma in ascending j ----
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
        if constexpr (NAV) {
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
    }
    if constexpr (NAV) {
#pragma unroll
        for (int i = 0; i < 14; i++) epl[i][ln] = eps[i];
    }
#pragma unroll
    for (int i = 0; i < 14; i++) xs[i] = xb[i] + xs[i];
#pragma unroll
    for (int j = 0; j < NU; j++) upv[j] = ub[j];
    R gap = R(0.0), bad = R(0.0);   // bad: 0 while every sampled state, node difference (and eps) is finite, else NaN
    R g_mass = ninf, g_glide = ninf, g_tilt = ninf, g_rate = ninf, g_tmax = ninf, g_tmin = ninf, g_gimbal = ninf, g_dp = ninf,
      g_fin = ninf, qn = R(0.0), fedmax = R(0.0);
    int n_lo = 0, n_hi = 0;         // commanded node controls k = 1..K outside the thrust band by more than tol, before the clamp
    DS pre[4];
    R prk[4];
    if constexpr (NAV) {
#pragma unroll
        for (int i = 0; i < 14; i++) bad = fma(eps[i], R(0.0), bad);
        // A_k and Kf_k of node 0 (a lane fetches elements ln, ln + 64, ..), and the model
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int e = ln + 64 * q;
            pre[q] = e < 196 ? tb[e] : DS(0);
            prk[q] = (mm > 0 && e < 14 * mm) ? kb[e] : R(0.0);
        }
        if (mm > 0)
            for (int e = ln; e < MCN_MODEL; e += 64) Hl[e] = hm[e];
    }
    // PV: the five path functions at every node, pathv[((b (K + 1) + k) 5 + f) S + s] -- the sample is the fastest index, a wavefront
    // stores one contiguous line per value
    R* pvb = PV ? pathv + (size_t)b * (K + 1) * SCVX_PSIG_N * S + s_ : nullptr;
    if (PV && live) pvb[(size_t)SCVX_PSIG_THRUST * S] = sqrt(upv[0] * upv[0] + upv[1] * upv[1] + upv[2] * upv[2]);
    for (int k = 0; k < K; k++) {
        if (PV && live) mc_path_store(pvb + (size_t)k * SCVX_PSIG_N * S, S, c.tggs, xs);
        if constexpr (NAV) {
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
        }
        // ---- node k: the next node's control from the flown state (NAV: from its ESTIMATE) and the applied control ----
        {
            R z[n];
#pragma unroll
            for (int i = 0; i < 14; i++) {
                if constexpr (NAV) z[i] = (xs[i] - eps[i]) - xb[(size_t)k * 14 + i];
                else z[i] = xs[i] - xb[(size_t)k * 14 + i];
            }
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
        if constexpr (NAV) {
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
                if constexpr (ACT) {
                    // the applied control: scale and first-order rotation of the thrust, scale of the fins
                    const R sc = R(1.0) + th[SCVX_VEH_THRUST];
                    R ua[NU];
                    ua[0] = sc * (uu[0] + (th[SCVX_VEH_MIS_Y] * uu[2] - th[SCVX_VEH_MIS_Z] * uu[1]));
                    ua[1] = sc * (uu[1] + th[SCVX_VEH_MIS_Z] * uu[0]);
                    ua[2] = sc * (uu[2] - th[SCVX_VEH_MIS_Y] * uu[0]);
                    if constexpr (FIN) {
                        ua[3] = (R(1.0) + th[SCVX_VEH_FIN]) * uu[3];
                        ua[4] = (R(1.0) + th[SCVX_VEH_FIN]) * uu[4];
                    }
                    rhs_only<AERO, FIN, TRQ>(pl, xt, ua, g);
                } else {
                    rhs_only<AERO, FIN, TRQ>(p, xt, uu, g);
                }
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
                if constexpr (NAV) {
#pragma unroll
                    for (int i = 0; i < 14; i++) xs[i] = fma(m.sw[i], etl[i][ln], xs[i]);
                } else {
                    R ev[16];   // group 1 + k, formed here and dead after the impulse
                    mc_draw_group(rg.seed, MC_STREAM_TRUTH, rc2, rc3, 1 + k, 14, ev);
#pragma unroll
                    for (int i = 0; i < 14; i++) xs[i] = fma(m.sw[i], ev[i], xs[i]);
                }
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
    // xs is the flown final node (NAV: eps the error eps_K of the estimate there, no measurement at node K)
    if (PV && live) mc_path_store(pvb + (size_t)K * SCVX_PSIG_N * S, S, c.tggs, xs);
    if constexpr (NAV) {
#pragma unroll
        for (int i = 0; i < 14; i++) eps[i] = epl[i][ln];
    }
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
        if constexpr (NAV) {
            if (navK) {
#pragma unroll
                for (int i = 0; i < 14; i++) navK[fl * 14 + i] = eps[i];
            }
        }
    }
    // ---- the wavefront's partial row ----
    R* pr = part + ((size_t)b * gridDim.x + blockIdx.x) * (NAV ? MCN_NP : MC_NP);
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
        R fm = R(0.0);
        if constexpr (NAV) fm = wave_nan_max(live ? fedmax : ninf);
        if (l0) {
            pr[MC_ANY] = R(ca);
            pr[MC_BAD] = R(cbad);
            pr[MC_LO] = lo;
            pr[MC_HI] = hi;
            if constexpr (NAV) pr[MCN_FED] = fm;
        }
    }
    const R* xK = xb + (size_t)K * 14;
    if constexpr (NAV) {
        R v[28];   // [e; eps_K]; + bad (0, or NaN): a flight poisoned through its error alone has a finite e, and its plan's rows are NaN
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
    } else {
        R e[14];
#pragma unroll
        for (int i = 0; i < 14; i++) {
            e[i] = xs[i] - xK[i];
            const R sm = wave_sum(live ? e[i] : R(0.0));
            if (l0) pr[MC_E + i] = sm;
        }
        int t = 0;
#pragma unroll
        for (int i = 0; i < 14; i++) {
#pragma unroll
            for (int j = i; j < 14; j++) {
                const R sm = wave_sum(live ? e[i] * e[j] : R(0.0));
                if (l0) pr[MC_EE + t] = sm;
                t++;
            }
        }
    }
}

// The front of both finish kernels (one block of 256 per plan): the partial rows [NP] of plan b combined in block order into sh, then the
// report, the mean and the covariance of the landing deviation.  Ends behind a barrier: every thread may read all of sh.
template <int NP>
__device__ __forceinline__ void mc_finish_front(int S, int K, int nblk, const double* __restrict__ part, double* sh,
                                                double* __restrict__ mcrep, double* __restrict__ xmean, double* __restrict__ xcov) {
    const int b = blockIdx.x, t = threadIdx.x;
    const double* pb = part + (size_t)b * nblk * NP;
    for (int e = t; e < NP; e += 256) {
        double a = pb[e];
        const bool mx = e < MC_SUM || (NP == MCN_NP && e == MCN_FED);
        for (int q = 1; q < nblk; q++) {
            const double v = pb[(size_t)q * NP + e];
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
}

// The noise of a sampled call: the impulse's size into m.sw (from sw itself, or with nav from the variance w), eta = nullptr when no
// component receives an impulse (the undisturbed kernel path, bit for bit), and the streams of the forms whose lanes make the draws.
inline McRngK mc_noise(McK& m, McCall& mc) {
    bool noise = false;
    if ((mc.drawn ? mc.noise != 0 : mc.eta != nullptr) && mc.w)
        for (int i = 0; i < 14; i++) {
            m.sw[i] = mc.nav ? std::sqrt(mc.w[i]) : mc.w[i];
            noise = noise || mc.w[i] > 0.0;
        }
    if (!noise) mc.eta = nullptr;
    return mc.drawn ? mc_rng_k(*mc.rng, noise) : McRngK{};
}

// What the flight on an estimate adds to the kernel's arguments, read off the record; all zero for the flight on the true state.
template <typename DS>
struct McNavA {
    int mm;              // rows of the measurement model
    const double* hm;    // the model in the workspace, behind the partial rows (mc_nav_model)
    const DS* deriv;
    const double *kf, *CN, *xin, *nud;
    double *navfed, *navK;
};
inline double* mc_nav_model(const scvx_ctx* ctx, const McCall& mc) { return ctx->mc_ws + (size_t)mc.B * ((mc.S + 63) / 64) * MCN_NP; }

// The launch of the flying kernel, for all four translation units: the instantiation of the context's model, with PV when pathv is
// asked for and RNG when the lanes make the draws.  mc: the device record as launch_mc prepared it (flights and q.pathv where the
// kernel writes them, eta behind mc_noise); the partial rows go to ctx->mc_ws.  ACT: the instantiations with vehicle errors.
template <bool NAV, typename DS, bool ACT>
hipError_t launch_mc_fly_t(scvx_ctx* ctx, const McCall& mc, const McK& m, const McRngK& rg, hipStream_t st) {
    const PathK c = path_constants(ctx->prob);
    const double dt = 1.0 / (mc.K + 1);
    const dim3 g((unsigned)((mc.S + 63) / 64), (unsigned)mc.B), blk(64);
    const DynP<double> dp(ctx->dyn);
    McNavA<DS> n{};
    if constexpr (NAV) {
        if constexpr (std::is_same<DS, double>::value) n.deriv = mc.deriv.d;
        else n.deriv = mc.deriv.f;
        n.mm = mc.m, n.hm = mc_nav_model(ctx, mc), n.kf = mc.kf, n.CN = mc.CN, n.xin = mc.xin, n.nud = mc.nud;
        n.navfed = mc.navfed, n.navK = mc.navK;
    }
#define SCVX_MC_ARGS(par)                                                                                                         \
    par, c, m, n.mm, n.hm, mc.S, mc.K, mc.x, mc.u, mc.sigma, mc.gain, mc.C0, mc.xi0, mc.eta, n.deriv, n.kf, n.CN, n.xin, n.nud, dt, \
        mc.nsub, mc.flags, ctx->mc_ws, mc.flights, mc.xland, mc.dx0, n.navfed, n.navK, mc.q.pathv, rg
#define SCVX_MC_RG(A, F, T, P, G, par)                                                                                           \
    do {                                                                                                                         \
        if constexpr (ACT)                                                                                                       \
            hipLaunchKernelGGL((mc_fly_kernel<A, F, T, P, G, NAV, DS, true, McVehK>), g, blk, 0, st, SCVX_MC_ARGS(par), mc_veh_k(mc.veh)); \
        else                                                                                                                     \
            hipLaunchKernelGGL((mc_fly_kernel<A, F, T, P, G, NAV, DS>), g, blk, 0, st, SCVX_MC_ARGS(par));                        \
    } while (0)
#define SCVX_MC_PV(A, F, T, P, par)                      \
    do {                                                 \
        if (mc.drawn) SCVX_MC_RG(A, F, T, P, true, par); \
        else SCVX_MC_RG(A, F, T, P, false, par);         \
    } while (0)
#define SCVX_MC(A, F, T, par)                           \
    do {                                                \
        if (mc.q.pathv) SCVX_MC_PV(A, F, T, true, par); \
        else SCVX_MC_PV(A, F, T, false, par);           \
    } while (0)
    if (ctx->dyn.trq) {
        const DynPT<double> dpt(ctx->dyn);
        if (ctx->dyn.fin) SCVX_MC(true, true, true, dpt);
        else SCVX_MC(true, false, true, dpt);
    } else if (ctx->dyn.fin) {
        if (ctx->dyn.aero) SCVX_MC(true, true, false, dp);
        else SCVX_MC(false, true, false, dp);
    } else if (ctx->dyn.aero)
        SCVX_MC(true, false, false, dp);
    else
        SCVX_MC(false, false, false, dp);
#undef SCVX_MC
#undef SCVX_MC_PV
#undef SCVX_MC_RG
#undef SCVX_MC_ARGS
    return hipGetLastError();
}

// The ACT instantiations of the launch are made in scvx_mc_veh.hip (NAV = false) and scvx_mc_nav_veh.hip (NAV = true, DS double and
// float) alone: these declarations keep every other translation unit from instantiating them, and with them their kernels.
#define SCVX_MC_FLY_ACT(NAV, DS) \
    hipError_t launch_mc_fly_t<NAV, DS, true>(scvx_ctx*, const McCall&, const McK&, const McRngK&, hipStream_t)
extern template SCVX_MC_FLY_ACT(false, double);
extern template SCVX_MC_FLY_ACT(true, double);
extern template SCVX_MC_FLY_ACT(true, float);

template <bool NAV, typename DS>
hipError_t launch_mc_fly(scvx_ctx* ctx, const McCall& mc, const McK& m, const McRngK& rg, hipStream_t st) {
    return mc.veh.v ? launch_mc_fly_t<NAV, DS, true>(ctx, mc, m, rg, st) : launch_mc_fly_t<NAV, DS, false>(ctx, mc, m, rg, st);
}

}  // namespace scvx
