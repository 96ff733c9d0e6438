// Navigation-error (LQG) covariance analysis (scvx_nav_cov_f64, include/scvx.h): the covariance Xi_k of the joint
// zeta_k = [z_k; eps_k], z = [dx; du] the deviation of the truth from the plan under the tracking law of scvx_track.hip and
// eps = x - xhat the error of the navigation estimate the law is fed, with a measurement update (Joseph form) and a time step per
// node, and the two per-trajectory reports read off it.  No counterpart in the reference.
//
// nav_cov_kernel: ONE WAVEFRONT PER TRAJECTORY, K sequential steps -- cov_propagate_kernel (scvx_cov.hip) on the joint.  N = n + 14.
// Neither T_k = [[M, -G Lx], [0, A]] nor U = blockdiag(I, J) is stored as a matrix:
//     update (m > 0):  HP = H P (m x 14),  S = HP H' + diag(rm),  S = C C' (left-looking, one lane per row),  Kf' = S^-1 HP (one lane
//                      per column),  J = I - Kf H,  Y = Xi[:, eps] J' (N x 14),  Xi[z, eps] = Y[z], Xi[eps, z] = Y[z]',
//                      Xi[eps, eps] = J Y[eps] + Kf diag(rm) Kf'  -- the z block is not touched
//     time step:       Mtop = [A B-] + B+ L (14 x n),  Gx = B+ Lx (14 x 14)  -- the rows 14.. of M and of G Lx are L and Lx themselves,
//                      the eps rows of T are A;  V = T Xi (N x N),  R = V T' over Xi,  Xi = (R + R') / 2 + W: every pair from both of
//                      its triangles, W = diag(w) in the xx, x eps, eps x and eps eps blocks
// with Xi, V, the tile, Mtop, Gx, L and H in LDS; S, Kf' and J live in V, which the update does not otherwise need (23.5 KB at NU = 3,
// 26.6 KB at NU = 5).  One lane per output element throughout; a row of T is one of three kinds (top, gain, eps), and the element
// maps keep the 64 lanes of a pass in at most two of them.  The tile and the gain block of step k + 1 are fetched into registers while
// step k computes and stored to LDS behind the step's last barrier.  DS is the tiles' storage type (double, or float with
// scvx_batch_set_linearization_f32: widened on load).  H, rm and w ride by value in the kernel argument and are copied to LDS once.
//
// The dispersion report is cov_propagate_kernel's, read off the z block (lanes 0..5 the running columns, 6..11 the final ones);
// lane 12 carries NAV_PEAK, lanes 13..19 the final columns of the navigation report.  With PS the s = sqrt(c' Xi_k[z,z] c) that lanes 1..5
// form at every node for their margins is kept as well (scvx_nav_path_sigma_f64): the truth block before the node's update, which
// the update does not touch -- the constraints bind the vehicle, not its estimate.
#include <cmath>
#include <limits>
#include "scvx_cov.hpp"

namespace scvx {

struct NavK {
    double mdry, tggs, sqcm, omMax, Tmax, Tmin;
    double w[14], rm[14], H[196];
    int m;
};

// square root of a variance (a rounded variance of -1e-40 is 0, a NaN stays a NaN)
__device__ __forceinline__ double nav_sd(double v) { return v > 0.0 ? sqrt(v) : (v != v ? v : 0.0); }

// c' S c for a gradient with (up to) three nonzeros c0, c1, c2 at i0, i1, i2; S with row stride n
__device__ __forceinline__ double nav_quad3(const double* S, int n, int i0, int i1, int i2, double c0, double c1, double c2) {
    const double d = c0 * c0 * S[i0 * n + i0] + c1 * c1 * S[i1 * n + i1] + c2 * c2 * S[i2 * n + i2];
    const double o = c0 * c1 * S[i0 * n + i1] + c0 * c2 * S[i0 * n + i2] + c1 * c2 * S[i1 * n + i2];
    return d + 2.0 * o;
}

// PS: 1 = also keep the per-node s of the five path functions (psig [B][K+1][SCVX_PSIG_N], lane - 1 is the column: SCVX_PSIG_MASS, GLIDE,
// TILT, RATE, THRUST); 0 = the reports alone, and nothing of it is compiled in
// VEH: 1 = vehicle errors as consider parameters (scvx_nav_cov_vehicle_f64; cov_propagate_kernel's VEH on the joint).  J_k = d z_k / d
// theta (n x 6: the eps rows are zero, the recursion of eps does not see theta) alternates between two LDS buffers, J_{k+1} = [Mtop; L]
// J_k + [Gamma_k; 0], updated in the V pass.  The outputs read Xi_k with J_k diag(sp^2) J_k' added to its [z, z] block, formed in V
// behind the step's last barrier; V is the update's scratch too, so the next step starts behind one more barrier.  Xi_k itself, and
// with it the eps blocks, kf and the navigation report, are the plain call's.  All of it under `if constexpr (VEH)`, the kernel
// argument a trailing pack that is empty without it.
template <typename DS, int NU, int PS = 0, int VEH = 0, typename... VA>
__global__ __launch_bounds__(64) void nav_cov_kernel(NavK c, int B, int K, const double* __restrict__ x, const double* __restrict__ u,
                                                     const DS* __restrict__ deriv, const double* __restrict__ gain,
                                                     const double* __restrict__ S0, const double* __restrict__ N0,
                                                     double* __restrict__ report, double* __restrict__ navrep, double* __restrict__ sig,
                                                     double* __restrict__ navsig, double* __restrict__ kf, double* __restrict__ joint,
                                                     double* __restrict__ psig, VA... va) {
    static_assert(sizeof...(VA) == (VEH ? 1 : 0), "the VEH instantiations take one CovVehK behind psig, the others nothing");
    constexpr int NJ = (14 + NU) * SCVX_VEH_N;
    constexpr int n = 14 + NU, N = n + 14, mt = 14 + 2 * NU, NC = mt + 1, DSZ = 14 * NC, ND = 14 * mt, NL = NU * n, NN = N * N;
    constexpr int NPRE = (ND + 63) / 64, NLPRE = (NL + 63) / 64;
    constexpr int NR = SCVX_COV_NREP + SCVX_NAV_NREP;
    static_assert(N * 14 + 2 * 196 <= NN && 196 <= N * 14, "Y (S before it), J and Kf' must fit into V");
    __shared__ double Xl[NN], Vl[NN], Dl[ND], Ml[14 * n], Gl[196], Ll[NL], Hl[196], rml[14], tl[14], Rl[NR + 2];
    // Kl: HP, then Kf' (m x 14);  Sl: S, then its factor C, dead before Y is born in its place
    double *Yl = Vl, *Sl = Vl, *Jl = Vl + N * 14, *Kl = Jl + 196;
    __shared__ double Tl[VEH ? 2 * NJ : 1], Gml[VEH ? 14 * SCVX_VEH_N : 1];   // VEH: d z / d theta at nodes k and k + 1; Gamma_k, column-major
    const double* const Xo = VEH ? Vl : Xl;   // what the outputs read: Xi_k, with VEH its [z, z] block + J_k diag(sp^2) J_k'
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const int m = c.m;
    const DS* tiles = deriv + (size_t)b * K * DSZ;
    const double* gb = gain + (size_t)b * K * NL;
    const double* xb = x + (size_t)b * (K + 1) * 14;
    const double* ub = u + (size_t)b * (K + 1) * NU;
    const double* s0 = S0 + (size_t)b * 196;
    const double* n0 = N0 + (size_t)b * 196;
    double* jb = joint ? joint + (size_t)b * (K + 1) * NN : nullptr;
    double* sigb = sig ? sig + (size_t)b * (K + 1) * n : nullptr;
    double* nsb = navsig ? navsig + (size_t)b * (K + 1) * 14 : nullptr;
    double* kfb = kf ? kf + (size_t)b * K * 14 * m : nullptr;
    double* psb = PS ? psig + (size_t)b * (K + 1) * SCVX_PSIG_N : nullptr;
    const double inf = std::numeric_limits<double>::infinity();
    // Xi_0 = blockdiag((S0 + S0') / 2, 0, (N0 + N0') / 2); tile 0 and gain block 0; H and rm
    for (int e = lane; e < NN; e += 64) {
        const int a = e / N, cc = e % N;
        double v = 0.0;
        if (a < 14 && cc < 14) v = 0.5 * (s0[a * 14 + cc] + s0[cc * 14 + a]);
        else if (a >= n && cc >= n) v = 0.5 * (n0[(a - n) * 14 + cc - n] + n0[(cc - n) * 14 + a - n]);
        Xl[e] = v;
    }
    for (int e = lane; e < ND; e += 64) Dl[e] = (double)tiles[e];
    for (int e = lane; e < NL; e += 64) Ll[e] = gb[e];
    for (int e = lane; e < m * 14; e += 64) Hl[e] = c.H[e];
    if (lane < 14) rml[lane] = c.rm[lane];
    if constexpr (VEH)
        for (int e = lane; e < NJ; e += 64) Tl[e] = 0.0;
    // the running columns: lane 0 SIG_PEAK (and its non-finite flag), 1 N_MASS, 2 N_GLIDE, 3 N_TILT, 4 N_RATE, 5 S_THRUST / N_TMAX /
    // N_TMIN, 12 NAV_PEAK (and its non-finite flag)
    double acc0 = (lane == 0 || lane == 12) ? 0.0 : inf, acc1 = inf, acc2 = 0.0, bad = 0.0;
    double pv0 = 0.0, pv1 = 0.0, pv2 = 0.0;
    __syncthreads();
    // sum_l T[a][l] col(l): row a of T is [Mtop | -Gx] (a < 14), [L | -Lx] (a < n) or [0 | A] (the eps rows)
    auto tdot = [&](int a, auto col) {
        double s = 0.0;
        if (a < 14) {
#pragma unroll
            for (int l = 0; l < n; l++) s = fma(Ml[l * 14 + a], col(l), s);
#pragma unroll
            for (int j = 0; j < 14; j++) s = fma(-Gl[j * 14 + a], col(n + j), s);
        } else if (a < n) {
            const double* lr = Ll + (a - 14) * n;
#pragma unroll
            for (int l = 0; l < n; l++) s = fma(lr[l], col(l), s);
#pragma unroll
            for (int j = 0; j < 14; j++) s = fma(-lr[j], col(n + j), s);
        } else {
#pragma unroll
            for (int j = 0; j < 14; j++) s = fma(Dl[j * 14 + a - n], col(n + j), s);
        }
        return s;
    };
    // dense outputs and the running columns at node k (the pre-update Xi_k in Xl; pv*: the plan values of node k this lane reads)
    auto node_out = [&](int k) {
        if (jb)
            for (int e = lane; e < NN; e += 64) jb[(size_t)k * NN + e] = Xo[e];
        if (sigb && lane < n) sigb[(size_t)k * n + lane] = nav_sd(Xo[lane * N + lane]);
        if (nsb && lane >= 32 && lane < 46) nsb[(size_t)k * 14 + lane - 32] = nav_sd(Xo[(n + lane - 32) * N + n + lane - 32]);
        if (lane == 0 || lane == 12) {
            const int o = lane == 0 ? 0 : n;
            double tr = 0.0;
#pragma unroll
            for (int i = 0; i < 14; i++) tr += Xo[(o + i) * N + o + i];
            bad = fma(tr, 0.0, bad);
            acc0 = nan_max(acc0, nav_sd(tr));
        } else if (k > 0 && lane < 6) {
            [[maybe_unused]] double sv = 0.0;   // PS: this lane's s at node k (0 where the margin skips the node: an undefined gradient)
            if (lane == 1) {
                const double s = nav_sd(Xo[0]);
                if constexpr (PS != 0) sv = s;
                if (!(s == 0.0)) acc0 = nan_min(acc0, -(c.mdry - pv0) / s);
            } else if (lane == 5) {
                const double nr = sqrt(pv0 * pv0 + pv1 * pv1 + pv2 * pv2);
                if (!(nr == 0.0)) {
                    const double s = nav_sd(nav_quad3(Xo, N, 14, 15, 16, pv0 / nr, pv1 / nr, pv2 / nr));
                    acc2 = nan_max(acc2, s);
                    if constexpr (PS != 0) sv = s;
                    if (!(s == 0.0)) {
                        acc0 = nan_min(acc0, -(nr - c.Tmax) / s);
                        acc1 = nan_min(acc1, -(c.Tmin - nr) / s);
                    }
                }
            } else {
                // 2 glide: g = tggs |r[2:3]| - r[1];  3 tilt: g = |q[3:4]| - sqcm;  4 rate: g = |w| - omMax
                const double a0 = lane == 2 ? pv1 : pv0, a1 = lane == 2 ? pv2 : pv1, a2 = lane == 4 ? pv2 : 0.0;
                const double nr = sqrt(a0 * a0 + a1 * a1 + a2 * a2);
                if (!(nr == 0.0)) {
                    double g, q;
                    if (lane == 2) {
                        g = c.tggs * nr - pv0;
                        q = nav_quad3(Xo, N, 1, 2, 3, -1.0, c.tggs * a0 / nr, c.tggs * a1 / nr);
                    } else if (lane == 3) {
                        g = nr - c.sqcm;
                        q = nav_quad3(Xo, N, 9, 10, 10, a0 / nr, a1 / nr, 0.0);
                    } else {
                        g = nr - c.omMax;
                        q = nav_quad3(Xo, N, 11, 12, 13, a0 / nr, a1 / nr, a2 / nr);
                    }
                    const double s = nav_sd(q);
                    if constexpr (PS != 0) sv = s;
                    if (!(s == 0.0)) acc0 = nan_min(acc0, -g / s);
                }
            }
            if constexpr (PS != 0) psb[(size_t)k * SCVX_PSIG_N + (lane - 1)] = sv;
        }
        if constexpr (PS != 0)
            if (k == 0 && lane >= 1 && lane < 6) psb[lane - 1] = 0.0;   // node 0: no margin reads it
    };
    // VEH: Xi_k with J_k diag(sp^2) J_k' on its [z, z] block into V, J_k (in the buffer k & 1) out as sens
    auto tot = [&](int k) {
        if constexpr (VEH) {
            const CovVehK& vk = veh_first(va...);
            const double* Jc = Tl + (k & 1) * NJ;
            for (int e = lane; e < NN; e += 64) {
                const int a = e / N, cc = e % N;
                double t = 0.0;
                if (a < n && cc < n) {
#pragma unroll
                    for (int j = 0; j < SCVX_VEH_N; j++) t = fma(Jc[a * SCVX_VEH_N + j] * Jc[cc * SCVX_VEH_N + j], vk.p[j], t);
                }
                Vl[e] = t == 0.0 ? Xl[e] : Xl[e] + t;
            }
            if (vk.sens)
                for (int e = lane; e < NJ; e += 64) vk.sens[((size_t)b * (K + 1) + k) * NJ + e] = Jc[e];
            __syncthreads();
        }
    };
    tot(0);
    node_out(0);
    for (int k = 0; k < K; k++) {
        // the next step's tile and gain block, and the plan values of node k + 1, in flight while this step computes
        DS pre[NPRE];
        double prel[NLPRE];
        if (k + 1 < K) {
            const DS* t = tiles + (size_t)(k + 1) * DSZ;
            const double* g = gb + (size_t)(k + 1) * NL;
#pragma unroll
            for (int i = 0; i < NPRE; i++) {
                const int e = lane + 64 * i;
                pre[i] = e < ND ? t[e] : DS(0);
            }
#pragma unroll
            for (int i = 0; i < NLPRE; i++) {
                const int e = lane + 64 * i;
                prel[i] = e < NL ? g[e] : 0.0;
            }
        }
        if (lane >= 1 && lane < 6) {
            const double* xn = xb + (size_t)(k + 1) * 14;
            const double* un = ub + (size_t)(k + 1) * NU;
            const double* p = lane == 1 ? xn : lane == 2 ? xn + 1 : lane == 3 ? xn + 9 : lane == 4 ? xn + 11 : un;
            pv0 = p[0];
            pv1 = lane == 1 ? 0.0 : p[1];
            pv2 = (lane == 1 || lane == 3) ? 0.0 : p[2];
        }
        if constexpr (VEH) {
            // Gamma_k's columns (include/scvx.h)
            const CovVehK& vk = veh_first(va...);
            const double* vt = vk.vtile ? vk.vtile + ((size_t)b * K + k) * SCVX_VTILE_N * 14 : nullptr;
            for (int e = lane; e < 14 * SCVX_VEH_N; e += 64) Gml[e] = veh_gamma<NU>(Dl, ub + (size_t)k * NU, vt, e % 14, e / 14);
            __syncthreads();   // node_out's reads of V are done: the update may use it
        }
        // Mtop = [A B-] + B+ L and Gx = B+ Lx (read by the time step; written here, behind the previous step's last barrier)
        for (int e = lane; e < 14 * n + 196; e += 64) {
            const bool top = e < 14 * n;
            const int f = top ? e : e - 14 * n, i = f % 14, cc = f / 14;
            double s = top ? Dl[f] : 0.0;
#pragma unroll
            for (int j = 0; j < NU; j++) s = fma(Dl[(n + j) * 14 + i], Ll[j * n + cc], s);
            (top ? Ml : Gl)[f] = s;
        }
        if (m > 0) {
            // ---- measurement update at node k, P = Xi[eps, eps] ----
            // HP = H P (P symmetric: row c read for column c)
            for (int e = lane; e < m * 14; e += 64) {
                const int i = e / 14, cc = e % 14;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 14; l++) s = fma(Hl[i * 14 + l], Xl[(n + cc) * N + n + l], s);
                Kl[e] = s;
            }
            __syncthreads();
            // S = HP H' + diag(rm)
            for (int e = lane; e < m * m; e += 64) {
                const int i = e / m, j = e % m;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 14; l++) s = fma(Kl[i * 14 + l], Hl[j * 14 + l], s);
                Sl[e] = i == j ? s + rml[i] : s;
            }
            __syncthreads();
            // S = C C', left-looking: lane i owns row i; column j needs the finished columns < j of rows i and j
            for (int j = 0; j < m; j++) {
                double s = 0.0;
                if (lane >= j && lane < m) {
                    s = Sl[lane * m + j];
                    for (int l = 0; l < j; l++) s = fma(-Sl[lane * m + l], Sl[j * m + l], s);
                    tl[lane] = s;
                }
                __syncthreads();
                if (lane >= j && lane < m) {
                    const double d = sqrt(tl[j]);
                    Sl[lane * m + j] = lane == j ? d : s / d;
                }
                __syncthreads();
            }
            // Kf' = S^-1 HP: lane cc solves column cc in place (forward, then backward)
            if (lane < 14) {
                for (int i = 0; i < m; i++) {
                    double s = Kl[i * 14 + lane];
                    for (int l = 0; l < i; l++) s = fma(-Sl[i * m + l], Kl[l * 14 + lane], s);
                    Kl[i * 14 + lane] = s / Sl[i * m + i];
                }
                for (int i = m - 1; i >= 0; i--) {
                    double s = Kl[i * 14 + lane];
                    for (int l = i + 1; l < m; l++) s = fma(-Sl[l * m + i], Kl[l * 14 + lane], s);
                    Kl[i * 14 + lane] = s / Sl[i * m + i];
                }
            }
            __syncthreads();
            // J = I - Kf H; the gain leaves as kf[k][14][m]
            for (int e = lane; e < 196; e += 64) {
                const int a = e / 14, cc = e % 14;
                double s = 0.0;
                for (int i = 0; i < m; i++) s = fma(Kl[i * 14 + a], Hl[i * 14 + cc], s);
                Jl[e] = (a == cc ? 1.0 : 0.0) - s;
            }
            if (kfb)
                for (int e = lane; e < 14 * m; e += 64) kfb[(size_t)k * 14 * m + e] = Kl[(e % m) * 14 + e / m];
            __syncthreads();
            // Y = Xi[:, eps] J' (S is dead: Y may take its place)
            for (int e = lane; e < N * 14; e += 64) {
                const int a = e / 14, cc = e % 14;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 14; l++) s = fma(Xl[a * N + n + l], Jl[cc * 14 + l], s);
                Yl[e] = s;
            }
            __syncthreads();
            // Xi[z, eps] = Y[z] and its transpose;  Xi[eps, eps] = J Y[eps] + Kf diag(rm) Kf'
            for (int e = lane; e < N * 14; e += 64) {
                const int a = e / 14, cc = e % 14;
                if (a < n) {
                    Xl[a * N + n + cc] = Yl[e];
                    Xl[(n + cc) * N + a] = Yl[e];
                } else {
                    double s = 0.0;
#pragma unroll
                    for (int l = 0; l < 14; l++) s = fma(Jl[(a - n) * 14 + l], Yl[(n + l) * 14 + cc], s);
                    for (int i = 0; i < m; i++) s = fma(Kl[i * 14 + a - n] * rml[i], Kl[i * 14 + cc], s);
                    Xl[a * N + n + cc] = s;
                }
            }
            __syncthreads();
            // the eps block symmetrised: every pair from both of its triangles
            for (int e = lane; e < 196; e += 64) {
                const int a = e / 14, cc = e % 14;
                if (a < cc) {
                    const double s = 0.5 * (Xl[(n + a) * N + n + cc] + Xl[(n + cc) * N + n + a]);
                    Xl[(n + a) * N + n + cc] = s;
                    Xl[(n + cc) * N + n + a] = s;
                }
            }
        }
        __syncthreads();
        // ---- time step ----
        // V = T Xi+ (Xi+ symmetric, read by rows): lanes run along a row of V, so a pass meets at most three rows of T
        for (int e = lane; e < NN; e += 64) {
            const int a = e / N, cc = e % N;
            Vl[e] = tdot(a, [&](int l) { return Xl[cc * N + l]; });
        }
        if constexpr (VEH) {
            // J_{k+1} = [Mtop; L] J_k + [Gamma_k; 0] into the other buffer
            const double* Jc = Tl + (k & 1) * NJ;
            double* Jn = Tl + ((k + 1) & 1) * NJ;
            for (int e = lane; e < NJ; e += 64) {
                const int a = e / SCVX_VEH_N, cI = e % SCVX_VEH_N;
                double s = a < 14 ? Gml[cI * 14 + a] : 0.0;
#pragma unroll
                for (int l = 0; l < n; l++) s = fma(a < 14 ? Ml[l * 14 + a] : Ll[(a - 14) * n + l], Jc[l * SCVX_VEH_N + cI], s);
                Jn[e] = s;
            }
        }
        __syncthreads();
        // R = V T', over Xi (no longer read): lanes run down a column of R
        for (int e = lane; e < NN; e += 64) {
            const int cc = e / N, a = e % N;
            Xl[a * N + cc] = tdot(cc, [&](int l) { return Vl[a * N + l]; });
        }
        __syncthreads();
        // Xi_{k+1} = (R + R') / 2 + W: one lane per pair, both triangles written with the same value
        for (int e = lane; e < NN; e += 64) {
            const int a = e / N, cc = e % N;
            if (a < cc) {
                double s = 0.5 * (Xl[a * N + cc] + Xl[cc * N + a]);
                if (a < 14 && cc == a + n) s += c.w[a];
                Xl[a * N + cc] = s;
                Xl[cc * N + a] = s;
            } else if (a == cc) {
                if (a < 14) Xl[e] += c.w[a];
                else if (a >= n) Xl[e] += c.w[a - n];
            }
        }
        if (k + 1 < K) {
#pragma unroll
            for (int i = 0; i < NPRE; i++) {
                const int e = lane + 64 * i;
                if (e < ND) Dl[e] = (double)pre[i];
            }
#pragma unroll
            for (int i = 0; i < NLPRE; i++) {
                const int e = lane + 64 * i;
                if (e < NL) Ll[e] = prel[i];
            }
        }
        __syncthreads();
        tot(k + 1);
        node_out(k + 1);
    }
    // the reports: running columns from their lanes, the final columns off Xi_K; Rl[NR], Rl[NR + 1]: the two non-finite flags
    auto blk = [&](int o, int i0, int i1) {
        double t = 0.0;
        for (int i = i0; i < i1; i++) t += Xo[(o + i) * N + o + i];
        return nav_sd(t);
    };
    // trace over [i0, i1) of Cov(xhat_K - xbar_K) = Sigma_xx - C - C' + P
    auto est = [&](int i0, int i1) {
        double t = 0.0;
        for (int i = i0; i < i1; i++) t += Xo[i * N + i] - Xo[i * N + n + i] - Xo[(n + i) * N + i] + Xo[(n + i) * N + n + i];
        return nav_sd(t);
    };
    double* Nl = Rl + SCVX_COV_NREP;
    if (lane == 0) {
        Rl[SCVX_COV_SIG_PEAK] = acc0;
        Rl[NR] = bad;
    } else if (lane == 1) {
        Rl[SCVX_COV_N_MASS] = acc0;
    } else if (lane == 2) {
        Rl[SCVX_COV_N_GLIDE] = acc0;
    } else if (lane == 3) {
        Rl[SCVX_COV_N_TILT] = acc0;
    } else if (lane == 4) {
        Rl[SCVX_COV_N_RATE] = acc0;
    } else if (lane == 5) {
        Rl[SCVX_COV_S_THRUST] = acc2;
        Rl[SCVX_COV_N_TMAX] = acc0;
        Rl[SCVX_COV_N_TMIN] = acc1;
    } else if (lane == 6) {
        Rl[SCVX_COV_SIG_M] = nav_sd(Xo[0]);
    } else if (lane == 7) {
        Rl[SCVX_COV_SIG_R] = blk(0, 1, 4);
    } else if (lane == 8) {
        Rl[SCVX_COV_SIG_V] = blk(0, 4, 7);
    } else if (lane == 9) {
        Rl[SCVX_COV_SIG_Q] = blk(0, 7, 11);
    } else if (lane == 10) {
        Rl[SCVX_COV_SIG_W] = blk(0, 11, 14);
    } else if (lane == 11) {
        // eigenvalues of [[a, h], [h, d]], the horizontal block of Sigma_K (state indices 2, 3), closed form
        const double a = Xo[2 * N + 2], d = Xo[3 * N + 3], h = Xo[2 * N + 3];
        const double mean = 0.5 * (a + d), dif = 0.5 * (a - d), rad = sqrt(dif * dif + h * h);
        Rl[SCVX_COV_ELL_A] = nav_sd(mean + rad);
        Rl[SCVX_COV_ELL_B] = nav_sd(mean - rad);
        Rl[SCVX_COV_ELL_ANG] = 0.5 * atan2(2.0 * h, a - d);
    } else if (lane == 12) {
        Nl[SCVX_NAV_PEAK] = acc0;
        Rl[NR + 1] = bad;
    } else if (lane == 13) {
        Nl[SCVX_NAV_M] = blk(n, 0, 1);
    } else if (lane == 14) {
        Nl[SCVX_NAV_R] = blk(n, 1, 4);
    } else if (lane == 15) {
        Nl[SCVX_NAV_V] = blk(n, 4, 7);
    } else if (lane == 16) {
        Nl[SCVX_NAV_Q] = blk(n, 7, 11);
    } else if (lane == 17) {
        Nl[SCVX_NAV_W] = blk(n, 11, 14);
    } else if (lane == 18) {
        Nl[SCVX_NAV_EST_R] = est(1, 4);
    } else if (lane == 19) {
        Nl[SCVX_NAV_EST_V] = est(4, 7);
    }
    __syncthreads();
    const double flag = Rl[NR] + Rl[NR + 1];
    if (lane < SCVX_COV_NREP) report[(size_t)b * SCVX_COV_NREP + lane] = Rl[lane] + flag;
    else if (lane < NR) navrep[(size_t)b * SCVX_NAV_NREP + lane - SCVX_COV_NREP] = Rl[lane] + flag;
    if constexpr (PS != 0) {
        // a non-finite Xi anywhere (either flag) poisons both reports; the rows of this trajectory, and of no other, follow them
        if (flag != flag)
            for (int e = lane; e < (K + 1) * SCVX_PSIG_N; e += 64) psb[e] = flag;
    }
}

template <typename DS>
static hipError_t launch_nav_cov_t(const scvx_ctx* ctx, const CovCall& a, const DS* deriv, hipStream_t st) {
    const PathK pk = path_constants(ctx->prob);
    NavK c{pk.mdry, pk.tggs, pk.sqcm, pk.omMax, pk.Tmax, pk.Tmin, {}, {}, {}, a.m};
    for (int i = 0; i < 14; i++) c.w[i] = a.w ? a.w[i] : 0.0;
    for (int i = 0; i < a.m; i++) c.rm[i] = a.rm[i];
    for (int i = 0; i < a.m * 14; i++) c.H[i] = a.H[i];
    const dim3 g((unsigned)a.B), blk(64);
    const CovVehK vk = cov_veh_k(a);
#define SCVX_NAV_ARGS \
    g, blk, 0, st, c, a.B, a.K, a.x, a.u, deriv, a.gain, a.S0, a.N0, a.report, a.navrep, a.sig, a.navsig, a.kf, a.joint, a.psig
#define SCVX_NAV_LAUNCH(NU)                                                                    \
    do {                                                                                       \
        if (a.veh && a.psig)                                                                   \
            hipLaunchKernelGGL((nav_cov_kernel<DS, NU, 1, 1, CovVehK>), SCVX_NAV_ARGS, vk);    \
        else if (a.veh)                                                                        \
            hipLaunchKernelGGL((nav_cov_kernel<DS, NU, 0, 1, CovVehK>), SCVX_NAV_ARGS, vk);    \
        else if (a.psig)                                                                       \
            hipLaunchKernelGGL((nav_cov_kernel<DS, NU, 1>), SCVX_NAV_ARGS);                    \
        else                                                                                   \
            hipLaunchKernelGGL((nav_cov_kernel<DS, NU, 0>), SCVX_NAV_ARGS);                    \
    } while (0)
    if (ctx->dyn.fin) SCVX_NAV_LAUNCH(5);
    else SCVX_NAV_LAUNCH(3);
#undef SCVX_NAV_LAUNCH
#undef SCVX_NAV_ARGS
    return hipGetLastError();
}

hipError_t launch_nav_call(const scvx_ctx* ctx, const CovCall& c, hipStream_t st) {
    return c.deriv.d ? launch_nav_cov_t(ctx, c, c.deriv.d, st) : launch_nav_cov_t(ctx, c, c.deriv.f, st);
}

int check_nav_model(scvx_ctx* ctx, int m, const double* H, const double* rm) {
    if (!ctx) return SCVX_ERR_ARG;
    if (m < 0 || m > 14) return fail(ctx, SCVX_ERR_ARG, "nav: the number of measurements m must be in [0,14]");
    if (m > 0 && (!H || !rm)) return fail(ctx, SCVX_ERR_ARG, "nav: m > 0 needs H[m][14] and rm[m]");
    for (int i = 0; i < m; i++)
        if (!(rm[i] > 0.0) || !std::isfinite(rm[i])) return fail(ctx, SCVX_ERR_ARG, "nav: the measurement variances rm must be finite and > 0");
    for (int i = 0; i < m * 14; i++)
        if (!std::isfinite(H[i])) return fail(ctx, SCVX_ERR_ARG, "nav: the measurement matrix H must be finite");
    return SCVX_OK;
}

}  // namespace scvx

// the record of the navigation forms: what every one of them takes
static scvx::CovCall nav_record(int B, int K, const double* x, const double* u, const double* deriv, const double* gain, const double* S0,
                                const double* N0, int m, const double* H, const double* rm, const double* w14, double* report,
                                double* navrep) {
    scvx::CovCall c = scvx::cov_record(B, K, x, u, deriv, gain, S0, w14, report);
    c.nav = true, c.N0 = N0, c.m = m, c.H = H, c.rm = rm, c.navrep = navrep;
    return c;
}

extern "C" {

int scvx_nav_cov_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                     const double* gain_dev, const double* S0_dev, const double* N0_dev, int m, const double* H, const double* rm,
                     const double* w14, double* report_dev, double* navrep_dev, double* sig_dev, double* navsig_dev, double* kf_dev,
                     double* joint_dev) {
    scvx::CovCall c = nav_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, N0_dev, m, H, rm, w14, report_dev, navrep_dev);
    c.sig = sig_dev, c.navsig = navsig_dev, c.kf = kf_dev, c.joint = joint_dev;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_nav_path_sigma_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                            const double* gain_dev, const double* S0_dev, const double* N0_dev, int m, const double* H, const double* rm,
                            const double* w14, double* report_dev, double* navrep_dev, double* psig_dev) {
    scvx::CovCall c = nav_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, N0_dev, m, H, rm, w14, report_dev, navrep_dev);
    c.psig = psig_dev, c.need_psig = true;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_nav_cov_vehicle_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                             const double* gain_dev, const double* S0_dev, const double* N0_dev, int m, const double* H, const double* rm,
                             const double* w14, double* report_dev, double* navrep_dev, double* psig_dev, double* sig_dev,
                             double* navsig_dev, double* kf_dev, double* joint_dev, const double* vtile_dev, const double* sp6,
                             double* sens_dev) {
    scvx::CovCall c = nav_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, N0_dev, m, H, rm, w14, report_dev, navrep_dev);
    c.psig = psig_dev, c.sig = sig_dev, c.navsig = navsig_dev, c.kf = kf_dev, c.joint = joint_dev;
    c.veh = true, c.vtile = vtile_dev, c.sp6 = sp6, c.sens = sens_dev;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_nav_cov_vehicle_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                                  const double* S0, const double* N0, int m, const double* H, const double* rm, const double* w14,
                                  double* report, double* navrep, double* psig, double* sig, double* navsig, double* kf, double* joint,
                                  const double* vtile, const double* sp6, double* sens) {
    scvx::CovCall c = nav_record(B, K, x, u, deriv, gain, S0, N0, m, H, rm, w14, report, navrep);
    c.psig = psig, c.sig = sig, c.navsig = navsig, c.kf = kf, c.joint = joint, c.veh = true, c.vtile = vtile, c.sp6 = sp6, c.sens = sens;
    return scvx::cov_call_host(ctx, c, "scvx_nav_cov_vehicle_f64_host");
}

int scvx_nav_path_sigma_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                                 const double* S0, const double* N0, int m, const double* H, const double* rm, const double* w14,
                                 double* report, double* navrep, double* psig) {
    scvx::CovCall c = nav_record(B, K, x, u, deriv, gain, S0, N0, m, H, rm, w14, report, navrep);
    c.psig = psig, c.need_psig = true;
    return scvx::cov_call_host(ctx, c, "scvx_nav_path_sigma_f64_host");
}

int scvx_nav_cov_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                          const double* S0, const double* N0, int m, const double* H, const double* rm, const double* w14, double* report,
                          double* navrep, double* sig, double* navsig, double* kf, double* joint) {
    scvx::CovCall c = nav_record(B, K, x, u, deriv, gain, S0, N0, m, H, rm, w14, report, navrep);
    c.sig = sig, c.navsig = navsig, c.kf = kf, c.joint = joint;
    return scvx::cov_call_host(ctx, c, "scvx_nav_cov_f64_host");
}

int scvx_track_fly_nav_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* sigma_dev,
                           const double* gain_dev, const double* dx0_dev, const double* nav_dev, int nsub, int flags,
                           double* report_dev, double* xfly_dev, double* ufly_dev) {
    int rc = scvx::check_track_fly(ctx, B, K, x_dev, u_dev, sigma_dev, gain_dev, nsub, flags, report_dev);
    if (rc) return rc;
    if (!nav_dev) return scvx::fail(ctx, SCVX_ERR_ARG, "track fly nav: null nav (without one, call scvx_track_fly_f64)");
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_fly_nav(ctx, B, K, x_dev, u_dev, sigma_dev, gain_dev, dx0_dev, nav_dev, nsub, flags, report_dev,
                                             xfly_dev, ufly_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_track_fly_nav_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, const double* gain,
                                const double* dx0, const double* nav, int nsub, int flags, double* report, double* xfly, double* ufly) {
    int rc = scvx::check_track_fly(ctx, B, K, x, u, sigma, gain, nsub, flags, report);
    if (rc) return rc;
    if (!nav) return scvx::fail(ctx, SCVX_ERR_ARG, "track fly nav: null nav (without one, call scvx_track_fly_f64_host)");
    const scvx::Dims d(B, K, scvx_control_dim(ctx));
    scvx::Staging s(ctx);
    const double *dx = s.in(x, d.x), *du = s.in(u, d.u), *ds = s.in(sigma, d.b), *dg = s.in(gain, d.gain), *dv = s.in(nav, d.seg),
                 *d0 = s.in(dx0, d.b14);
    double *dr = s.out(report, d.frep), *df = s.out(xfly, d.x), *dc = s.out(ufly, d.u);
    s.launch([&] { return scvx::launch_track_fly_nav(ctx, B, K, dx, du, ds, dg, d0, dv, nsub, flags, dr, df, dc, s.st); });
    return s.finish("scvx_track_fly_nav_f64_host");
}

}  // extern "C"
