// Closed-loop covariance analysis of tracked plans (scvx_cov_propagate_f64, include/scvx.h): the covariance of the augmented deviation
// z_k = [dx_k; du_k] under the tracking law of scvx_track.hip, Sigma_{k+1} = M_k Sigma_k M_k' + diag(w, 0), M_k = F_k + G_k L_k, and the
// per-trajectory dispersion report read off it.  No counterpart in the reference.
//
// cov_propagate_kernel: ONE WAVEFRONT PER TRAJECTORY, K sequential steps -- track_gains_kernel run forwards.  The rows 14.. of M_k are
// L_k itself and only its 14 top rows meet the tile, so M is never stored as a matrix: the top rows are formed IN PLACE in the tile's
// [A | B-] columns (Mtop = [A B-] + B+ L: the B+ columns are read, never written), the bottom rows are read from L.  One step is
//     Mtop = [A B-] + B+ L (14 x n, NU deep),  V = M Sigma (n x n, n deep; Sigma symmetric, read by rows),
//     T = V M' (n x n, n deep) written over Sigma,  Sigma = (T + T') / 2 + diag(w, 0): every pair from both of its triangles
// with Sigma, the tile, L and V in LDS (7,432 B at NU = 3, 9,384 B at NU = 5: below the gains kernel's 10,080 / 13,088 B).  The two
// n-deep products are the work.  MF = 0: one lane per output element.  MF = 1: the 16 x 16 corner of each product on the FP64
// matrix pipe (5 x v_mfma_f64_16x16x4_f64: n = 17 / 19 pads to 20 k-slots) and the border (n^2 - 256 = 33 / 105 elements) one lane per
// element -- two 16 x 16 tiles per side would spend three quarters of the matrix work on padding.  The tile and the gain block of step
// k + 1 are fetched into registers while step k computes and stored to LDS behind the step's last barrier.  DS is the tiles' storage type
// (double, or float with scvx_batch_set_linearization_f32: widened on load).
//
// The report is a handful of sparse quadratic forms per node: lanes 0..5 each carry one running extremum in registers (the plan values
// of node k + 1 they need are loaded at the top of step k), lanes 6..11 read the final columns off Sigma_K.
#include <cmath>
#include <cstdlib>
#include <limits>
#include "scvx_cov.hpp"

namespace scvx {

// the constants of the path functions it reads (path_constants) and the process noise
struct CovK {
    double mdry, tggs, sqcm, omMax, Tmax, Tmin;
    double w[14];
};

typedef double cov_v4f64 __attribute__((ext_vector_type(4)));

// square root of a variance (a rounded variance of -1e-40 is 0, a NaN stays a NaN)
__device__ __forceinline__ double cov_sd(double v) { return v > 0.0 ? sqrt(v) : (v != v ? v : 0.0); }

// c' Sigma c for a gradient with (up to) three nonzeros c0, c1, c2 at i0, i1, i2
__device__ __forceinline__ double cov_quad3(const double* S, int n, int i0, int i1, int i2, double c0, double c1, double c2) {
    const double d = c0 * c0 * S[i0 * n + i0] + c1 * c1 * S[i1 * n + i1] + c2 * c2 * S[i2 * n + i2];
    const double o = c0 * c1 * S[i0 * n + i1] + c0 * c2 * S[i0 * n + i2] + c1 * c2 * S[i1 * n + i2];
    return d + 2.0 * o;
}

// The 16 x 16 corner C[0..15][0..15] of an n-deep product on the FP64 matrix pipe (fragment maps as track_mm16: A: lane l holds
// A[l & 15][l >> 4], B: B[l >> 4][l & 15], C: register r of lane l is C[(l >> 4) + 4 r][l & 15]).  n >= 17, so every row and column of
// the corner exists; k-slots >= KD are fed zeros from a clamped, valid address.
template <int KD, class FA, class FB, class FC>
__device__ __forceinline__ void cov_mm16(FA fa, FB fb, FC store, int lane) {
    const int rc = lane & 15, kq = lane >> 4;
    cov_v4f64 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < (KD + 3) / 4; s++) {
        const int k = 4 * s + kq, kc = k < KD ? k : KD - 1;
        const double a = fa(rc, kc), b = fb(kc, rc);
        c = __builtin_amdgcn_mfma_f64_16x16x4f64(k < KD ? a : 0.0, k < KD ? b : 0.0, c, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; r++) store(kq + 4 * r, rc, c[r]);
}

// MF: 0 = one lane per element, 1 = the 16 x 16 corner of the two n-deep products on the matrix pipe
// PS: 1 = also keep the per-node s = sqrt(c' Sigma_k c) of the five path functions that lanes 1..5 form for the margins
// (scvx_cov_path_sigma_f64: psig [B][K+1][SCVX_PSIG_N]); 0 = the report alone, and nothing of it is compiled in
// VEH: 1 = vehicle errors as consider parameters (scvx_cov_vehicle_f64, include/scvx.h).  J_k = d z_k / d theta (n x 6) is carried in LDS
// beside Sigma_k, J_{k+1} = M_k J_k + [Gamma_k; 0], in two buffers that alternate (the update rides in the V pass: no barrier of its
// own).  Gamma_k's four control columns are formed from the tile's B- / B+ columns and the plan's controls BEFORE Mtop overwrites
// [A B-] in place (one barrier), its ISP and AERO columns are read from vtile.  Everything node_out and the final report read comes
// from Sigma_k^tot = Sigma_k + J_k diag(sp^2) J_k', formed in V (dead between the T pass and the next step's V pass) behind the step's
// last barrier (one more barrier); Sigma_k itself is never touched.  Every statement of it sits under `if constexpr (VEH)` and its
// kernel argument (CovVehK) is a trailing pack that is empty without it: the instantiations without VEH keep their code.
// SAT: 1 = the clamp-aware analysis by statistical linearisation (scvx_cov_clamp_f64, include/scvx.h): a mean mu_k (n, in LDS) is
// carried beside Sigma_k, and at every step, BEFORE Mtop overwrites [A B-] in place, the mean command chat = ubar_{k+1} + L mu (lane
// j < NU one n-deep dot product, then NU shuffles: no barrier), g = L[0:3,:]' e and s^2 = g' Sigma g (one n-deep matrix-vector pass, one barrier, a wavefront
// reduction that leaves every lane the same bits), the scalars P_lo, P_hi, gamma, E (uniform: a wavefront runs them once for all its
// lanes), mu_{k+1} from the untouched [A | B- | B+] columns (kept in a register until Mtop's barrier), and the three thrust rows of L
// overwritten with N L (one more barrier).  After that the step is the plain one.  An unsaturated node (P_lo == P_hi == 0) touches
// neither L nor the arithmetic of Sigma.  Every statement of it sits under `if constexpr (SAT)` and its kernel argument (CovSatK) is the
// trailing pack's one element; SAT with VEH is not instantiated.
template <typename DS, int NU, int MF, int PS = 0, int VEH = 0, int SAT = 0, typename... VA>
__global__ __launch_bounds__(64) void cov_propagate_kernel(CovK c, int B, int K, const double* __restrict__ x, const double* __restrict__ u,
                                                           const DS* __restrict__ deriv, const double* __restrict__ gain,
                                                           const double* __restrict__ S0, double* __restrict__ report,
                                                           double* __restrict__ sig, double* __restrict__ covK, double* __restrict__ cov,
                                                           double* __restrict__ psig, VA... va) {
    static_assert(sizeof...(VA) == (VEH || SAT ? 1 : 0), "the VEH / SAT instantiations take one CovVehK / CovSatK behind psig, the others nothing");
    static_assert(!(VEH && SAT), "the clamp-aware analysis has no vehicle-error form");
    constexpr int n = 14 + NU, m = 14 + 2 * NU, NC = m + 1, DSZ = 14 * NC, ND = 14 * m, NL = NU * n, NN = n * n;
    constexpr int NJ = n * SCVX_VEH_N;
    constexpr int NPRE = (ND + 63) / 64, NLPRE = (NL + 63) / 64;
    constexpr int NBORD = NN - 256;   // elements of an n x n product outside its 16 x 16 corner
    __shared__ double Sl[NN], Dl[ND], Ll[NL], Vl[NN], Rl[SCVX_COV_NREP + 1];
    __shared__ double Jl[VEH ? 2 * NJ : 1], Gml[VEH ? 14 * SCVX_VEH_N : 1];   // VEH: J_k and J_{k+1}; Gamma_k, column-major
    __shared__ double Mul[SAT ? n : 1], Gl[SAT ? n : 1];                       // SAT: mu_k; g = L[0:3,:]' e
    const double* const So = VEH ? Vl : Sl;   // what the outputs read: Sigma_k, with VEH Sigma_k^tot
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const DS* tiles = deriv + (size_t)b * K * DSZ;
    const double* gb = gain + (size_t)b * K * NL;
    const double* xb = x + (size_t)b * (K + 1) * 14;
    const double* ub = u + (size_t)b * (K + 1) * NU;
    const double* s0 = S0 + (size_t)b * 196;
    double* covb = cov ? cov + (size_t)b * (K + 1) * NN : nullptr;
    double* sigb = sig ? sig + (size_t)b * (K + 1) * n : nullptr;
    double* psb = PS ? psig + (size_t)b * (K + 1) * SCVX_PSIG_N : nullptr;
    const double inf = std::numeric_limits<double>::infinity();
    // Sigma_0 = blockdiag((S0 + S0') / 2, 0); tile 0 and gain block 0
    for (int e = lane; e < NN; e += 64) {
        const int a = e / n, cc = e % n;
        Sl[e] = (a < 14 && cc < 14) ? 0.5 * (s0[a * 14 + cc] + s0[cc * 14 + a]) : 0.0;
    }
    for (int e = lane; e < ND; e += 64) Dl[e] = (double)tiles[e];
    for (int e = lane; e < NL; e += 64) Ll[e] = gb[e];
    if constexpr (VEH)
        for (int e = lane; e < NJ; e += 64) Jl[e] = 0.0;
    // SAT: the running columns of satrep, the same in every lane: sums of P_lo and P_hi, min gamma, max |mu_k[0:14]|
    [[maybe_unused]] double splo = 0.0, sphi = 0.0, gmin = inf, bpk = 0.0;
    if constexpr (SAT) {
        const CovSatK& sk = veh_first(va...);
        if (lane < n) {
            Mul[lane] = 0.0;
            if (sk.mean) sk.mean[(size_t)b * (K + 1) * n + lane] = 0.0;
        }
    }
    // the running columns: lane 0 SIG_PEAK (and the non-finite flag), 1 N_MASS, 2 N_GLIDE, 3 N_TILT, 4 N_RATE, 5 S_THRUST / N_TMAX / N_TMIN
    double acc0 = lane == 0 ? 0.0 : inf, acc1 = inf, acc2 = 0.0, bad = 0.0;
    double pv0 = 0.0, pv1 = 0.0, pv2 = 0.0;
    __syncthreads();
    // row a of M: the top rows sit in the tile's first n columns (column-major, stride 14), the bottom rows are L's
    auto mrow = [&](int a, int& st) -> const double* {
        st = a < 14 ? 14 : 1;
        return a < 14 ? Dl + a : Ll + (a - 14) * n;
    };
    auto velem = [&](int a, int cc) {   // V[a][cc] = sum_l M[a][l] Sigma[cc][l]
        int st;
        const double* mp = mrow(a, st);
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < n; l++) s = fma(mp[l * st], Sl[cc * n + l], s);
        return s;
    };
    auto telem = [&](int a, int cc) {   // T[a][cc] = sum_l V[a][l] M[cc][l]
        int st;
        const double* mp = mrow(cc, st);
        double s = 0.0;
#pragma unroll
        for (int l = 0; l < n; l++) s = fma(Vl[a * n + l], mp[l * st], s);
        return s;
    };
    auto border = [](int e, int& a, int& cc) {   // e < NBORD: rows 16.. first, then the columns 16.. of rows 0..15
        if (e < (n - 16) * n) {
            a = 16 + e / n;
            cc = e % n;
        } else {
            e -= (n - 16) * n;
            a = e % 16;
            cc = 16 + e / 16;
        }
    };
    // dense outputs and the running columns at node k (Sigma_k in Sl; pv*: the plan values of node k this lane's column reads)
    auto node_out = [&](int k) {
        if (covb)
            for (int e = lane; e < NN; e += 64) covb[(size_t)k * NN + e] = So[e];
        if (sigb && lane < n) sigb[(size_t)k * n + lane] = cov_sd(So[lane * n + lane]);
        if (lane == 0) {
            double tr = 0.0;
#pragma unroll
            for (int i = 0; i < 14; i++) tr += So[i * n + i];
            bad = fma(tr, 0.0, bad);
            acc0 = nan_max(acc0, cov_sd(tr));
        } else if (k > 0 && lane < 6) {
            double sv = 0.0;   // PS: this lane's s at node k (0 where the margin skips the node)
            if (lane == 1) {
                const double s = cov_sd(So[0]);
                sv = s;
                if (!(s == 0.0)) acc0 = nan_min(acc0, -(c.mdry - pv0) / s);
            } else if (lane == 5) {
                const double nr = sqrt(pv0 * pv0 + pv1 * pv1 + pv2 * pv2);
                if (!(nr == 0.0)) {
                    const double s = cov_sd(cov_quad3(So, n, 14, 15, 16, pv0 / nr, pv1 / nr, pv2 / nr));
                    acc2 = nan_max(acc2, s);
                    sv = s;
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
                        q = cov_quad3(So, n, 1, 2, 3, -1.0, c.tggs * a0 / nr, c.tggs * a1 / nr);
                    } else if (lane == 3) {
                        g = nr - c.sqcm;
                        q = cov_quad3(So, n, 9, 10, 10, a0 / nr, a1 / nr, 0.0);
                    } else {
                        g = nr - c.omMax;
                        q = cov_quad3(So, n, 11, 12, 13, a0 / nr, a1 / nr, a2 / nr);
                    }
                    const double s = cov_sd(q);
                    sv = s;
                    if (!(s == 0.0)) acc0 = nan_min(acc0, -g / s);
                }
            }
            if constexpr (PS != 0) psb[(size_t)k * SCVX_PSIG_N + (lane - 1)] = sv;
        } else if (PS != 0 && lane < 6) {
            psb[lane - 1] = 0.0;   // node 0: no margin reads it
        }
    };
    // VEH: Sigma_k^tot = Sigma_k + J_k diag(sp^2) J_k' into V, J_k (in the buffer k & 1) out as sens; (J J) p keeps it symmetric bit for bit,
    // and a zero update leaves the very Sigma_k
    auto tot = [&](int k) {
        if constexpr (VEH) {
            const CovVehK& vk = veh_first(va...);
            const double* Jc = Jl + (k & 1) * NJ;
            for (int e = lane; e < NN; e += 64) {
                const int a = e / n, cc = e % n;
                double t = 0.0;
#pragma unroll
                for (int j = 0; j < SCVX_VEH_N; j++) t = fma(Jc[a * SCVX_VEH_N + j] * Jc[cc * SCVX_VEH_N + j], vk.p[j], t);
                Vl[e] = t == 0.0 ? Sl[e] : Sl[e] + t;
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
        [[maybe_unused]] double mun = 0.0;   // SAT: mu_{k+1}[lane], stored behind Mtop's barrier
        if constexpr (SAT) {
            const CovSatK& sk = veh_first(va...);
            const double* un = ub + (size_t)(k + 1) * NU;
            // 1, 2: the mean command, its norm and direction; dl = L mu is the mean deviation of the command
            // (lane j < NU forms row j's dot product, the lanes behind it row NU - 1 again; every lane then takes all NU)
            double dl[NU];
            double dj = 0.0;
            {
                const double* lr = Ll + (lane < NU ? lane : NU - 1) * n;
#pragma unroll
                for (int l = 0; l < n; l++) dj = fma(lr[l], Mul[l], dj);
            }
#pragma unroll
            for (int j = 0; j < NU; j++) dl[j] = __shfl(dj, j);
            const double c0 = un[0] + dl[0], c1 = un[1] + dl[1], c2 = un[2] + dl[2];
            const double That = sqrt(c0 * c0 + c1 * c1 + c2 * c2);
            const bool zero = That == 0.0;   // the flight's clamp leaves a zero thrust alone
            const double e0 = zero ? 0.0 : c0 / That, e1 = zero ? 0.0 : c1 / That, e2 = zero ? 0.0 : c2 / That;
            // 3: g and s
            double gl = 0.0;
            if (lane < n) {
                gl = fma(Ll[2 * n + lane], e2, fma(Ll[n + lane], e1, Ll[lane] * e0));
                Gl[lane] = gl;
            }
            __syncthreads();
            double q = 0.0;
            if (lane < n) {
                double t = 0.0;
#pragma unroll
                for (int l = 0; l < n; l++) t = fma(Sl[lane * n + l], Gl[l], t);
                q = gl * t;
            }
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) q += __shfl_xor(q, o);
            const double s = cov_sd(q);
            // 4, 5: the shares, the describing-function gain and the mean of the clamped norm
            // (E is formed as That + dE, dE = E - That = s (a P_lo + b P_hi + phi(a) - phi(b)): where the clamp is rarely reached every
            // term of dE is small, and the mean's input dE e does not come out of a difference of terms of the plan's own size)
            double plo, phi, gam, dE;
            if (zero) {
                plo = 0.0, phi = 0.0, gam = 1.0, dE = 0.0;
            } else if (s == 0.0) {
                plo = That < sk.Tlo ? 1.0 : 0.0, phi = That > sk.Thi ? 1.0 : 0.0;
                gam = (plo == 0.0 && phi == 0.0) ? 1.0 : 0.0;
                dE = fmin(fmax(That, sk.Tlo), sk.Thi) - That;
            } else {
                constexpr double r2 = 1.4142135623730951, i2p = 0.3989422804014327;   // sqrt 2, 1 / sqrt(2 pi)
                const double a = (sk.Tlo - That) / s, bb = (sk.Thi - That) / s;
                const bool nolo = sk.Tlo == 0.0;   // a norm is never below 0: no lower clamp, as Thi = +inf is no upper one
                plo = nolo ? 0.0 : 0.5 * erfc(-a / r2), phi = 0.5 * erfc(bb / r2);
                gam = 1.0 - plo - phi;
                const double hi = phi == 0.0 ? 0.0 : bb * phi, pa = nolo ? 0.0 : i2p * exp(-0.5 * a * a);
                dE = s * (a * plo + hi + (pa - i2p * exp(-0.5 * bb * bb)));
            }
            const double E = That + dE;
            const bool satd = !(plo == 0.0 && phi == 0.0);   // a NaN saturates: it reaches L, Sigma and the reports
            // 6, 7: the applied mean about the plan, and mu_{k+1} from the untouched tile
            if (satd) dl[0] = fma(dE, e0, dl[0]), dl[1] = fma(dE, e1, dl[1]), dl[2] = fma(dE, e2, dl[2]);   // E e - ubar = L mu + dE e
            if (lane < 14) {
                double t = 0.0;
#pragma unroll
                for (int l = 0; l < n; l++) t = fma(Dl[l * 14 + lane], Mul[l], t);
#pragma unroll
                for (int j = 0; j < NU; j++) t = fma(Dl[(n + j) * 14 + lane], dl[j], t);
                mun = t;
            } else if (lane < n) {
#pragma unroll
                for (int j = 0; j < NU; j++)
                    if (lane == 14 + j) mun = dl[j];
            }
            // 8: the thrust rows of L become N L = (E / That) L + (gamma - E / That) e g'
            if (satd && lane < n) {
                const double r = E / That, d = (gam - r) * gl;
                Ll[lane] = fma(r, Ll[lane], d * e0);
                Ll[n + lane] = fma(r, Ll[n + lane], d * e1);
                Ll[2 * n + lane] = fma(r, Ll[2 * n + lane], d * e2);
            }
            if (lane == 0 && sk.satk) {
                double* o = sk.satk + ((size_t)b * K + k) * 4;
                o[0] = That, o[1] = s, o[2] = plo, o[3] = phi;
            }
            if (sk.mean && lane < n) sk.mean[((size_t)b * (K + 1) + k + 1) * n + lane] = mun;
            splo += plo, sphi += phi;
            gmin = nan_min(gmin, gam);
            __syncthreads();
        }
        if constexpr (VEH) {
            // Gamma_k's columns (include/scvx.h), while the tile still holds B-
            const CovVehK& vk = veh_first(va...);
            const double* vt = vk.vtile ? vk.vtile + ((size_t)b * K + k) * SCVX_VTILE_N * 14 : nullptr;
            for (int e = lane; e < 14 * SCVX_VEH_N; e += 64) Gml[e] = veh_gamma<NU>(Dl, ub + (size_t)k * NU, vt, e % 14, e / 14);
            __syncthreads();
        }
        // Mtop = [A B-] + B+ L, in place
        for (int e = lane; e < 14 * n; e += 64) {
            const int i = e % 14, cc = e / 14;
            double s = Dl[e];
#pragma unroll
            for (int j = 0; j < NU; j++) s = fma(Dl[(n + j) * 14 + i], Ll[j * n + cc], s);
            Dl[e] = s;
        }
        __syncthreads();
        if constexpr (SAT)
            if (lane < n) Mul[lane] = mun;   // next read behind the step's later barriers
        // V = M Sigma
        if (MF) {
            cov_mm16<n>([&](int i, int l) { int st; const double* mp = mrow(i, st); return mp[l * st]; },
                        [&](int l, int j) { return Sl[j * n + l]; }, [&](int i, int j, double v) { Vl[i * n + j] = v; }, lane);
            for (int e = lane; e < NBORD; e += 64) {
                int a, cc;
                border(e, a, cc);
                Vl[a * n + cc] = velem(a, cc);
            }
        } else {
            for (int e = lane; e < NN; e += 64) {
                const int a = e % n, cc = e / n;
                Vl[a * n + cc] = velem(a, cc);
            }
        }
        if constexpr (VEH) {
            // J_{k+1} = M J_k + [Gamma_k; 0] into the other buffer
            const double* Jc = Jl + (k & 1) * NJ;
            double* Jn = Jl + ((k + 1) & 1) * NJ;
            for (int e = lane; e < NJ; e += 64) {
                const int a = e / SCVX_VEH_N, cI = e % SCVX_VEH_N;
                int st;
                const double* mp = mrow(a, st);
                double s = a < 14 ? Gml[cI * 14 + a] : 0.0;
#pragma unroll
                for (int l = 0; l < n; l++) s = fma(mp[l * st], Jc[l * SCVX_VEH_N + cI], s);
                Jn[e] = s;
            }
        }
        __syncthreads();
        // T = V M', over Sigma (no longer read)
        if (MF) {
            cov_mm16<n>([&](int i, int l) { return Vl[i * n + l]; },
                        [&](int l, int j) { int st; const double* mp = mrow(j, st); return mp[l * st]; },
                        [&](int i, int j, double v) { Sl[i * n + j] = v; }, lane);
            for (int e = lane; e < NBORD; e += 64) {
                int a, cc;
                border(e, a, cc);
                Sl[a * n + cc] = telem(a, cc);
            }
        } else {
            for (int e = lane; e < NN; e += 64) {
                const int cc = e % n, a = e / n;
                Sl[e] = telem(a, cc);
            }
        }
        __syncthreads();
        // Sigma_{k+1} = (T + T') / 2 + diag(w, 0): one lane per pair, both triangles written with the same value
        for (int e = lane; e < NN; e += 64) {
            const int a = e / n, cc = e % n;
            if (a < cc) {
                const double s = 0.5 * (Sl[a * n + cc] + Sl[cc * n + a]);
                Sl[a * n + cc] = s;
                Sl[cc * n + a] = s;
            } else if (a == cc && a < 14) {
                Sl[e] += c.w[a];
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
        if constexpr (SAT) {
            double t = 0.0;
#pragma unroll
            for (int i = 0; i < 14; i++) t = fma(Mul[i], Mul[i], t);
            bpk = nan_max(bpk, sqrt(t));
        }
        tot(k + 1);
        node_out(k + 1);
    }
    // the report: running columns from their lanes, the final columns off Sigma_K
    if (covK) {
        double* o = covK + (size_t)b * NN;
        for (int e = lane; e < NN; e += 64) o[e] = So[e];
    }
    auto blk = [&](int i0, int i1) {
        double t = 0.0;
        for (int i = i0; i < i1; i++) t += So[i * n + i];
        return cov_sd(t);
    };
    if (lane == 0) {
        Rl[SCVX_COV_SIG_PEAK] = acc0;
        Rl[SCVX_COV_NREP] = bad;
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
        Rl[SCVX_COV_SIG_M] = cov_sd(So[0]);
    } else if (lane == 7) {
        Rl[SCVX_COV_SIG_R] = blk(1, 4);
    } else if (lane == 8) {
        Rl[SCVX_COV_SIG_V] = blk(4, 7);
    } else if (lane == 9) {
        Rl[SCVX_COV_SIG_Q] = blk(7, 11);
    } else if (lane == 10) {
        Rl[SCVX_COV_SIG_W] = blk(11, 14);
    } else if (lane == 11) {
        // eigenvalues of [[a, h], [h, d]], the horizontal block of Sigma_K (state indices 2, 3), closed form
        const double a = So[2 * n + 2], d = So[3 * n + 3], h = So[2 * n + 3];
        const double mean = 0.5 * (a + d), dif = 0.5 * (a - d), rad = sqrt(dif * dif + h * h);
        Rl[SCVX_COV_ELL_A] = cov_sd(mean + rad);
        Rl[SCVX_COV_ELL_B] = cov_sd(mean - rad);
        Rl[SCVX_COV_ELL_ANG] = 0.5 * atan2(2.0 * h, a - d);
    }
    __syncthreads();
    if (lane < SCVX_COV_NREP) report[(size_t)b * SCVX_COV_NREP + lane] = Rl[lane] + Rl[SCVX_COV_NREP];
    if constexpr (SAT) {
        // satrep: one column per lane; the poison of the report is its poison
        const CovSatK& sk = veh_first(va...);
        auto mblk = [&](int i0, int i1) {
            double t = 0.0;
            for (int i = i0; i < i1; i++) t += Mul[i] * Mul[i];
            return sqrt(t);
        };
        if (lane < SCVX_SAT_NREP) {
            double v;
            if (lane <= SCVX_SAT_SIG_W) {
                v = Rl[lane];   // SCVX_SAT_SIG_* are SCVX_COV_SIG_*
            } else if (lane == SCVX_SAT_BIAS_M) {
                v = fabs(Mul[0]);
            } else if (lane == SCVX_SAT_BIAS_R || lane == SCVX_SAT_RMS_R) {
                v = mblk(1, 4);
                if (lane == SCVX_SAT_RMS_R) v = sqrt(Rl[SCVX_COV_SIG_R] * Rl[SCVX_COV_SIG_R] + v * v);
            } else if (lane == SCVX_SAT_BIAS_V || lane == SCVX_SAT_RMS_V) {
                v = mblk(4, 7);
                if (lane == SCVX_SAT_RMS_V) v = sqrt(Rl[SCVX_COV_SIG_V] * Rl[SCVX_COV_SIG_V] + v * v);
            } else if (lane == SCVX_SAT_BIAS_Q) {
                v = mblk(7, 11);
            } else if (lane == SCVX_SAT_BIAS_W) {
                v = mblk(11, 14);
            } else if (lane == SCVX_SAT_P_LO) {
                v = splo / K;
            } else if (lane == SCVX_SAT_P_HI) {
                v = sphi / K;
            } else if (lane == SCVX_SAT_GAIN_MIN) {
                v = gmin;
            } else {
                v = bpk;
            }
            sk.satrep[(size_t)b * SCVX_SAT_NREP + lane] = v + Rl[SCVX_COV_NREP];
        }
    }
    if constexpr (PS != 0) {
        // a non-finite Sigma anywhere poisons the report; the rows of this trajectory follow it
        const double bd = Rl[SCVX_COV_NREP];
        if (bd != bd)
            for (int e = lane; e < (K + 1) * SCVX_PSIG_N; e += 64) psb[e] = bd;
    }
}

constexpr bool kCovMfmaDefault = false;   // the lane form, which the parity tests pin, until the A/B of tools/bench_cov.py is measured

template <typename DS>
static hipError_t launch_cov_t(const scvx_ctx* ctx, const CovCall& a, const DS* deriv, hipStream_t st) {
    const PathK pk = path_constants(ctx->prob);
    CovK c{pk.mdry, pk.tggs, pk.sqcm, pk.omMax, pk.Tmax, pk.Tmin, {}};
    for (int i = 0; i < 14; i++) c.w[i] = a.w ? a.w[i] : 0.0;
    // SCVX_COV_MFMA = 0 / 1 forces the lane-per-element / matrix-pipe form of the two n-deep products (A/B: tools/bench_cov.py)
    bool mf = kCovMfmaDefault;
    if (const char* v = std::getenv("SCVX_COV_MFMA"); v && *v) mf = std::atoi(v) != 0;
    const dim3 g((unsigned)a.B), blk(64);
    const CovVehK vk = cov_veh_k(a);
    const CovSatK sk = cov_sat_k(a, pk.Tmin, pk.Tmax);
#define SCVX_COV_ARGS g, blk, 0, st, c, a.B, a.K, a.x, a.u, deriv, a.gain, a.S0, a.report, a.sig, a.covK, a.cov, a.psig
#define SCVX_COV_LAUNCH(NU, MF)                                                                      \
    do {                                                                                             \
        if (a.sat)                                                                                   \
            hipLaunchKernelGGL((cov_propagate_kernel<DS, NU, MF, 0, 0, 1, CovSatK>), SCVX_COV_ARGS, sk); \
        else if (a.veh && a.psig)                                                                    \
            hipLaunchKernelGGL((cov_propagate_kernel<DS, NU, MF, 1, 1, 0, CovVehK>), SCVX_COV_ARGS, vk); \
        else if (a.veh)                                                                              \
            hipLaunchKernelGGL((cov_propagate_kernel<DS, NU, MF, 0, 1, 0, CovVehK>), SCVX_COV_ARGS, vk); \
        else if (a.psig)                                                                             \
            hipLaunchKernelGGL((cov_propagate_kernel<DS, NU, MF, 1>), SCVX_COV_ARGS);                \
        else                                                                                         \
            hipLaunchKernelGGL((cov_propagate_kernel<DS, NU, MF, 0>), SCVX_COV_ARGS);                \
    } while (0)
    if (ctx->dyn.fin) {
        if (mf) SCVX_COV_LAUNCH(5, 1);
        else SCVX_COV_LAUNCH(5, 0);
    } else {
        if (mf) SCVX_COV_LAUNCH(3, 1);
        else SCVX_COV_LAUNCH(3, 0);
    }
#undef SCVX_COV_LAUNCH
#undef SCVX_COV_ARGS
    return hipGetLastError();
}

hipError_t launch_cov_call(const scvx_ctx* ctx, const CovCall& c, hipStream_t st) {
    if (c.nav) return launch_nav_call(ctx, c, st);
    return c.deriv.d ? launch_cov_t(ctx, c, c.deriv.d, st) : launch_cov_t(ctx, c, c.deriv.f, st);
}

int check_cov_call(scvx_ctx* ctx, const CovCall& c, const CovBatch* own) {
    if (!ctx) return SCVX_ERR_ARG;
    const bool margins = own && own->margins;
    int rc;
    if (!own) {
        if (c.B < 1) return fail(ctx, SCVX_ERR_ARG, "cov: B >= 1 required");
        if (c.K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "cov: K must equal the problem's K");
        if (!c.x || !c.u || !(c.deriv.d || c.deriv.f) || !c.gain || !c.S0 || !c.report) return fail(ctx, SCVX_ERR_ARG, "cov: null buffer");
    } else if (margins) {
        const std::string who = own->thrust ? "thrust margins: " : c.nav ? "margins from nav: " : "margins from cov: ";
        if (!c.S0) return fail(ctx, SCVX_ERR_ARG, who + "null buffer (S0)");
        if (c.nav && !c.N0) return fail(ctx, SCVX_ERR_ARG, who + "null buffer (N0)");
        if (!(own->nsigma >= 0.0) || !std::isfinite(own->nsigma)) return fail(ctx, SCVX_ERR_ARG, who + "nsigma must be finite and >= 0");
        if (!(own->cap > 0.0 && own->cap < 0.5))
            return fail(ctx, SCVX_ERR_ARG, who + (own->thrust ? "cap must lie in (0, 0.5), a fraction of Tmax - Tmin"
                                                              : "cap must lie in (0, 0.5), a fraction of the constraint's width"));
        if (own->which == 0u || (own->which & ~(unsigned)SCVX_MARGIN_ALL))
            return fail(ctx, SCVX_ERR_ARG, (c.nav ? who : std::string("margins from cov: ")) + "which must be a non-empty mask of SCVX_MARGIN_*");
    } else if (!c.S0 || (c.nav && !c.N0)) {
        return fail(ctx, SCVX_ERR_ARG, c.nav ? "nav: null buffer (S0, N0)" : "cov: null buffer");
    }
    if (c.w)
        for (int i = 0; i < 14; i++)
            if (!(c.w[i] >= 0.0) || !std::isfinite(c.w[i])) return fail(ctx, SCVX_ERR_ARG, "cov: the process noise w must be finite and >= 0");
    if (c.nav) {
        if (!own && (!c.N0 || !c.navrep)) return fail(ctx, SCVX_ERR_ARG, "nav: null buffer (N0, navrep)");
        if ((rc = check_nav_model(ctx, c.m, c.H, c.rm))) return rc;
    }
    if (c.sat) {
        if (!own && !c.satrep) return fail(ctx, SCVX_ERR_ARG, "cov clamp: null buffer (satrep)");
        if (c.band2) {
            const double lo = c.band2[0], hi = c.band2[1];
            if (!std::isfinite(lo) || hi != hi || lo < 0.0 || lo > hi)
                return fail(ctx, SCVX_ERR_ARG, "cov clamp: band2 must be (Tlo, Thi) with a finite Tlo >= 0 and Tlo <= Thi (Thi may be +inf)");
        }
    }
    if (c.need_psig && !c.psig) return fail(ctx, SCVX_ERR_ARG, c.nav ? "nav: null buffer (psig)" : "cov: null buffer (psig)");
    // the tracking weights: the margins calls refuse them before the vehicle, the batch-level analyses after it
    if (margins && (rc = check_track_weights(ctx, own->q14, own->rNU, own->qf14))) return rc;
    if (c.veh) {
        const double* sp = c.sp6;
        if (!sp) return fail(ctx, SCVX_ERR_ARG, "vehicle: null sp6");
        for (int i = 0; i < SCVX_VEH_N; i++)
            if (!(sp[i] >= 0.0) || !std::isfinite(sp[i])) return fail(ctx, SCVX_ERR_ARG, "vehicle: sp must be finite and >= 0");
        if (sp[SCVX_VEH_AERO] != 0.0 && !ctx->dyn.aero)
            return fail(ctx, SCVX_ERR_ARG, "vehicle: sp[AERO] != 0 on a model without aerodynamics");
        if (sp[SCVX_VEH_FIN] != 0.0 && !ctx->dyn.fin) return fail(ctx, SCVX_ERR_ARG, "vehicle: sp[FIN] != 0 on a model without fins");
        if (!own && !c.vtile && (sp[SCVX_VEH_ISP] != 0.0 || sp[SCVX_VEH_AERO] != 0.0))   // a batch's tiles are its own: never missing
            return fail(ctx, SCVX_ERR_ARG, "vehicle: sp[ISP] or sp[AERO] != 0 needs vtile (scvx_vehicle_tiles_f64)");
    }
    return own && !margins ? check_track_weights(ctx, own->q14, own->rNU, own->qf14) : (int)SCVX_OK;
}

CovCall stage_cov(Staging& s, const Dims& d, const CovCall& c, bool own) {
    CovCall dev = c;
    if (!own) dev.x = s.in(c.x, d.x), dev.u = s.in(c.u, d.u), dev.deriv = Tiles{s.in(c.deriv.d, d.deriv), nullptr}, dev.gain = s.in(c.gain, d.gain);
    dev.S0 = s.in(c.S0, d.c14), dev.N0 = s.in(c.N0, d.c14);
    if (!own) dev.vtile = s.in(c.vtile, d.vtile);
    dev.report = s.out_always(c.report, d.crep), dev.navrep = c.nav ? s.out_always(c.navrep, d.nrep) : nullptr;
    dev.psig = s.out(c.psig, d.psig), dev.sig = s.out(c.sig, d.sig), dev.navsig = s.out(c.navsig, d.navsig);
    dev.covK = s.out(c.covK, d.covK), dev.cov = s.out(c.cov, d.cov), dev.kf = s.out(c.m > 0 ? c.kf : nullptr, d.kf);
    dev.joint = s.out(c.joint, d.joint), dev.sens = s.out(c.sens, d.sens);
    dev.satrep = c.sat ? s.out_always(c.satrep, d.srep) : nullptr, dev.mean = s.out(c.mean, d.sig), dev.satk = s.out(c.satk, d.satk);
    return dev;
}

int cov_call_dev(scvx_ctx* ctx, const CovCall& c) {
    int rc = check_cov_call(ctx, c);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, launch_cov_call(ctx, c, ctx->stream));
    return SCVX_OK;
}

int cov_call_host(scvx_ctx* ctx, const CovCall& c, const char* entry) {
    int rc = check_cov_call(ctx, c);
    if (rc) return rc;
    const Dims d(c.B, c.K, scvx_control_dim(ctx), 0, c.m);
    Staging s(ctx);
    const CovCall dev = stage_cov(s, d, c, false);
    s.launch([&] { return launch_cov_call(ctx, dev, s.st); });
    return s.finish(entry);
}

}  // namespace scvx

extern "C" {

int scvx_cov_propagate_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                           const double* gain_dev, const double* S0_dev, const double* w14, double* report_dev, double* sig_dev,
                           double* covK_dev, double* cov_dev) {
    scvx::CovCall c = scvx::cov_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, w14, report_dev);
    c.sig = sig_dev, c.covK = covK_dev, c.cov = cov_dev;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_cov_path_sigma_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                            const double* gain_dev, const double* S0_dev, const double* w14, double* report_dev, double* psig_dev) {
    scvx::CovCall c = scvx::cov_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, w14, report_dev);
    c.psig = psig_dev, c.need_psig = true;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_cov_clamp_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                       const double* gain_dev, const double* S0_dev, const double* w14, const double* band2, double* report_dev,
                       double* satrep_dev, double* mean_dev, double* sig_dev, double* covK_dev, double* cov_dev, double* satk_dev) {
    scvx::CovCall c = scvx::cov_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, w14, report_dev);
    c.sig = sig_dev, c.covK = covK_dev, c.cov = cov_dev, c.sat = true, c.band2 = band2, c.satrep = satrep_dev, c.mean = mean_dev, c.satk = satk_dev;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_cov_clamp_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                            const double* S0, const double* w14, const double* band2, double* report, double* satrep, double* mean,
                            double* sig, double* covK, double* cov, double* satk) {
    scvx::CovCall c = scvx::cov_record(B, K, x, u, deriv, gain, S0, w14, report);
    c.sig = sig, c.covK = covK, c.cov = cov, c.sat = true, c.band2 = band2, c.satrep = satrep, c.mean = mean, c.satk = satk;
    return scvx::cov_call_host(ctx, c, "scvx_cov_clamp_f64_host");
}

int scvx_cov_vehicle_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* deriv_dev,
                         const double* gain_dev, const double* S0_dev, const double* w14, double* report_dev, double* psig_dev,
                         double* sig_dev, double* covK_dev, double* cov_dev, const double* vtile_dev, const double* sp6,
                         double* sens_dev) {
    scvx::CovCall c = scvx::cov_record(B, K, x_dev, u_dev, deriv_dev, gain_dev, S0_dev, w14, report_dev);
    c.psig = psig_dev, c.sig = sig_dev, c.covK = covK_dev, c.cov = cov_dev, c.veh = true, c.vtile = vtile_dev, c.sp6 = sp6, c.sens = sens_dev;
    return scvx::cov_call_dev(ctx, c);
}

int scvx_cov_vehicle_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                              const double* S0, const double* w14, double* report, double* psig, double* sig, double* covK, double* cov,
                              const double* vtile, const double* sp6, double* sens) {
    scvx::CovCall c = scvx::cov_record(B, K, x, u, deriv, gain, S0, w14, report);
    c.psig = psig, c.sig = sig, c.covK = covK, c.cov = cov, c.veh = true, c.vtile = vtile, c.sp6 = sp6, c.sens = sens;
    return scvx::cov_call_host(ctx, c, "scvx_cov_vehicle_f64_host");
}

int scvx_cov_path_sigma_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                                 const double* S0, const double* w14, double* report, double* psig) {
    scvx::CovCall c = scvx::cov_record(B, K, x, u, deriv, gain, S0, w14, report);
    c.psig = psig, c.need_psig = true;
    return scvx::cov_call_host(ctx, c, "scvx_cov_path_sigma_f64_host");
}

int scvx_cov_propagate_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* deriv, const double* gain,
                                const double* S0, const double* w14, double* report, double* sig, double* covK, double* cov) {
    scvx::CovCall c = scvx::cov_record(B, K, x, u, deriv, gain, S0, w14, report);
    c.sig = sig, c.covK = covK, c.cov = cov;
    return scvx::cov_call_host(ctx, c, "scvx_cov_propagate_f64_host");
}

}  // extern "C"
