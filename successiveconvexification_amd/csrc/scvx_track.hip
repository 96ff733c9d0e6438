// Plan tracking (scvx_track_gains_f64 / scvx_track_fly_f64, include/scvx.h): the finite-horizon time-varying LQR about a batch of
// plans and the closed-loop flight under it.  No counterpart in the reference, which never flies a plan.
//
// track_gains_kernel: ONE WAVEFRONT PER TRAJECTORY, K sequential steps of the backward Riccati recursion on the first-order-hold
// model z_{k+1} = F_k z_k + G_k v_k, z = [dx; du], v = du_{k+1}, F = [[A, B-], [0, 0]], G = [B+; I] -- A, B-, B+ are the first
// 14 + 2 NU columns D of the derivative tile K1 wrote.  Only the 14 x 14 block Pxx of P_{k+1} meets the tile, so one step is
//     W = Pxx D (14 x m, m = 14 + 2 NU),  T = D' W (m x m),  Y = Pux D (NU x m)
//     H = T[B+, AB-] + Y[:, AB-],  S = R + T[B+, B+] + Y[:, B+] + Y[:, B+]' + Puu,  L = -S^-1 H,  P = Qz + T[AB-, AB-] + H' L
// with all operands in LDS (P, D, W, T, Y; H, L, S in W's space: 10.1 KB at NU = 3, 13.1 KB at NU = 5), the two 14-deep products W and T
// on the FP64 matrix pipe (or one lane per output element: SCVX_TRACK_MFMA=0), everything else one lane per element, the NU x NU
// Cholesky redundantly on the n lanes that each solve one column of L.  The tile of step k - 1 is fetched into registers (one
// contiguous run, coalesced) while step k computes and stored to LDS behind the step's last barrier.  DS is the tiles' storage
// type (double, or float with scvx_batch_set_linearization_f32: widened on load).
//
// The closed-loop flight itself is the TRACK instantiation of fly_kernel (scvx_flight.hip, launch_track_fly): the walk of the flight
// check with the feedback formed at every node.  This file keeps the gains kernel, the argument checks and the entry points.
#include <cmath>
#include <cstdlib>
#include "scvx_internal.hpp"
#include "scvx_stage.hpp"

namespace scvx {

struct TrackW {
    double q[14], r[5], qf[14];
};

typedef double v4f64 __attribute__((ext_vector_type(4)));

// One 16 x 16 tile of C = A B over 14 k-slots on the FP64 matrix pipe (4 x v_mfma_f64_16x16x4_f64; fragment maps as in scvx_socp.hpp:
// A: lane l holds A[l & 15][l >> 4], B: B[l >> 4][l & 15], C: register r of lane l is C[(l >> 4) + 4 r][l & 15]).  Operands in LDS with
// element strides; rows >= ni of A, columns >= nj of B and k >= 14 are fed zeros -- every lane reads a clamped, valid address and the
// value is masked afterwards.  C element (i, j) is stored at Cm[idx(i, j)] unless idx is negative.
template <class Idx>
__device__ __forceinline__ void track_mm16(double* Cm, Idx idx, const double* A, int sai, int sak, int ni, const double* Bm, int sbk,
                                           int sbj, int nj, int lane) {
    const int rc = lane & 15, kq = lane >> 4;
    const int ia = rc < ni ? rc : ni - 1, jb = rc < nj ? rc : nj - 1;
    v4f64 c = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const int k = 4 * s + kq, kc = k < 14 ? k : 13;
        const double a = A[ia * sai + kc * sak], b = Bm[kc * sbk + jb * sbj];
        c = __builtin_amdgcn_mfma_f64_16x16x4f64((rc < ni && k < 14) ? a : 0.0, (rc < nj && k < 14) ? b : 0.0, c, 0, 0, 0);
    }
    if (rc < nj) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int row = kq + 4 * r;
            const int at = row < ni ? idx(row, rc) : -1;
            if (at >= 0) Cm[at] = c[r];
        }
    }
}

// MF: the two 14-deep products W = Pxx D and T = D' W as 16 x 16 tiles on the matrix pipe (2 + 4 tiles) instead of one lane per element
template <typename DS, int NU, bool MF>
__global__ __launch_bounds__(64) void track_gains_kernel(TrackW w, int B, int K, const DS* __restrict__ deriv, double* __restrict__ gain,
                                                         double* __restrict__ p0) {
    constexpr int n = 14 + NU, m = 14 + 2 * NU, NC = m + 1, DSZ = 14 * NC, ND = 14 * m;
    constexpr int NPRE = (ND + 63) / 64;
    // T is kept without the block above the B+ columns (never read): rows < n with stride n, then the NU rows of B+ with stride m.
    // H, L and S are born after W's last use and live in its space.  10,064 B at NU = 3: 16 blocks per CU, so that the 32 blocks a CU gets
    // at B = 8,192 run in two rounds; 13,072 B at NU = 5.
    constexpr int NT = n * n + NU * m;
    static_assert(2 * NU * n + NU * NU <= ND, "H, L, S must fit into W");
    __shared__ double Pl[n * n], Dl[ND], Wl[ND], Yl[NU * m], Tl[NT];
    double *Hl = Wl, *Ll = Wl + NU * n, *Sl = Wl + 2 * NU * n;
    auto tidx = [](int a, int c) { return a < n ? (c < n ? a * n + c : -1) : n * n + (a - n) * m + c; };
    const int b = blockIdx.x, lane = threadIdx.x;
    if (b >= B) return;
    const DS* tiles = deriv + (size_t)b * K * DSZ;
    double* gb = gain + (size_t)b * K * NU * n;
    // P_K = diag(Qf, 0); tile K - 1
    for (int e = lane; e < n * n; e += 64) {
        const int a = e / n, c = e % n;
        Pl[e] = (a == c && a < 14) ? w.qf[a] : 0.0;
    }
    {
        const DS* t = tiles + (size_t)(K - 1) * DSZ;
        for (int e = lane; e < ND; e += 64) Dl[e] = (double)t[e];
    }
    __syncthreads();
    for (int k = K - 1; k >= 0; k--) {
        // the next step's tile, in flight while this one computes
        DS pre[NPRE];
        if (k > 0) {
            const DS* t = tiles + (size_t)(k - 1) * DSZ;
#pragma unroll
            for (int i = 0; i < NPRE; i++) {
                const int e = lane + 64 * i;
                pre[i] = e < ND ? t[e] : DS(0);
            }
        }
        // W = Pxx D (P is symmetric: P[i][l] read for P[l][i], contiguous over the lanes' l), Y = Pux D
        if (MF) {
            for (int j0 = 0; j0 < m; j0 += 16)
                track_mm16(Wl + j0 * 14, [](int i, int j) { return i + 14 * j; }, Pl, n, 1, 14, Dl + j0 * 14, 1, 14, m - j0 < 16 ? m - j0 : 16, lane);
        } else {
            for (int e = lane; e < ND; e += 64) {
                const int l = e % 14, c = e / 14;
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < 14; i++) s = fma(Pl[i * n + l], Dl[c * 14 + i], s);
                Wl[e] = s;
            }
        }
        for (int e = lane; e < NU * m; e += 64) {
            const int j = e % NU, c = e / NU;
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < 14; i++) s = fma(Pl[(14 + j) * n + i], Dl[c * 14 + i], s);
            Yl[j * m + c] = s;
        }
        __syncthreads();
        // T = D' W: the [A B-] x [A B-] block and the B+ rows (the block above the B+ columns is their transpose: not formed)
        if (MF) {
            for (int i0 = 0; i0 < m; i0 += 16)
                for (int j0 = 0; j0 < m; j0 += 16)
                    track_mm16(Tl, [=](int i, int j) { return tidx(i0 + i, j0 + j); }, Dl + i0 * 14, 14, 1, m - i0 < 16 ? m - i0 : 16,
                               Wl + j0 * 14, 1, 14, m - j0 < 16 ? m - j0 : 16, lane);
        } else {
            for (int e = lane; e < m * m; e += 64) {
                const int a = e % m, c = e / m;
                if (a < n && c >= n) continue;
                double s = 0.0;
#pragma unroll
                for (int l = 0; l < 14; l++) s = fma(Dl[a * 14 + l], Wl[c * 14 + l], s);
                Tl[tidx(a, c)] = s;
            }
        }
        __syncthreads();
        // H = G' P F (NU x n), S = R + G' P G (NU x NU, symmetrised)
        for (int e = lane; e < NU * n + NU * NU; e += 64) {
            if (e < NU * n) {
                const int j = e / n, c = e % n;
                Hl[e] = Tl[tidx(n + j, c)] + Yl[j * m + c];
            } else {
                const int j = (e - NU * n) / NU, l = (e - NU * n) % NU;
                const double s = 0.5 * (Tl[tidx(n + j, n + l)] + Tl[tidx(n + l, n + j)]) + (Yl[j * m + n + l] + Yl[l * m + n + j]) +
                                 Pl[(14 + j) * n + 14 + l];
                Sl[j * NU + l] = j == l ? s + w.r[j] : s;
            }
        }
        __syncthreads();
        // L = -S^-1 H: lane c factorises S = C C' (its own copy) and solves column c
        if (lane < n) {
            double C[NU][NU], y[NU];
#pragma unroll
            for (int j = 0; j < NU; j++) {
#pragma unroll
                for (int i = j; i < NU; i++) {
                    double s = Sl[i * NU + j];
#pragma unroll
                    for (int l = 0; l < j; l++) s = fma(-C[i][l], C[j][l], s);
                    C[i][j] = i == j ? sqrt(s) : s / C[j][j];
                }
            }
#pragma unroll
            for (int i = 0; i < NU; i++) {
                double s = Hl[i * n + lane];
#pragma unroll
                for (int l = 0; l < i; l++) s = fma(-C[i][l], y[l], s);
                y[i] = s / C[i][i];
            }
#pragma unroll
            for (int i = NU - 1; i >= 0; i--) {
                double s = y[i];
#pragma unroll
                for (int l = i + 1; l < NU; l++) s = fma(-C[l][i], y[l], s);
                y[i] = s / C[i][i];
            }
#pragma unroll
            for (int i = 0; i < NU; i++) {
                Ll[i * n + lane] = -y[i];
                gb[(size_t)k * NU * n + i * n + lane] = -y[i];
            }
        }
        __syncthreads();
        // P = Qz + F' P F + H' L, symmetrised: each element from both of its triangles
        for (int e = lane; e < n * n; e += 64) {
            const int a = e / n, c = e % n;
            double s1 = Tl[a * n + c], s2 = Tl[c * n + a];
#pragma unroll
            for (int j = 0; j < NU; j++) {
                s1 = fma(Hl[j * n + a], Ll[j * n + c], s1);
                s2 = fma(Hl[j * n + c], Ll[j * n + a], s2);
            }
            const double s = 0.5 * (s1 + s2);
            Pl[e] = (a == c && a < 14) ? s + w.q[a] : s;
        }
        if (k > 0) {
#pragma unroll
            for (int i = 0; i < NPRE; i++) {
                const int e = lane + 64 * i;
                if (e < ND) Dl[e] = (double)pre[i];
            }
        }
        __syncthreads();
    }
    if (p0) {
        double* o = p0 + (size_t)b * n * n;
        for (int e = lane; e < n * n; e += 64) o[e] = Pl[e];
    }
}

constexpr bool kTrackMfmaDefault = true;   // measured: 0.78 against 1.19 ms at B = 8,192 (exo), bit-identical gains (profiles/track.md)

template <typename DS>
static hipError_t launch_gains_t(const scvx_ctx* ctx, int B, int K, const DS* deriv, const TrackW& w, double* gain, double* p0,
                                 hipStream_t st) {
    // SCVX_TRACK_MFMA = 0 / 1 forces the lane-per-element / matrix-pipe form of the two 14-deep products (A/B: profiles/track.md)
    bool mf = kTrackMfmaDefault;
    if (const char* v = std::getenv("SCVX_TRACK_MFMA"); v && *v) mf = std::atoi(v) != 0;
    const dim3 g((unsigned)B), blk(64);
    if (ctx->dyn.fin) {
        if (mf) hipLaunchKernelGGL((track_gains_kernel<DS, 5, true>), g, blk, 0, st, w, B, K, deriv, gain, p0);
        else hipLaunchKernelGGL((track_gains_kernel<DS, 5, false>), g, blk, 0, st, w, B, K, deriv, gain, p0);
    } else {
        if (mf) hipLaunchKernelGGL((track_gains_kernel<DS, 3, true>), g, blk, 0, st, w, B, K, deriv, gain, p0);
        else hipLaunchKernelGGL((track_gains_kernel<DS, 3, false>), g, blk, 0, st, w, B, K, deriv, gain, p0);
    }
    return hipGetLastError();
}

static TrackW pack_weights(const scvx_ctx* ctx, const double* q, const double* r, const double* qf) {
    TrackW w{};
    const int NU = ctx->dyn.fin ? 5 : 3;
    for (int i = 0; i < 14; i++) { w.q[i] = q[i]; w.qf[i] = qf[i]; }
    for (int j = 0; j < NU; j++) w.r[j] = r[j];
    return w;
}

hipError_t launch_track_gains(const scvx_ctx* ctx, int B, int K, Tiles deriv, const double* q, const double* r, const double* qf,
                              double* gain, double* p0, hipStream_t st) {
    const TrackW w = pack_weights(ctx, q, r, qf);
    return deriv.d ? launch_gains_t<double>(ctx, B, K, deriv.d, w, gain, p0, st) : launch_gains_t<float>(ctx, B, K, deriv.f, w, gain, p0, st);
}

// ---------------------------------------------------------------------------------------------------------------------------------
int check_track_weights(scvx_ctx* ctx, const double* q, const double* r, const double* qf) {
    if (!ctx) return SCVX_ERR_ARG;
    if (!q || !r || !qf) return fail(ctx, SCVX_ERR_ARG, "track: null weight array (q[14], r[NU], qf[14])");
    const int NU = ctx->dyn.fin ? 5 : 3;
    for (int i = 0; i < 14; i++)
        if (!(q[i] >= 0.0) || !std::isfinite(q[i]) || !(qf[i] >= 0.0) || !std::isfinite(qf[i]))
            return fail(ctx, SCVX_ERR_ARG, "track: the weights q and qf must be finite and >= 0");
    for (int j = 0; j < NU; j++)
        if (!(r[j] > 0.0) || !std::isfinite(r[j])) return fail(ctx, SCVX_ERR_ARG, "track: the weights r must be finite and > 0");
    return SCVX_OK;
}

int check_track_gains(scvx_ctx* ctx, int B, int K, const void* deriv, const double* q, const double* r, const double* qf,
                      const void* gain) {
    if (!ctx) return SCVX_ERR_ARG;
    if (B < 1) return fail(ctx, SCVX_ERR_ARG, "track gains: B >= 1 required");
    if (K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "track gains: K must equal the problem's K");
    if (!deriv || !gain) return fail(ctx, SCVX_ERR_ARG, "track gains: null buffer");
    return check_track_weights(ctx, q, r, qf);
}

int check_track_fly(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, const void* gain, int nsub, int flags,
                    const void* report) {
    if (!ctx) return SCVX_ERR_ARG;
    if (B < 1) return fail(ctx, SCVX_ERR_ARG, "track fly: B >= 1 required");
    if (K != ctx->prob.K) return fail(ctx, SCVX_ERR_ARG, "track fly: K must equal the problem's K");
    if (nsub < 1 || nsub > 1000) return fail(ctx, SCVX_ERR_ARG, "track fly: nsub must be in [1,1000]");
    if (flags & ~SCVX_TRACK_CLAMP) return fail(ctx, SCVX_ERR_ARG, "track fly: unknown flags (SCVX_TRACK_CLAMP)");
    if (!x || !u || !sigma || !gain || !report) return fail(ctx, SCVX_ERR_ARG, "track fly: null buffer");
    if (ctx->prob.aero_kind == 1 && !ctx->dyn.aero)
        return fail(ctx, SCVX_ERR_STATE, "AtmosphericData problem: call scvx_set_aero_table first");
    return SCVX_OK;
}

}  // namespace scvx

extern "C" {

int scvx_track_gains_f64(scvx_ctx* ctx, int B, int K, const double* deriv_dev, const double* q14, const double* rNU, const double* qf14,
                         double* gain_dev, double* p0_dev) {
    int rc = scvx::check_track_gains(ctx, B, K, deriv_dev, q14, rNU, qf14, gain_dev);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_gains(ctx, B, K, scvx::Tiles{deriv_dev, nullptr}, q14, rNU, qf14, gain_dev, p0_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_track_gains_f64_host(scvx_ctx* ctx, int B, int K, const double* deriv, const double* q14, const double* rNU,
                              const double* qf14, double* gain, double* p0) {
    int rc = scvx::check_track_gains(ctx, B, K, deriv, q14, rNU, qf14, gain);
    if (rc) return rc;
    const scvx::Dims d(B, K, scvx_control_dim(ctx));
    scvx::Staging s(ctx);
    const double* dd = s.in(deriv, d.deriv);
    double *dg = s.out(gain, d.gain), *dp = s.out(p0, d.p0);
    s.launch([&] { return scvx::launch_track_gains(ctx, B, K, scvx::Tiles{dd, nullptr}, q14, rNU, qf14, dg, dp, s.st); });
    return s.finish("scvx_track_gains_f64_host");
}

int scvx_track_fly_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* sigma_dev,
                       const double* gain_dev, const double* dx0_dev, int nsub, int flags, double* report_dev, double* xfly_dev,
                       double* ufly_dev) {
    int rc = scvx::check_track_fly(ctx, B, K, x_dev, u_dev, sigma_dev, gain_dev, nsub, flags, report_dev);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_track_fly(ctx, B, K, x_dev, u_dev, sigma_dev, gain_dev, dx0_dev, nsub, flags, report_dev, xfly_dev,
                                         ufly_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_track_fly_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, const double* gain,
                            const double* dx0, int nsub, int flags, double* report, double* xfly, double* ufly) {
    int rc = scvx::check_track_fly(ctx, B, K, x, u, sigma, gain, nsub, flags, report);
    if (rc) return rc;
    const scvx::Dims d(B, K, scvx_control_dim(ctx));
    scvx::Staging s(ctx);
    const double *dx = s.in(x, d.x), *du = s.in(u, d.u), *ds = s.in(sigma, d.b), *dg = s.in(gain, d.gain), *d0 = s.in(dx0, d.b14);
    double *dr = s.out(report, d.frep), *df = s.out(xfly, d.x), *dc = s.out(ufly, d.u);
    s.launch([&] { return scvx::launch_track_fly(ctx, B, K, dx, du, ds, dg, d0, nsub, flags, dr, df, dc, s.st); });
    return s.finish("scvx_track_fly_f64_host");
}

}  // extern "C"
