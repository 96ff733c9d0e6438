// Vehicle tiles (scvx_vehicle_tiles_f64, include/scvx.h): the two per-segment sensitivities to the vehicle errors that the derivative
// tiles do not hold, d x_{k+1} / d theta_ISP and d x_{k+1} / d theta_AERO about the plan at theta = 0.  No counterpart in the reference.
//
// vehicle_tiles_kernel: ONE LANE PER SEGMENT, as K2's propagate_kernel -- the same RK4, first-order hold, nsub and dt = 1 / (K + 1),
// from the planned node x_k -- with the two columns integrated beside the state,
//     c' = sigma (A(t) c + phi(t)),  c(0) = 0,
// so the result is the derivative of the discrete flow itself (RK4 on the variational system is the derivative of RK4).  A(t) c is
// K1's: the lane evaluates the stage with stage_eval_publish into a record of its own in LDS (StageRec: 58 .. 100 doubles per lane, 64
// lanes: 29 .. 50 KB per block) and applies it with column_deriv_rec_pieces, the code that covers every model (exo, aero, aero + torque,
// fins, aero + fins, aero + fins + torque).  A lane reads only the record it wrote: no barrier.
//     phi_ISP  = e_0 (-alpha |uu|)                        the mass equation's own right-hand side
//     phi_AERO = F_aero / m in the v rows (+ Jinv tau_aero in the w rows with the aerodynamic torque): what scales with force_scalar
// The fin force is a control, not aerodynamics: it is not in phi_AERO.  Without aerodynamics the AERO column is written as zeros.
#include "scvx_internal.hpp"
#include "scvx_stage.hpp"

namespace scvx {

template <bool AERO, bool FIN, bool TRQ>
__global__ __launch_bounds__(64) void vehicle_tiles_kernel(DynPK<double, TRQ> p, long nseg, int K, const double* __restrict__ x,
                                                           const double* __restrict__ u, const double* __restrict__ sigma, double dt,
                                                           int nsub, double* __restrict__ vtile) {
    constexpr int NU = FIN ? 5 : 3, NR = StageRec<AERO, FIN, TRQ>::N, NCOL = AERO ? 2 : 1;
    __shared__ double recl[NR * 64];
    const int lane = threadIdx.x;
    const long gid = (long)blockIdx.x * 64 + lane;
    const bool live = gid < nseg;
    const long seg = live ? gid : nseg - 1;   // a lane past the end integrates the last segment again and writes nothing
    const long b = seg / K;
    const int k = (int)(seg - b * K);
    const double* xk = x + ((size_t)b * (K + 1) + k) * 14;
    const double* uk = u + ((size_t)b * (K + 1) + k) * NU;
    const double sig = sigma[b];
    double* rec = recl + lane;
    double xs[14], cs[NCOL][14];
#pragma unroll
    for (int i = 0; i < 14; i++) xs[i] = xk[i];
#pragma unroll
    for (int cI = 0; cI < NCOL; cI++)
#pragma unroll
        for (int i = 0; i < 14; i++) cs[cI][i] = 0.0;
    double ukv[NU], upv[NU], wc[NU];
#pragma unroll
    for (int j = 0; j < NU; j++) { ukv[j] = uk[j]; upv[j] = uk[NU + j]; wc[j] = 0.0; }
    const double h = dt / double(nsub);
    const double inv_n = 1.0 / double(nsub);
    for (int s = 0; s < nsub; s++) {
        double xa[14], xt[14], ca[NCOL][14], ct[NCOL][14];
#pragma unroll
        for (int i = 0; i < 14; i++) {
            xa[i] = xs[i];
            xt[i] = xs[i];
#pragma unroll
            for (int cI = 0; cI < NCOL; cI++) { ca[cI][i] = cs[cI][i]; ct[cI][i] = cs[cI][i]; }
        }
#pragma unroll 1   // one copy of the stage: unrolled four times the aerodynamic models spill
        for (int stg = 0; stg < 4; stg++) {
            const double lkp = (double(s) + (stg == 0 ? 0.0 : (stg == 3 ? 1.0 : 0.5))) * inv_n;
            const double lkm = 1.0 - lkp;
            double uu[NU];
#pragma unroll
            for (int j = 0; j < NU; j++) uu[j] = fma(ukv[j], lkm, upv[j] * lkp);
            double g[14];
            stage_eval_publish<AERO, FIN, TRQ>(p, xt, uu, g, rec, 64, true);
            // the forcing of the two columns at this stage's state
            double fa[3] = {0.0, 0.0, 0.0}, ta[3] = {0.0, 0.0, 0.0};
            if constexpr (AERO) {
                double C[9], F[3], tau[3] = {0.0, 0.0, 0.0};
                dcm(xt + 7, C);
                aero_force<false, double, TRQ>(p, xt + 7, xt + 4, C, F, nullptr, tau);
                const double invm = 1.0 / xt[0];
#pragma unroll
                for (int i = 0; i < 3; i++) {
                    fa[i] = F[i] * invm;
                    if constexpr (TRQ) ta[i] = p.Jinv[3 * i] * tau[0] + p.Jinv[3 * i + 1] * tau[1] + p.Jinv[3 * i + 2] * tau[2];
                }
            }
            const double wacc = h * ((stg == 0 || stg == 3) ? (1.0 / 6.0) : (1.0 / 3.0));
            const double wnext = h * (stg == 2 ? 1.0 : 0.5);
#pragma unroll
            for (int cI = 0; cI < NCOL; cI++) {
                double dc[14];
                column_deriv_rec_pieces<AERO, FIN, TRQ>(p, rec, 64, ct[cI], wc, 0.0, sig, dc);
                if (cI == 0) {
                    dc[0] = fma(sig, g[0], dc[0]);
                } else {
#pragma unroll
                    for (int i = 0; i < 3; i++) {
                        dc[4 + i] = fma(sig, fa[i], dc[4 + i]);
                        if constexpr (TRQ) dc[11 + i] = fma(sig, ta[i], dc[11 + i]);
                    }
                }
#pragma unroll
                for (int i = 0; i < 14; i++) {
                    ca[cI][i] = fma(wacc, dc[i], ca[cI][i]);
                    if (stg < 3) ct[cI][i] = fma(wnext, dc[i], cs[cI][i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 14; i++) {
                const double dx = sig * g[i];
                xa[i] = fma(wacc, dx, xa[i]);
                if (stg < 3) xt[i] = fma(wnext, dx, xs[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 14; i++) {
            xs[i] = xa[i];
#pragma unroll
            for (int cI = 0; cI < NCOL; cI++) cs[cI][i] = ca[cI][i];
        }
    }
    if (!live) return;
    double* o = vtile + (size_t)seg * SCVX_VTILE_N * 14;
#pragma unroll
    for (int i = 0; i < 14; i++) {
        o[SCVX_VTILE_ISP * 14 + i] = cs[0][i];
        o[SCVX_VTILE_AERO * 14 + i] = AERO ? cs[NCOL - 1][i] : 0.0;
    }
}

hipError_t launch_vehicle_tiles(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, double* vtile,
                                hipStream_t st) {
    const long nseg = (long)B * K;
    if (nseg == 0) return hipSuccess;
    const dim3 g((unsigned)((nseg + 63) / 64)), blk(64);
    const double dt = 1.0 / (K + 1);
    const DynP<double> dp(ctx->dyn);
#define SCVX_VTILE_LAUNCH(AERO, FIN, TRQ, P) \
    hipLaunchKernelGGL((vehicle_tiles_kernel<AERO, FIN, TRQ>), g, blk, 0, st, P, nseg, K, x, u, sigma, dt, ctx->nsub, vtile)
    if (ctx->dyn.trq) {
        const DynPT<double> dpt(ctx->dyn);
        if (ctx->dyn.fin) SCVX_VTILE_LAUNCH(true, true, true, dpt);
        else SCVX_VTILE_LAUNCH(true, false, true, dpt);
    } else if (ctx->dyn.fin) {
        if (ctx->dyn.aero) SCVX_VTILE_LAUNCH(true, true, false, dp);
        else SCVX_VTILE_LAUNCH(false, true, false, dp);
    } else if (ctx->dyn.aero) {
        SCVX_VTILE_LAUNCH(true, false, false, dp);
    } else {
        SCVX_VTILE_LAUNCH(false, false, false, dp);
    }
#undef SCVX_VTILE_LAUNCH
    return hipGetLastError();
}

// the refusals of scvx_propagate_f64
int check_vehicle_tiles(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, const void* vtile) {
    if (!ctx) return SCVX_ERR_ARG;
    if (B < 0 || K < 1) return fail(ctx, SCVX_ERR_ARG, "B >= 0 and K >= 1 required");
    if (B > 0 && (!x || !u || !sigma || !vtile)) return fail(ctx, SCVX_ERR_ARG, "null buffer");
    if (ctx->prob.aero_kind == 1 && !ctx->dyn.aero)
        return fail(ctx, SCVX_ERR_STATE, "AtmosphericData problem: call scvx_set_aero_table first");
    return SCVX_OK;
}

}  // namespace scvx

extern "C" {

int scvx_vehicle_tiles_f64(scvx_ctx* ctx, int B, int K, const double* x_dev, const double* u_dev, const double* sigma_dev,
                           double* vtile_dev) {
    int rc = scvx::check_vehicle_tiles(ctx, B, K, x_dev, u_dev, sigma_dev, vtile_dev);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_vehicle_tiles(ctx, B, K, x_dev, u_dev, sigma_dev, vtile_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_vehicle_tiles_f64_host(scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, double* vtile) {
    int rc = scvx::check_vehicle_tiles(ctx, B, K, x, u, sigma, vtile);
    if (rc) return rc;
    if (B == 0) return SCVX_OK;
    const scvx::Dims d(B, K, scvx_control_dim(ctx));
    scvx::Staging s(ctx);
    const double *dx = s.in(x, d.x), *du = s.in(u, d.u), *ds = s.in(sigma, d.b);
    double* dv = s.out(vtile, d.vtile);
    s.launch([&] { return scvx::launch_vehicle_tiles(ctx, B, K, dx, du, ds, dv, s.st); });
    return s.finish("scvx_vehicle_tiles_f64_host");
}

}  // extern "C"
