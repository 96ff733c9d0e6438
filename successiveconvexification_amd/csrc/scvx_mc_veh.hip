// The flying kernel of the sampled closed-loop dispersion with per-flight VEHICLE ERRORS (the _veh entry points, include/scvx.h), flown on
// the true state: mc_fly_kernel (scvx_mc_fly.hpp) with ACT = true and NAV = false, 24 kernels over (model) x (PV) x (RNG), in a
// translation unit of their own so that they compile beside scvx_mc.hip's instead of behind them.  Also the argument checks of the
// vehicle errors, shared by the context-level and the batch-level entry points.
#include "scvx_mc_fly.hpp"

namespace scvx {

template SCVX_MC_FLY_ACT(false, double);

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

int check_mc_veh_draws(scvx_ctx* ctx, const scvx_mc_rng* rng, int noise, const void* xi0, const void* eta, const void* xin,
                       const void* nud, const void* zeta) {
    if (!ctx) return SCVX_ERR_ARG;
    if (rng) {
        if (xi0 || eta || xin || nud || zeta)
            return fail(ctx, SCVX_ERR_ARG, "vehicle: with rng the uploaded draws (xi0, eta, xin, nud, zeta) must be NULL");
    } else if (noise != 0)
        return fail(ctx, SCVX_ERR_ARG, "vehicle: noise without rng (pass eta)");
    return SCVX_OK;
}

}  // namespace scvx
