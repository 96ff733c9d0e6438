// The flying kernel of the sampled closed-loop dispersion with per-flight VEHICLE ERRORS (the _veh entry points, include/scvx.h), flown on
// the true state: mc_fly_kernel (scvx_mc_fly.hpp) with ACT = true and NAV = false, 24 kernels over (model) x (PV) x (RNG), in a
// translation unit of their own so that they compile beside scvx_mc.hip's instead of behind them.
#include "scvx_mc_fly.hpp"

namespace scvx {

template SCVX_MC_FLY_ACT(false, double);

}  // namespace scvx
