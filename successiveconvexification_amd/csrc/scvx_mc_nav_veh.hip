// The flying kernel of the sampled closed-loop dispersion with per-flight VEHICLE ERRORS flown on a navigation ESTIMATE: mc_fly_kernel
// (scvx_mc_fly.hpp) with ACT = true and NAV = true, 48 kernels over (model) x (PV) x (RNG) x (DS, the tiles' storage type), in a
// translation unit of their own: with scvx_mc_nav.hip's they are the slowest to compile, and the build compiles the two side by side.
#include "scvx_mc_fly.hpp"

namespace scvx {

template SCVX_MC_FLY_ACT(true, double);
template SCVX_MC_FLY_ACT(true, float);

}  // namespace scvx
