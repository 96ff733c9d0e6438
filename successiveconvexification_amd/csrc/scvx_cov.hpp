// One call of the first-order analyses (scvx_cov.hip, scvx_nav.hip): the record every entry point fills -- scvx_cov_*_f64[_host],
// scvx_nav_*_f64[_host], scvx_batch_[nav_]cov[_veh], scvx_batch_margins_from_* -- and the one check, staging and launch behind it.
// Not part of the ABI.  The members carry the names of include/scvx.h; what a form does not take stays nullptr / 0.
#pragma once
#include "scvx_internal.hpp"
#include "scvx_stage.hpp"

namespace scvx {

struct CovCall {
    int B = 0, K = 0;
    const double *x = nullptr, *u = nullptr;
    Tiles deriv;
    const double *gain = nullptr, *S0 = nullptr, *w = nullptr;   // w: host array of 14 or nullptr
    double *report = nullptr, *sig = nullptr, *covK = nullptr, *cov = nullptr, *psig = nullptr;
    bool need_psig = false;   // the _path_sigma forms: psig is what the call is for
    // nav: the analysis on the joint [z; eps] (nav_cov_kernel), and what it adds; H[m][14] and rm[m] are host arrays
    bool nav = false;
    const double* N0 = nullptr;
    int m = 0;
    const double *H = nullptr, *rm = nullptr;
    double *navrep = nullptr, *navsig = nullptr, *kf = nullptr, *joint = nullptr;
    // veh: a _vehicle / _veh form (the VEH instantiations); sp6: the six standard deviations (host)
    bool veh = false;
    const double *vtile = nullptr, *sp6 = nullptr;
    double* sens = nullptr;
    // sat: a _clamp form (the SAT instantiations); band2: (Tlo, Thi), a host array, or nullptr for the problem's (Tmin, Tmax)
    bool sat = false;
    const double* band2 = nullptr;
    double *satrep = nullptr, *mean = nullptr, *satk = nullptr;
};

// the record of a context-level form: what every one of them takes
inline CovCall cov_record(int B, int K, const double* x, const double* u, const double* deriv, const double* gain, const double* S0,
                          const double* w14, double* report) {
    CovCall c;
    c.B = B, c.K = K, c.x = x, c.u = u, c.deriv = Tiles{deriv, nullptr}, c.gain = gain, c.S0 = S0, c.w = w14, c.report = report;
    return c;
}

// What a batch-level form checks besides: the plan, the gains, the tiles, the vehicle tiles and the shape are the batch's own and are
// not checked, report (and navrep) are optional.  margins: the scvx_batch_margins_from_* calls, with nsigma, cap, which and refusals in
// words of their own; thrust: scvx_batch_thrust_margins_from_cov, whose refusals keep their wording.
struct CovBatch {
    const double *q14, *rNU, *qf14;
    bool margins = false, thrust = false;
    double nsigma = 0.0, cap = 0.0;
    unsigned which = 0u;
};

// every refusal of every form, in the order tests/golden/cov_refusals.txt and cov_batch_refusals.txt pin
int check_cov_call(scvx_ctx* ctx, const CovCall& c, const CovBatch* own = nullptr);
// The device record of a host record: the inputs (vtile last), then the outputs, declared on s in the order the hand-written bodies
// had.  own: a batch-level form -- x, u, deriv, gain and vtile are device arrays already and report / navrep are always allocated.
CovCall stage_cov(Staging& s, const Dims& d, const CovCall& c, bool own);
// the one launch: cov_propagate_kernel, or with nav nav_cov_kernel (launch_nav_call, scvx_nav.hip); float tiles with deriv.f
hipError_t launch_cov_call(const scvx_ctx* ctx, const CovCall& c, hipStream_t st);
hipError_t launch_nav_call(const scvx_ctx* ctx, const CovCall& c, hipStream_t st);
// the two shapes of a context-level entry point: check, launch on device arrays; check, stage, launch, finish on host arrays
int cov_call_dev(scvx_ctx* ctx, const CovCall& c);
int cov_call_host(scvx_ctx* ctx, const CovCall& c, const char* entry);

// the kernel argument of the VEH instantiations (zeros without veh: the plain instantiations do not take it)
inline CovVehK cov_veh_k(const CovCall& c) {
    CovVehK k{c.veh ? c.vtile : nullptr, c.veh ? c.sens : nullptr, {}};
    for (int i = 0; i < SCVX_VEH_N; i++) k.p[i] = c.veh ? c.sp6[i] * c.sp6[i] : 0.0;
    return k;
}

// the kernel argument of the SAT instantiations: the caller's band, or the problem's
inline CovSatK cov_sat_k(const CovCall& c, double Tmin, double Tmax) {
    return CovSatK{c.band2 ? c.band2[0] : Tmin, c.band2 ? c.band2[1] : Tmax, c.satrep, c.mean, c.satk};
}

}  // namespace scvx
