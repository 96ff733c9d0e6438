// Internal declarations shared by the translation units of libscvx_hip.so (not part of the ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <string>
#include "scvx.h"
#include "scvx_dyn.hpp"

namespace scvx { struct TdCache; }   // device tables + workspace of the 3-DoF initialiser (scvx_threedof.hip)

#define SCVX_MAX_PARTS 4   // parts a split solve_step runs as, one side stream each (scvx_batch.hip)

struct scvx_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    // Side streams of the split solve_step / reset (scvx_batch.hip): non-blocking, created on first use, destroyed with the context.
    // `epoch` counts the context-level calls that change `stream` or what a launch reads from the context (scvx_set_stream,
    // scvx_use_null_stream, scvx_set_nsub, scvx_set_aero_table): a batch that has not seen the current value forks from `stream` again.
    hipStream_t side[SCVX_MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};
    unsigned long long epoch = 0;
    scvx_problem prob{};
    scvx::DynParams dyn{};
    int nsub = 10;
    int k1_persist = -1; // persistent blocks in K1's producer/consumer kernel: -1 auto (by npts), 0 / 1 forced (SCVX_K1_PERSIST)
    int num_cus = 0;     // compute units of the device (persistent-block launch shapes)
    int k1_variant = 1;  // 0: one-lane-per-column kernel, 1: producer/consumer kernel (SCVX_K1_VARIANT overrides)
    int k1_sg = 1;       // producer/consumer pipeline per RK stage (1, default) or per substep (0); SCVX_K1_SG overrides
    double* d_cdrag = nullptr;
    double* d_clift = nullptr;
    double* d_ctrq = nullptr;   // prefiltered torque table, uploaded only with SCVX_MODEL_AERO_TORQUE
    void* comm = nullptr;   // ncclComm_t of scvx_comm_create (RCCL, bound at run time: csrc/scvx_comm.hip)
    int comm_rank = 0, comm_world = 0;
    scvx::TdCache* td = nullptr;
    double* mc_ws = nullptr;     // partial rows of scvx_track_mc_f64's reduction (scvx_mc.hip), grown on demand
    size_t mc_ws_doubles = 0;
    double* mcq_ws = nullptr;    // dense flights / pathv of a _q call that asks for their order statistics only, grown on demand
    size_t mcq_ws_doubles = 0;
    std::string err;
};

namespace scvx {

struct NcclId { char internal[SCVX_COMM_ID_BYTES]; };   // layout of ncclUniqueId (rccl.h), passed by value to RCCL

// K1: endpoint[B*K][14], deriv[B*K][14+2NU+1][14] from x[B][K+1][14], u[B][K+1][NU], sigma[B]  (NU = scvx_control_dim).
hipError_t launch_linearize(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma,
                            double dt, double* endpoint, double* deriv, hipStream_t st, const int* skip = nullptr);
// K1 in double arithmetic with the derivative tiles stored as float (scvx_batch_set_linearization_f32)
hipError_t launch_linearize_store_f32(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma,
                                      double dt, double* endpoint, float* deriv, hipStream_t st, const int* skip = nullptr);
// K2: xnext[B*K][14].
hipError_t launch_propagate(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma,
                            double dt, double* xnext, hipStream_t st);

// fp32 forms (column-per-lane kernel / one thread per segment, float arithmetic): scvx_linearize_f32, scvx_propagate_f32
hipError_t launch_linearize_f32(const scvx_ctx* ctx, int B, int K, const float* x, const float* u, const float* sigma,
                                float dt, float* endpoint, float* deriv, hipStream_t st);
hipError_t launch_propagate_f32(const scvx_ctx* ctx, int B, int K, const float* x, const float* u, const float* sigma,
                                float dt, float* xnext, hipStream_t st);

// the constants of the path functions, formed as oracle/socp.py:99-101,188 / rocketland.jl:63-65 form them (scvx_flight.hip)
struct PathK {
    double rIf[3], vIf[3], qBIf[4], wBf[3];
    double mdry, tggs, sqcm, omMax, Tmax, Tmin, inv_cosd, vmax, finmxf;
    int dp;   // SCVX_MODEL_DPMAX
};
PathK path_constants(const scvx_problem& P);

// NaN-propagating running extrema (fmax / fmin alone drop a NaN): once NaN, always NaN
__device__ __forceinline__ double nan_max(double a, double v) { return (v > a || v != v) ? v : a; }
__device__ __forceinline__ double nan_min(double a, double v) { return (v < a || v != v) ? v : a; }

// the derivative tiles of a launch that reads them in either format: double, or float as scvx_batch_set_linearization_f32 stores them;
// exactly one member is set
struct Tiles {
    const double* d = nullptr;
    const float* f = nullptr;
};

// Flight check (scvx_flight.hip): report[B][SCVX_FLIGHT_NREP], xfly[B][K+1][14] or nullptr; one lane per trajectory, dt = 1 / (K + 1).
hipError_t launch_flight(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, int nsub,
                         int mode, double* report, double* xfly, hipStream_t st);
// argument checks shared by scvx_flight_check_f64[_host] and scvx_batch_flight_check (scvx_api.hip)
int check_flight(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, int nsub, int mode, const void* report);

// Segment audit (scvx_audit.hip): seg[B][K][SCVX_SEG_N], report[B][SCVX_FLIGHT_NREP] (the PLAN-mode report, reduced from seg) or
// nullptr; one lane per (b, k), dt = 1 / (K + 1).
hipError_t launch_segment_audit(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, int nsub,
                                double* seg, double* report, hipStream_t st);
int check_segment_audit(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, int nsub, const void* seg);
// scvx_batch_audit_margins: new = min(old + gain e_k, cap width_k) into marg [B][K+1][2] (lo alone) and pmarg [B][K+1][SCVX_PMARG_N];
// capw = cap times the constant widths, the glide width is that of x [B][K+1][14]
struct AuditCaps { double thrust, tilt, rate, cap, itan; };
hipError_t launch_audit_margins(int B, int K, const double* seg, const double* x, double gain, double tol, const AuditCaps& capw,
                                unsigned which, double* marg, double* pmarg, hipStream_t st);

// Plan tracking (scvx_track.hip).  Gains: one wavefront per trajectory over the derivative tiles; gain[B][K][NU][14+NU],
// p0[B][14+NU][14+NU] or nullptr; q / r / qf are host arrays.
// Closed-loop flight (the flight check's kernel with TRACK set, scvx_flight.hip): dx0[B][14], xfly[B][K+1][14], ufly[B][K+1][NU] or nullptr.
hipError_t launch_track_gains(const scvx_ctx* ctx, int B, int K, Tiles deriv, const double* q, const double* r, const double* qf,
                              double* gain, double* p0, hipStream_t st);
hipError_t launch_track_fly(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, const double* gain,
                            const double* dx0, int nsub, int flags, double* report, double* xfly, double* ufly, hipStream_t st);
// the same with the law fed a navigation estimate: nav[B][K][14], the estimate's error at node k (never nullptr)
hipError_t launch_track_fly_nav(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma,
                                const double* gain, const double* dx0, const double* nav, int nsub, int flags, double* report,
                                double* xfly, double* ufly, hipStream_t st);
// argument checks shared by the context-level and the batch-level entry points
int check_track_weights(scvx_ctx* ctx, const double* q, const double* r, const double* qf);
int check_track_fly(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, const void* gain, int nsub, int flags,
                    const void* report);

// Sampled dispersion (scvx_mc.hip, scvx_mc_nav.hip): S flights per plan, one lane per flight, a wavefront = 64 samples of one plan.
// Every form goes through one record, one check, one staging and one launch: scvx_mc.hpp.  The partial rows live in ctx->mc_ws.
void mc_workspace_free(scvx_ctx* ctx);

// Covariance analysis (scvx_cov.hip): one wavefront per trajectory over the derivative tiles and the gains; S0[B][14][14]; w: host
// array of 14 or nullptr; report[B][SCVX_COV_NREP]; sig[B][K+1][n], covK[B][n][n], cov[B][K+1][n][n] or nullptr.  With psig
// [B][K+1][SCVX_PSIG_N] the per-node s of the five path functions are kept (scvx_cov_path_sigma_f64).
// Navigation-error covariance analysis (scvx_nav.hip): cov_propagate_kernel on the joint [z; eps], N = 14 + NU + 14.  N0[B][14][14];
// m measurements per node, H[m][14] and rm[m] host arrays (nullptr with m = 0); navrep[B][SCVX_NAV_NREP]; sig[B][K+1][n],
// navsig[B][K+1][14], kf[B][K][14][m], joint[B][K+1][N][N] or nullptr; psig as above, read off the truth block Xi_k[z,z].
// Vehicle errors in the two (include/scvx.h "consider parameters"): vtile[B][K][SCVX_VTILE_N][14] (scvx_vtile.hip) or nullptr, sp6: the
// six standard deviations (host), sens[B][K+1][n][6] or nullptr.
// Every form of both goes through one record, one check, one staging and one launch: scvx_cov.hpp.
int check_nav_model(scvx_ctx* ctx, int m, const double* H, const double* rm);   // shared with the sampled flights on an estimate

// the kernel argument of the VEH instantiations: p = sp^2 (cov_veh_k, scvx_cov.hpp)
struct CovVehK {
    const double* vtile;
    double* sens;
    double p[SCVX_VEH_N];
};
// the kernel argument of the SAT instantiations (scvx_cov_clamp_f64): the band, satrep [B][SCVX_SAT_NREP], and mean [B][K+1][n],
// satk [B][K][4] or nullptr (cov_sat_k, scvx_cov.hpp)
struct CovSatK {
    double Tlo, Thi;
    double *satrep, *mean, *satk;
};
// the one element of a VEH or SAT instantiation's trailing kernel-argument pack
template <typename T>
__device__ __forceinline__ const T& veh_first(const T& t) { return t; }
// Element (i, cI) of Gamma_k = d x_{k+1} / d theta (include/scvx.h): D the segment's tile (column-major, stride 14: A | B- | B+), uk =
// ubar_k with ubar_{k+1} behind it, vt the segment's vehicle tile [SCVX_VTILE_N][14] or nullptr.  w- / w+ are d ua / d theta at the two
// ends of the hold: THRUST u;  MIS_Y e_y x u = (u2, 0, -u0);  MIS_Z e_z x u = (-u1, u0, 0);  FIN u[3:5].
template <int NU>
__device__ __forceinline__ double veh_gamma(const double* D, const double* uk, const double* vt, int i, int cI) {
    constexpr int n = 14 + NU;
    double s = 0.0;
    if (cI == SCVX_VEH_ISP || cI == SCVX_VEH_AERO) {
        if (vt) s = vt[(cI == SCVX_VEH_ISP ? SCVX_VTILE_ISP : SCVX_VTILE_AERO) * 14 + i];
    } else if (cI == SCVX_VEH_FIN) {
        if constexpr (NU == 5) {
#pragma unroll
            for (int j = 3; j < 5; j++) s = fma(D[(14 + j) * 14 + i], uk[j], fma(D[(n + j) * 14 + i], uk[NU + j], s));
        }
    } else {
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double sy = j == 0 ? 1.0 : (j == 2 ? -1.0 : 0.0), sz = j == 0 ? -1.0 : (j == 1 ? 1.0 : 0.0);
            const int jy = j == 0 ? 2 : 0, jz = j == 0 ? 1 : 0;
            const double wm = cI == SCVX_VEH_THRUST ? uk[j] : (cI == SCVX_VEH_MIS_Y ? sy * uk[jy] : sz * uk[jz]);
            const double wp = cI == SCVX_VEH_THRUST ? uk[NU + j] : (cI == SCVX_VEH_MIS_Y ? sy * uk[NU + jy] : sz * uk[NU + jz]);
            s = fma(D[(14 + j) * 14 + i], wm, fma(D[(n + j) * 14 + i], wp, s));
        }
    }
    return s;
}
hipError_t launch_vehicle_tiles(const scvx_ctx* ctx, int B, int K, const double* x, const double* u, const double* sigma, double* vtile,
                                hipStream_t st);
int check_vehicle_tiles(scvx_ctx* ctx, int B, int K, const void* x, const void* u, const void* sigma, const void* vtile);

// K0 (scvx_threedof.hip): the batched 3-DoF landing SOCP on device arrays, enqueued on ctx->stream; sol [B][(K+1)*15+1],
// info [B][6] = status, iters, pobj, gap, pres, dres.  threedof_to_record overwrites the trajectory records [B][(K+1)*(14+NU)+1]
// of the trajectories whose solve is optimal with the LinPoints of initial_solve.jl:90-105.
int threedof_solve_dev(scvx_ctx* ctx, int B, const double* ic_dev, const scvx_threedof_opts* opts, double* sol_dev,
                       double* info_dev);
int threedof_to_record(scvx_ctx* ctx, int B, int K, const double* sol_dev, const double* info_dev, double* rec_dev, int attitude);
void td_cache_free(scvx_ctx* ctx);

inline int fail(scvx_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    return code;
}

}  // namespace scvx

#define SCVX_HIP(ctx, call)                                                                        \
    do {                                                                                           \
        hipError_t e_ = (call);                                                                    \
        if (e_ != hipSuccess)                                                                      \
            return scvx::fail((ctx), SCVX_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)
