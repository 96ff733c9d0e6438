/*
 * scvx.h — C ABI of the MI355X-native successive-convexification (SCvx) hot path.
 *
 * This is the drop-in boundary for the SCvx inner loop of BenChung/SuccessiveConvexification
 * (reference citations are file:line into that repository):
 *
 *   Dynamics.linearize_dynamics   dynamics.jl:321-334  ->  scvx_linearize_f64[_host]
 *   Dynamics.predict_state        dynamics.jl:315-317  ->  scvx_propagate_f64[_host]
 *   (no counterpart: open-loop flight + path audit)    ->  scvx_flight_check_f64[_host], scvx_batch_flight_check
 *   (no counterpart: LQR gains + closed-loop flight)   ->  scvx_track_gains_f64[_host], scvx_track_fly_f64[_host], scvx_batch_track_*
 *   (no counterpart: closed-loop covariance analysis)  ->  scvx_cov_propagate_f64[_host], scvx_batch_cov
 *   (no counterpart: sampled closed-loop dispersion)   ->  scvx_track_mc_f64[_host], scvx_batch_track_mc
 *   (no counterpart: its quantiles, per-node samples)   ->  scvx_order_stats_f64[_host], scvx_track_mc[_nav]_q_f64[_host], scvx_batch_track_mc[_nav]_q
 *   (no counterpart: its draws made on the device)     ->  scvx_mc_draws_f64[_host], scvx_track_mc[_nav]_rng_f64[_host], scvx_batch_track_mc[_nav]_rng
 *   (no counterpart: per-flight vehicle errors)        ->  scvx_track_mc[_nav]_veh_f64[_host], scvx_batch_track_mc[_nav]_veh
 *   Rocketland.create_initial     rocketland.jl:34-39  ->  scvx_batch_create + scvx_batch_init
 *   FirstRound.solve_initial      initial_solve.jl:17-110 -> scvx_threedof_solve, scvx_batch_init_threedof
 *   Rocketland.solve_step         rocketland.jl:226-321->  scvx_solve_step
 *   Rocketland.solve_problem      rocketland.jl:432-443->  scvx_solve
 *   MOI.optimize! (conic solve)   rocketland.jl:271    ->  scvx_socp_solve (batched interior-point, device)
 *
 * Conventions (reference: dynamics.jl:13-19, 136-139):
 *   state  x[14] = [m, r(3), v(3), q(4, scalar first), w(3)]
 *   control u[3] = thrust in the body frame
 *   augmented input inp[21] = [x; u_k; u_{k+1}; sigma]
 *   LinRes.derivative is Julia column-major 14x21: element (i,j) at j*14 + i   (master.jl:90-93)
 *
 * FIN EXTENSION (model_flags & SCVX_MODEL_FINS; BASELINE configs[4] "6-DoF + fin aero").  The reference carries the fin model
 * only as commented-out code, so the model is DEFINED BY THIS BUILD from exactly those comments: control_dim = 5,
 * u[4:5] = coordinates of the fin force along fd1 = normalize((C(q) e2) x v) and fd2 = fd1 x v (dynamics.jl:60-63), the force
 * added to the aerodynamic force (:66) and its torque cross(rFB, ff) to the body torque (:69), and the cone
 * |u[4:5]| <= finmxf at every node (rocketland.jl:203-209).  Three choices the comments leave open, stated so that configs[4]
 * numbers are not read as matching a reference model that does not exist:
 *   (1) the commented expression at dynamics.jl:69 is `cross(info.rFB, ff) + bdy_trq`; the fin flag enables Jinv * (rFB x ff); the
 *       aerodynamic body torque bdy_trq is the separate opt-in SCVX_MODEL_AERO_TORQUE below (default: dropped, as in the live
 *       model, dynamics.jl:69,93), and the two combine freely;
 *   (2) rFB is a body-frame arm and ff = u4 fd1 + u5 fd2 is built from inertial-frame vectors: the cross product mixes the two
 *       frames as the comment does -- kept as written, not "fixed";
 *   (3) the linearised thrust lower bound (rocketland.jl:199-201) uses |u[1:3]|, the thrust part of the control; the reference's
 *       `norm(iterAbout[n].control)` would be the norm of all five components once the control had five.
 * Every array below then uses NU = 5:
 *   u [B][K+1][5], inp[25], derivative 14x25 ([A | B- (5) | B+ (5) | Sigma]), trajectory record [(K+1)*19 + 1].
 * scvx_control_dim(ctx) returns NU.
 *
 * All pointers named *_dev are device (HBM) pointers valid on the context's device; all others are
 * host pointers.  Device entry points are asynchronous on the context's stream (scvx_set_stream):
 * work ordered after a call on that stream sees the call's results.  scvx_solve_step[_async] and
 * scvx_batch_reset of a large batch run as two contiguous parts on side streams that the context owns
 * and make the context's stream wait for them on the device, so that statement holds for them too; a
 * part waits for the context's stream only when another call has touched the batch or the stream
 * since its last step (after scvx_batch_trajectory_dev: at every step).  SCVX_STEP_SPLIT=1 in the
 * environment keeps every step on the context's stream; results are the same bit for bit;
 * the *_host entry points copy in, run, copy out and synchronise.  Every function returns 0 on
 * success and a negative code on failure; scvx_last_error(ctx) then describes the failure.
 * No C++ types and no exceptions cross this boundary.
 */
#ifndef SCVX_H
#define SCVX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SCVX_NX 14
#define SCVX_NU 3
#define SCVX_NP 21 /* 14 + 3 + 3 + 1 */
#define SCVX_NU_FINS 5
#define SCVX_NP_FINS 25 /* 14 + 5 + 5 + 1 */

#define SCVX_OK 0
#define SCVX_ERR_ARG -1
#define SCVX_ERR_HIP -2
#define SCVX_ERR_STATE -3
#define SCVX_ERR_NOMEM -4
#define SCVX_ERR_COMM -5 /* RCCL missing or a collective failed */

/* per-trajectory status codes written by scvx_solve_step / scvx_solve */
#define SCVX_ST_CONVERGED 0   /* ||nu|| <= nuTol and dJ <= delTol             (rocketland.jl:436) */
#define SCVX_ST_RUNNING 1     /* accepted step, not yet converged / imax hit                      */
#define SCVX_ST_REJECTED 2    /* rho < rh0: iterate kept, radius shrunk, dJ=Inf (rocketland.jl:299-301) */
#define SCVX_ST_SOLVER 3      /* conic solver did not reach tolerance        (rocketland.jl:273-276) */
#define SCVX_ST_NONFINITE 4   /* NaN/Inf encountered                                              */
#define SCVX_ST_INFEASIBLE 5  /* the subproblem has no feasible point: a boundary value violates a path cone (solver status 5) */

/* model_flags: enforce the dynamic-pressure limit 1/2 rho |v_k|^2 <= dpMax at nodes 1..K as the second-order cone
 * |v_k| <= sqrt(2 dpMax / rho) (fields master.jl:27,30; the constraint is a "todo" at rocketland.jl:211-212).  The
 * initial velocity must satisfy it. */
#define SCVX_MODEL_DPMAX 1
/* model_flags: the fin extension described at the top of this file (control_dim = 5).  Needs finmxf > 0. */
#define SCVX_MODEL_FINS 2
/* model_flags: the aerodynamic body torque.  The reference loads a torque table next to drag and lift (aerodynamics.jl:17-21), its
 * symbolic aero_force returns the torque bdy_trq (aerodynamics.jl:60-77), and dx_static comments it out (dynamics.jl:69, 93-94).
 * With this bit the rate equation becomes
 *     wdot = Jinv (rTB x u [+ rFB x ff with FINS] + tau_aero - w x J w),
 *     tau_aero = T(c, M) * length_scalar * force_scalar * (v x bv),   bv = C(q) e1,
 * where c = clamp(bv.v / (M sos), -1, 1) (0 at M <= 0) and M = |v| / sos are the arguments of the drag and lift tables and T is the
 * torque table under the same cubic B-spline, axes and Flat() extrapolation.  Three properties of the model, kept as written:
 *   (1) the direction is NOT normalised: the symbolic aero_force returns trq * ifnz.(trqd / |trqd|, trqd) and ifnz(val, nz) = nz, so
 *       each component is (v x bv)_i (aerodynamics.jl:67-68,76; its Jacobian rule (0, 1), dynamics.jl:205-207, makes the reference's
 *       derivative that of T (v x bv)).  The numeric aero_force (:38-57, normalised, drag-only at |cos| >= 0.95) is never evaluated by
 *       the loop; the host mirror aerodynamics.aero_force keeps that numeric form.  The term is smooth and vanishes at v || bv and v = 0;
 *   (2) v x bv is an inertial-frame vector added to the body-frame torque sum, as the comment at dynamics.jl:69 does (the same frame
 *       mix as fin choice (2));
 *   (3) rTB and rFB lie on the body x axis, so no control produces a body-x torque: the x component of tau_aero is absorbed by the
 *       virtual control nu.  On the sample problem the term is a small perturbation (|Jinv tau| <~ 0.05 about roll, <~ 2e-3 about
 *       pitch and yaw, against up to 3.3 from the thrust).
 * Valid only with aero_kind == 1 (scvx_ctx_create returns SCVX_ERR_ARG otherwise, and for any model_flags bit outside
 * DPMAX | FINS | AERO_TORQUE); scvx_set_aero_table then needs trq != NULL.  Bit clear: today's model, bit for bit. */
#define SCVX_MODEL_AERO_TORQUE 4

/* Flat image of DescentProblem (master.jl:17-71) + the aero scalars of AtmosphericData (master.jl:10-16).
 * Angles in degrees exactly as the reference stores them.  jB is column-major 3x3. */
typedef struct scvx_problem {
    double g, mdry, mwet, Tmin, Tmax;
    double deltaMax, thetaMax, gammaGs, omMax, dpMax;
    double jB[9];
    double alpha, rho, sos;
    double rTB[3], rFB[3];
    double rIi[3], rIf[3], vIi[3], vIf[3];
    double qBIi[4], qBIf[4];
    double wBi[3], wBf[3];
    double wNu, wID, wDS, wCst, wTviol, nuTol, delTol, tf_guess;
    double ri, rh0, rh1, rh2, alph, bet;
    double force_scalar, length_scalar; /* AtmosphericData scalars; ignored when aero_kind == 0 */
    double finmxf; /* fin extension: bound of |u[4:5]| (rocketland.jl:205 pins it to 0.01 in the commented code); read only with SCVX_MODEL_FINS */
    int32_t K, imax;
    int32_t aero_kind; /* 0 = ExoatmosphericData, 1 = AtmosphericData */
    int32_t model_flags; /* SCVX_MODEL_* bits: model terms and constraints the reference sketches but never wired up; 0 = the reference's model */
} scvx_problem;

/* Tunables of the batched conic solver that replaces MOI.optimize! (rocketland.jl:271): a structure-
 * exploiting primal-dual interior-point method (the algorithm class of the reference's Mosek / ECOS),
 * one wavefront per trajectory.  DESIGN.md explains why it is not the first-order splitting first planned. */
typedef struct scvx_solver_opts {
    int32_t max_iter;  /* interior-point iteration cap per SOCP (default 60)                                   */
    int32_t refine;    /* iterative-refinement passes per Newton solve, at most (default 6; a pass is skipped  */
                       /* when the solve's residual is already below a tenth of the dual tolerance)            */
    double tol;        /* primal / dual residual and relative-gap tolerance (default 1e-8)                     */
    double accept_tol; /* a solve that stops on its numerical floor with tol <= merit < accept_tol is reported */
                       /* as solver status 4 "almost optimal" and still feeds the trust-region test (MOI's     */
                       /* ALMOST_OPTIMAL band).  DEFAULT = tol (1e-8): the reference errors on anything but     */
                       /* OPTIMAL (rocketland.jl:273-276), so such solves become SCVX_ST_SOLVER; a wider band   */
                       /* (e.g. 1e-6) is opt-in.                                                                */
    int32_t reuse_inactive_tr; /* 0 (default): every solve_step solves its subproblem, as the reference does.  1: after a   */
                       /* REJECTED step (same about / dynam, radius halved, rocketland.jl:299-301) the conic solve is skipped  */
                       /* when the optimum just found lies strictly inside the new radius -- the radius row is then inactive  */
                       /* and that optimum is provably the new subproblem's optimum too.  The SCvx iterates are unchanged;   */
                       /* on the sample problems ~6 of the 14 solves of a solve_problem are such repeats.                    */
    int32_t warm_start;        /* 1 (default): the solve that follows a REJECTED step (same about / dynam, radius halved,  */
                       /* rocketland.jl:299-301) starts from the optimum the previous solve returned, as long as that point */
                       /* lies inside the new radius: the residuals of the NEW subproblem are evaluated there and the solve */
                       /* returns at once when they meet `tol` (1 iteration, no factorisation), else it iterates on from    */
                       /* there; every solve still ends at `tol`.  0: every solve starts cold, like the reference's.        */
    int32_t retries;           /* default 5, at most 7.  A solve that ends on its numerical floor above `tol` is run again from the   */
                       /* cold start with another step rule (step fraction, centring exponent, starting shift, centring    */
                       /* floor), at most this many times, before the trajectory is frozen as SCVX_ST_SOLVER: such failures */
                       /* sit at the precision floor of the Newton system and move with the path taken.  0: one attempt.    */
                       /* The iteration count reported for a solve is the sum over its attempts.                            */
    int32_t reserved0;         /* must be 0: scvx_batch_set_solver returns SCVX_ERR_ARG otherwise (a struct from before `retries` ends here) */
} scvx_solver_opts;

/* ---- ABI guard ----------------------------------------------------------------------------- */
/* scvx_problem, scvx_solver_opts and scvx_threedof_opts carry no size member: a binding written against another revision of
 * this header would hand over a struct of another layout and nothing would fail.  SCVX_ABI_VERSION is raised with every change
 * of a struct layout or of a signature below; scvx_abi_version() returns the value the LIBRARY was compiled with and
 * scvx_abi_struct_sizes() the sizeof of the three structs as the library sees them, in that order.  A binding compares both
 * with its own image before its first call (Python: _lib.lib(); Julia: ScvxAMD.check_abi(); C: tests/abi_harness.c).
 * Neither function touches the device. */
#define SCVX_ABI_VERSION 4
int scvx_abi_version(void);
int scvx_abi_struct_sizes(int32_t out[3]);

typedef struct scvx_ctx scvx_ctx;     /* owns device, stream, problem constants, aero tables */
typedef struct scvx_batch scvx_batch; /* owns the batched iterate (ProblemIteration x B)     */

/* ---- context ------------------------------------------------------------------------------- */
int scvx_ctx_create(const scvx_problem *p, int device, scvx_ctx **out);
void scvx_ctx_destroy(scvx_ctx *ctx);
const char *scvx_last_error(const scvx_ctx *ctx);
/* control_dim of the context's model: 3, or 5 with SCVX_MODEL_FINS.  Sizes every u / derivative / trajectory array. */
int scvx_control_dim(const scvx_ctx *ctx);
/* Stream every kernel and copy of the context is enqueued on.  NULL selects the context's OWN stream (created
 * hipStreamNonBlocking: it does not synchronise with HIP's default stream) -- a caller that produces or consumes
 * device buffers on another stream orders against it with scvx_get_stream + events, or scvx_synchronize.
 * scvx_use_null_stream selects HIP's legacy default stream (handle 0) itself. */
int scvx_set_stream(scvx_ctx *ctx, void *hip_stream);
int scvx_use_null_stream(scvx_ctx *ctx);
int scvx_get_stream(const scvx_ctx *ctx, void **hip_stream); /* the effective stream (never "NULL = own") */
int scvx_synchronize(scvx_ctx *ctx);
/* RK4 substeps per segment: the `npts` keyword of Dynamics.rk4 (dynamics.jl:112, default 10). */
int scvx_set_nsub(scvx_ctx *ctx, int nsub);
int scvx_get_nsub(const scvx_ctx *ctx);
/* Aerodynamics.load_aerodata tables (aerodynamics.jl:11-28): three n_aoa x n_mach grids, cos(AoA)
 * fastest, on axes aoa0 + i*daoa, mach0 + j*dmach.  Host pointers; prefiltered on the host, uploaded.  trq is read only with
 * SCVX_MODEL_AERO_TORQUE (then it must not be NULL); otherwise it may be NULL. */
int scvx_set_aero_table(scvx_ctx *ctx, const double *drag, const double *lift, const double *trq,
                        int n_aoa, int n_mach, double aoa0, double daoa, double mach0, double dmach);

/* ---- discretisation: Dynamics.linearize_dynamics / predict_state ---------------------------- */
/* x [B][K+1][14], u [B][K+1][NU], sigma [B]; endpoint [B][K][14]; deriv [B][K][14+2NU+1][14]  (NU = scvx_control_dim). */
int scvx_linearize_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev,
                       const double *sigma_dev, double dt, double *endpoint_dev, double *deriv_dev);
int scvx_linearize_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u,
                            const double *sigma, double dt, double *endpoint, double *deriv);
/* xnext [B][K][14]: state at the end of each segment started from node k with FOH (u_k,u_{k+1}). */
int scvx_propagate_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev,
                       const double *sigma_dev, double dt, double *xnext_dev);
int scvx_propagate_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u,
                            const double *sigma, double dt, double *xnext);

/* ---- flight check: open-loop rollout of a plan and audit of its path constraints between the nodes ----------------
 * scvx_solve imposes every path constraint of build_model (rocketland.jl:136-209) AT THE NODES only, and its dynamic-feasibility
 * evidence is the virtual control.  This call flies a plan (x, u, sigma) with the integrator of scvx_propagate_f64 (RK4,
 * first-order-hold control, `nsub` substeps per segment -- an argument of the call, independent of scvx_set_nsub, so a plan made
 * with 10 substeps can be flown with 40) and reports, per trajectory, SCVX_FLIGHT_NREP doubles:
 *   SCVX_FLIGHT_SHOOT  single shooting: the end of segment k starts segment k+1 -- the flight of the plan from x[0];
 *   SCVX_FLIGHT_PLAN   the state restarts at the planned x[k] at every node -- the plan itself, audited between its nodes; its
 *                      GAP is the largest scvx_propagate_f64 defect.
 * The path functions are evaluated at the nsub + 1 substep boundaries s = 0..nsub of every segment (control
 * u_k (1 - s/nsub) + u_{k+1} s/nsub; RK stage points are not sampled) and the report keeps their maxima over all samples from
 * node 0 to node K (the SOCP leaves node 0 or node K out of some rows; the report does not).  g <= 0 means satisfied; the
 * problem's own normalised units; state constraints on the FLOWN state.  A non-finite state makes the trajectory's GAP, MISS_*,
 * state G_* and QNORM NaN; it cannot disturb another trajectory.
 * G_TMIN > 0 between two nodes that sit on the bound with different thrust directions belongs to the reference's formulation
 * (the non-convex lower bound is linearised at the nodes, rocketland.jl:199-201, and the control is a first-order hold whose
 * chord passes inside the sphere), not to the solver. */
#define SCVX_FLIGHT_SHOOT 0
#define SCVX_FLIGHT_PLAN 1
#define SCVX_FLIGHT_NREP 16
#define SCVX_FLIGHT_GAP 0       /* max over nodes k = 1..K of |x_fly[k] - x[k]|_inf                                  */
#define SCVX_FLIGHT_MISS_R 1    /* |r - rIf|_2 at the flown final node                                              */
#define SCVX_FLIGHT_MISS_V 2    /* |v - vIf|_2                                                                      */
#define SCVX_FLIGHT_MISS_Q 3    /* |q - qBIf|_2                                                                     */
#define SCVX_FLIGHT_MISS_W 4    /* |w - wBf|_2                                                                      */
#define SCVX_FLIGHT_MASS_END 5  /* flown final mass                                                                 */
#define SCVX_FLIGHT_G_MASS 6    /* max of mdry - m                                             (rocketland.jl:137) */
#define SCVX_FLIGHT_G_GLIDE 7   /* max of tan(gammaGs) |r[2:3]| - r[1]                                  (:142-148) */
#define SCVX_FLIGHT_G_TILT 8    /* max of |q[3:4]| - sqrt((1 - cos thetaMax) / 2)                       (:155-160) */
#define SCVX_FLIGHT_G_RATE 9    /* max of |w| - omMax                                                   (:163-167) */
#define SCVX_FLIGHT_G_TMAX 10   /* max of |u[1:3]| - Tmax                                                   (:186) */
#define SCVX_FLIGHT_G_TMIN 11   /* max of Tmin - |u[1:3]|: the true bound, not its linearisation        (:199-201) */
#define SCVX_FLIGHT_G_GIMBAL 12 /* max of |u[1:3]| - u[1] / cos deltaMax                                    (:188) */
#define SCVX_FLIGHT_G_DP 13     /* max of |v| - sqrt(2 dpMax / rho) with SCVX_MODEL_DPMAX, else -inf               */
#define SCVX_FLIGHT_G_FIN 14    /* max of |u[4:5]| - finmxf with SCVX_MODEL_FINS, else -inf                        */
#define SCVX_FLIGHT_QNORM 15    /* max of | |q| - 1 |                                                               */
/* x [B][K+1][14], u [B][K+1][NU], sigma [B]; report [B][SCVX_FLIGHT_NREP]; xfly [B][K+1][14] = the flown node states
 * (xfly[.][0] = x[.][0]), or NULL.  dt = 1 / (K + 1); K must equal the problem's.  Asynchronous on the context's stream.
 * SCVX_ERR_ARG for nsub outside [1, 1000], an unknown mode, B < 1, K != the problem's K, a null x / u / sigma / report. */
int scvx_flight_check_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *sigma_dev,
                          int nsub, int mode, double *report_dev, double *xfly_dev);
int scvx_flight_check_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *sigma,
                               int nsub, int mode, double *report, double *xfly);

/* ---- plan tracking: time-varying LQR gains about a plan and the closed-loop flight under them ----------------------
 * The flight check flies a plan from exactly its own x[0].  These two calls answer what happens when the vehicle is NOT there.
 * Notation: NU = scvx_control_dim, n = 14 + NU, dx_k = x_k - xbar_k, du_k = u_k - ubar_k (bars: the plan), sigma held.  The
 * derivative tile of segment k, column-major 14 x (14 + 2 NU + 1) = [A_k | B-_k | B+_k | Sigma_k], gives
 *     dx_{k+1} = A_k dx_k + B-_k du_k + B+_k du_{k+1}.
 * The control is a first-order hold, so the decision at node k is the NEXT node's control: with z_k = [dx_k; du_k] and
 * v_k = du_{k+1},  z_{k+1} = F_k z_k + G_k v_k,  F_k = [[A_k, B-_k], [0, 0]],  G_k = [B+_k; I].  Cost, diagonal weights
 * q[14] >= 0, r[NU] > 0, qf[14] >= 0 in the problem's normalised units:
 *     J = sum_{k=0}^{K-1} (dx_k' Q dx_k + v_k' R v_k) + dx_K' Qf dx_K.
 * Backward recursion from P_K = diag(Qf, 0), Qz = diag(Q, 0), k = K-1 .. 0:
 *     S_k = R + G_k' P_{k+1} G_k,  H_k = G_k' P_{k+1} F_k,  L_k = -S_k^-1 H_k (Cholesky),
 *     P_k = Qz + F_k' P_{k+1} F_k + H_k' L_k, symmetrised.
 * Feedback: u_{k+1} = ubar_{k+1} + L_k [x_k - xbar_k; u_k - ubar_k], u_0 = ubar_0; z_0' P_0 z_0 is the predicted cost of an
 * initial deviation.  The weights are the caller's choice (the quaternion and mass directions are nearly uncontrollable).
 *
 * gain [B][K][NU][14+NU] row-major: du_{k+1}[j] = sum_i gain[b][k][j][i] * z_k[i];  p0 [B][14+NU][14+NU] or NULL.
 * deriv [B][K][14+2NU+1][14] as scvx_linearize_f64 writes it.  q14 / rNU / qf14 are HOST arrays in both forms.  The _f64 form
 * is asynchronous on the context's stream.  SCVX_ERR_ARG for any r[j] <= 0, a negative or non-finite weight, B < 1,
 * K != the problem's K, a null deriv / weight / gain. */
int scvx_track_gains_f64(scvx_ctx *ctx, int B, int K, const double *deriv_dev, const double *q14, const double *rNU,
                         const double *qf14, double *gain_dev, double *p0_dev);
int scvx_track_gains_f64_host(scvx_ctx *ctx, int B, int K, const double *deriv, const double *q14, const double *rNU,
                              const double *qf14, double *gain, double *p0);
/* Closed-loop flight: x_fly[0] = xbar_0 + dx0, u_fly[0] = ubar_0; at every node k = 0..K-1 the feedback above forms
 * u_fly[k+1] from the flown state and the applied control, then segment k is integrated from x_fly[k] under the hold
 * (u_fly[k], u_fly[k+1]) with the arithmetic of the flight check.  The report is the flight check's, column for column
 * (SCVX_FLIGHT_*): samples at every substep boundary, GAP = max over nodes 1..K of |x_fly - xbar|_inf, G_* on the flown
 * state and the APPLIED control.  All-zero gains, dx0 = NULL, flags = 0 is the SCVX_FLIGHT_SHOOT flight check.
 * flags: SCVX_TRACK_CLAMP rescales, after the feedback, the thrust part u[1:3] of the new node control (direction kept) so
 * that its norm lies in [Tmin, Tmax], and with SCVX_MODEL_FINS u[4:5] so that its norm is at most finmxf.  The gimbal cone is
 * not projected (G_GIMBAL reports it).  Without the flag the commanded control is applied as it is and G_TMAX / G_TMIN show
 * what the law asked for.
 * dx0 [B][14] or NULL (= 0); report [B][SCVX_FLIGHT_NREP]; xfly [B][K+1][14] or NULL; ufly [B][K+1][NU] or NULL.
 * SCVX_ERR_ARG for nsub outside [1, 1000], unknown flag bits, B < 1, K != the problem's K, a null x / u / sigma / gain / report. */
#define SCVX_TRACK_CLAMP 1
int scvx_track_fly_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *sigma_dev,
                       const double *gain_dev, const double *dx0_dev, int nsub, int flags, double *report_dev,
                       double *xfly_dev, double *ufly_dev);
int scvx_track_fly_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *sigma,
                            const double *gain, const double *dx0, int nsub, int flags, double *report, double *xfly,
                            double *ufly);

/* ---- covariance analysis: the closed-loop dispersion of a tracked plan, to first order --------------------------------
 * scvx_track_fly_f64 flies ONE displaced start per trajectory.  This call answers the statistical question -- given a handover
 * dispersion, how large is the landing dispersion and how much thrust headroom does the tracking law need -- for every plan of a
 * batch in one forward pass over the derivative tiles and the gains, without sampling.  Notation as above: NU = scvx_control_dim,
 * n = 14 + NU, Sigma_k (n x n) the covariance of z_k = [x_k - xbar_k; u_k - ubar_k] under the law
 * u_{k+1} = ubar_{k+1} + L_k z_k, u_0 = ubar_0 (exactly scvx_track_fly_f64 without SCVX_TRACK_CLAMP):
 *     Sigma_0     = blockdiag(S0, 0)                        S0 [14][14] symmetric positive semi-definite, per trajectory
 *     M_k         = F_k + G_k L_k                           (rows 14.. of M_k are L_k itself)
 *     Sigma_{k+1} = M_k Sigma_k M_k' + blockdiag(diag(w), 0)   w [14] >= 0: process-noise variance added per segment (NULL = 0)
 * symmetrised every step: Sigma_{k+1} = (T + T') / 2 with T the product as computed, each element from both of its triangles.  Only
 * the symmetric part (S0 + S0') / 2 of S0 is used; that it is positive semi-definite is the caller's responsibility.
 * Limits: the analysis is FIRST ORDER (linear about the plan: the derivative tiles and the gains); the covariances live at the
 * nodes; the clamp is not modelled (N_TMIN / N_TMAX say how far the law is from needing it); w is a crude per-segment lump, not a
 * continuous-time noise model; the 14 state coordinates are taken as they are -- the quaternion's norm direction is a coordinate
 * like any other, as in a start x[0] + dx0.  Gimbal, dynamic-pressure and fin margins are not reported.
 *
 * The dispersion report, SCVX_COV_NREP doubles per trajectory (state indices: 0 mass, 1 altitude -- the glide-slope row --, 2 and 3
 * the horizontal plane): */
#define SCVX_COV_NREP 16
#define SCVX_COV_SIG_M 0      /* sqrt(Sigma_K[0][0]): 1 sigma of the final mass                                            */
#define SCVX_COV_SIG_R 1      /* sqrt(trace of the r block of Sigma_K): the 1 sigma counterpart of SCVX_FLIGHT_MISS_R      */
#define SCVX_COV_SIG_V 2      /* the same for v                                                                            */
#define SCVX_COV_SIG_Q 3      /* the same for q                                                                            */
#define SCVX_COV_SIG_W 4      /* the same for w                                                                            */
#define SCVX_COV_ELL_A 5      /* 1 sigma landing ellipse in the horizontal plane: sqrt of the larger eigenvalue of the 2 x 2 */
#define SCVX_COV_ELL_B 6      /* block of Sigma_K at state indices 2, 3 (closed form); sqrt of the smaller one;              */
#define SCVX_COV_ELL_ANG 7    /* angle of the major axis from the index-2 axis, in (-pi/2, pi/2]                            */
#define SCVX_COV_SIG_PEAK 8   /* max over nodes 0..K of sqrt(trace Sigma_k[0:14][0:14])                                     */
#define SCVX_COV_S_THRUST 9   /* max over nodes 1..K of s_T = sqrt(e' Sigma_k[uu] e), e = ubar_k[1:3] / |ubar_k[1:3]|: one  */
                              /* standard deviation of the commanded thrust norm, to first order (a node with |ubar| = 0 is skipped) */
#define SCVX_COV_N_MASS 10    /* margins in standard deviations to the path functions of SCVX_FLIGHT_G_MASS .. G_TMIN (same  */
#define SCVX_COV_N_GLIDE 11   /* constants, same g <= 0 convention): with c the gradient of g in z at the planned node and   */
#define SCVX_COV_N_TILT 12    /* s = sqrt(c' Sigma_k c),  N = min over nodes k = 1..K of -g(xbar_k, ubar_k) / s.  A node where */
#define SCVX_COV_N_RATE 13    /* the gradient is undefined (a norm that is exactly 0, e.g. the glide slope at the landing     */
#define SCVX_COV_N_TMAX 14    /* point) or where s == 0 is skipped; +inf when every node is skipped; negative when the plan   */
#define SCVX_COV_N_TMIN 15    /* itself violates.                                                                            */
/* x [B][K+1][14], u [B][K+1][NU] the plan; deriv [B][K][14+2NU+1][14] as scvx_linearize_f64 writes it; gain [B][K][NU][14+NU] as
 * scvx_track_gains_f64 writes it; S0 [B][14][14]; w14 a HOST array or NULL in both forms; report [B][SCVX_COV_NREP].  Optional dense
 * outputs (NULL = not wanted): sig [B][K+1][14+NU] = sqrt(diag Sigma_k), the 1 sigma corridor about the plan; covK [B][n][n] =
 * Sigma_K; cov [B][K+1][n][n] = every Sigma_k.  A non-finite tile, gain or S0 entry makes every column of its own trajectory's
 * report NaN (a non-finite plan value: the columns that read it) and cannot disturb another trajectory.  The _f64 form is
 * asynchronous on the context's stream.  SCVX_ERR_ARG for B < 1, K != the problem's K, a null x / u / deriv / gain / S0 / report,
 * a negative or non-finite w. */
int scvx_cov_propagate_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                           const double *gain_dev, const double *S0_dev, const double *w14, double *report_dev, double *sig_dev,
                           double *covK_dev, double *cov_dev);
int scvx_cov_propagate_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv,
                                const double *gain, const double *S0, const double *w14, double *report, double *sig,
                                double *covK, double *cov);
/* The same launch, keeping what the margins are made of: psig [B][K+1][SCVX_PSIG_N] = s = sqrt(c' Sigma_k c) of the path functions
 * of N_MASS, N_GLIDE, N_TILT, N_RATE and of the thrust norm (N_TMAX and N_TMIN share it: s_T of SCVX_COV_S_THRUST) at every node.
 * Node 0 is 0 and so is a node that the margin skips (undefined gradient).  A non-finite tile, gain or S0 entry makes every row of
 * its own trajectory NaN.  Arguments up to report as scvx_cov_propagate_f64, whose outputs this call leaves bitwise unchanged;
 * SCVX_ERR_ARG also for a null psig. */
#define SCVX_PSIG_N 5
#define SCVX_PSIG_MASS 0
#define SCVX_PSIG_GLIDE 1
#define SCVX_PSIG_TILT 2
#define SCVX_PSIG_RATE 3
#define SCVX_PSIG_THRUST 4
int scvx_cov_path_sigma_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                            const double *gain_dev, const double *S0_dev, const double *w14, double *report_dev, double *psig_dev);
int scvx_cov_path_sigma_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv,
                                 const double *gain, const double *S0, const double *w14, double *report, double *psig);

/* ---- navigation-error (LQG) covariance analysis: the closed loop flown on an ESTIMATE, to first order -----------------------
 * Everything above feeds the tracking law the true state.  A vehicle feeds it a navigation estimate xhat_k whose error is correlated
 * from node to node, is corrected by measurements and is driven by the same disturbances that move the truth; the lump w of
 * scvx_cov_propagate_f64 cannot express that.  This call propagates the joint covariance of truth dispersion and navigation error.
 * Notation as above (NU, n = 14 + NU, z_k, F_k, G_k, L_k, M_k = F_k + G_k L_k; A_k = the first 14 columns of the tile), and
 *     eps_k  = x_k - xhat_k (14)       the navigation error BEFORE the measurement at node k
 *     zeta_k = [z_k; eps_k]            of size N = n + 14 (31, or 33 with fins)
 *     Xi_k   = Cov(zeta_k),  Xi_0 = blockdiag(S0, 0_NU, N0): truth dispersion and navigation error independent at the handover
 *     y_k    = H x_k + v_k             the measurement at nodes k = 0..K-1:  H [m][14], 0 <= m <= 14, Cov v = diag(rm), rm > 0;
 *                                      H and rm are HOST arrays shared by the batch; m = 0 (H, rm NULL): inertial propagation only
 * Per node k = 0..K-1:
 *   1. update (skipped when m = 0):  P = Xi[eps eps],  S = H P H' + diag(rm),  Kf = P H' S^-1 (Cholesky of S),  J = I - Kf H,
 *          Xi+ = U Xi U' + blockdiag(0_n, Kf diag(rm) Kf'),  U = blockdiag(I_n, J)        (the Joseph form: the short form
 *          (I - Kf H) P loses positivity)
 *   2. law:  u_{k+1} = ubar_{k+1} + L_k [(x_k - eps+_k) - xbar_k; u_k - ubar_k]        -- the law is fed the UPDATED estimate
 *   3. time step:  Xi_{k+1} = T_k Xi+ T_k' + W,   T_k = [[M_k, -G_k L_k[:, 0:14]], [0, A_k]],   W = diag(w) in all four of the
 *          xx, x eps, eps x and eps eps blocks: the filter propagates its estimate with the plan's model and the applied control, so
 *          the disturbance the truth receives is exactly what the estimate misses, and the control cancels in eps to first order.
 *          Symmetrised as above: each pair from both of its triangles.
 * Limits: FIRST ORDER about the plan; Kf is the optimal gain for the stated model (no mismodelling study); no measurement at node K;
 * the clamp is not modelled; the quaternion's norm direction is a coordinate like any other.  Only the symmetric parts of S0 and N0
 * are used; that they are positive semi-definite is the caller's responsibility.
 *
 * report [B][SCVX_COV_NREP]: the sixteen SCVX_COV_* columns above with unchanged definitions, read off the z block of Xi.
 * navrep [B][SCVX_NAV_NREP]: */
#define SCVX_NAV_NREP 8
#define SCVX_NAV_M 0       /* sqrt of the block traces of Xi_K[eps eps], the navigation error at the landing: mass,          */
#define SCVX_NAV_R 1       /* position,                                                                                    */
#define SCVX_NAV_V 2       /* velocity,                                                                                    */
#define SCVX_NAV_Q 3       /* attitude,                                                                                    */
#define SCVX_NAV_W 4       /* rate (the block layout of SCVX_COV_SIG_*)                                                    */
#define SCVX_NAV_PEAK 5    /* max over nodes 0..K of sqrt(trace Xi_k[eps eps]) (before the update at the node)             */
#define SCVX_NAV_EST_R 6   /* sqrt of the r / v block trace of Cov(xhat_K - xbar_K) = Sigma_xx - C - C' + P, C = Xi_K[x eps]: */
#define SCVX_NAV_EST_V 7   /* the miss the vehicle BELIEVES it has                                                          */
/* x, u, deriv, gain, S0, w14 as scvx_cov_propagate_f64; N0 [B][14][14]; m, H [m][14], rm [m] as above (host arrays in both forms).
 * Optional dense outputs (NULL = not wanted): sig [B][K+1][n] and navsig [B][K+1][14] = sqrt(diag Xi_k) of the z and the eps block;
 * kf [B][K][14][m] = the filter gains (not touched when m = 0); joint [B][K+1][N][N] = every Xi_k, before the update at its node.
 * A non-finite tile, gain, S0 or N0 entry makes every column of its own trajectory's two reports NaN and cannot disturb another
 * trajectory.  The _f64 form is asynchronous on the context's stream.  SCVX_ERR_ARG for everything scvx_cov_propagate_f64 refuses, a
 * null N0 or navrep, m outside [0, 14], m > 0 with a null H or rm, an rm <= 0 or non-finite, a non-finite H. */
int scvx_nav_cov_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                     const double *gain_dev, const double *S0_dev, const double *N0_dev, int m, const double *H, const double *rm,
                     const double *w14, double *report_dev, double *navrep_dev, double *sig_dev, double *navsig_dev,
                     double *kf_dev, double *joint_dev);
int scvx_nav_cov_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv, const double *gain,
                          const double *S0, const double *N0, int m, const double *H, const double *rm, const double *w14,
                          double *report, double *navrep, double *sig, double *navsig, double *kf, double *joint);
/* The same launch, keeping what the margins are made of (scvx_cov_path_sigma_f64 for the closed loop flown on an estimate): psig
 * [B][K+1][SCVX_PSIG_N] = s = sqrt(c' Xi_k[z z] c) of the five path functions at every node -- the TRUTH block of the joint, before
 * the update at the node (which does not touch it): the constraints bind the vehicle, not its estimate.  Same contract: node 0 is 0
 * and so is a node that the margin skips (undefined gradient); a non-finite tile, gain, S0 or N0 entry makes every row of its own
 * trajectory NaN, and nothing of another's.  With N0 = 0 the estimate never errs and psig is scvx_cov_path_sigma_f64's to rounding.
 * Arguments up to navrep as scvx_nav_cov_f64, whose two reports this call leaves bitwise unchanged (max_k psig[k][THRUST] is
 * S_THRUST); SCVX_ERR_ARG also for a null psig.  The _f64 form is asynchronous on the context's stream. */
int scvx_nav_path_sigma_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                            const double *gain_dev, const double *S0_dev, const double *N0_dev, int m, const double *H,
                            const double *rm, const double *w14, double *report_dev, double *navrep_dev, double *psig_dev);
int scvx_nav_path_sigma_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv,
                                 const double *gain, const double *S0, const double *N0, int m, const double *H, const double *rm,
                                 const double *w14, double *report, double *navrep, double *psig);
/* scvx_track_fly_f64 with the law fed an estimate: nav [B][K][14] is the error eps+_k of the estimate at node k, and the deviation
 * is formed as z = [(x_fly - nav_k) - xbar_k; u_k - ubar_k], so an all-zero nav reproduces scvx_track_fly_f64 bit for bit.  nav must
 * not be NULL (SCVX_ERR_ARG): without one, call scvx_track_fly_f64.  Everything else as there. */
int scvx_track_fly_nav_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *sigma_dev,
                           const double *gain_dev, const double *dx0_dev, const double *nav_dev, int nsub, int flags,
                           double *report_dev, double *xfly_dev, double *ufly_dev);
int scvx_track_fly_nav_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *sigma,
                                const double *gain, const double *dx0, const double *nav, int nsub, int flags, double *report,
                                double *xfly, double *ufly);

/* ---- sampled closed-loop dispersion: S flights per plan, reduced on the device --------------------------------------------------
 * Both covariance analyses above are FIRST ORDER about the plan and do not model the clamp.  This call is their nonlinear
 * counterpart: it flies S samples of EVERY plan of a batch under the tracking law, optionally disturbed at every node, and returns
 * one row of statistics per plan.  A flight is the pair (plan b, sample s); the plan, its sigma and its gains are read once per
 * wavefront, not copied per sample as a sampled check through scvx_track_fly_f64 has to, and no dense output need leave the device.
 * Model.  Flight (b, s) is scvx_track_fly_f64's closed loop, arithmetic included, from the start
 *     x_fly[0] = xbar_0 + dx0,   dx0[i] = sum_j C0[b][i][j] xi0[s][j]      (fma, ascending j from 0)
 * C0 [B][14][14] row-major: a factor of the plan's handover covariance, S0 = C0 C0'; xi0 [S][14]: standard-normal draws SHARED by
 * all plans (common random numbers: two plans are compared on the same draws).  With eta = NULL a flight's 16 SCVX_FLIGHT_* columns
 * are bitwise those of scvx_track_fly_f64 for the same plan, gains, flags, nsub and the dx0 this call formed.
 * Process noise (optional): eta [S][K][14] standard-normal draws, also shared by all plans, and sw14 [14] >= 0 = sqrt(w), a HOST
 * array.  The noise is an IMPULSE at the nodes: after segment k is integrated,
 *     x_fly[k+1][i] = fma(sw[i], eta[s][k][i], x_fly[k+1][i])              k = 0..K-1
 * before node k+1's gap, landing row and feedback see the state.  Its covariance is exactly the + diag(w) of
 * scvx_cov_propagate_f64.  The s = nsub sample of segment k sees the undisturbed state, the s = 0 sample of segment k+1 the disturbed
 * one; the last impulse (k = K-1) is followed by no sample: it enters GAP at node K, the MISS_* columns, MASS_END and the landing
 * statistics only.  eta = NULL, or sw14 all zero, gives bitwise the undisturbed result.
 * Per flight, besides the 16 columns: two counters over the COMMANDED node controls k = 1..K, before the clamp, of
 * Tmin - |u[1:3]| > tol and of |u[1:3]| - Tmax > tol, and the landing deviation e = x_fly[K] - xbar_K.
 * Reduction: on the device, deterministic (a fixed butterfly per wavefront, the wavefronts of a plan combined in order; no
 * floating-point atomics): two calls with the same inputs give bitwise equal outputs.  mcrep [B][SCVX_MC_NREP], c = 0..15 the
 * SCVX_FLIGHT_* columns: */
#define SCVX_MC_NREP 48
#define SCVX_MC_MAX 0      /* 0..15   MAX_c: the largest value of flight column c over the S flights (a NaN flight makes it NaN)     */
#define SCVX_MC_MEAN 16    /* 16..31  MEAN_c: the mean of flight column c, ordinary IEEE arithmetic: a column that is -inf for the    */
                           /*         model stays -inf, a NaN flight makes it NaN                                                    */
#define SCVX_MC_P_MASS 32  /* 32..40  P_MASS .. P_FIN: the share of flights whose G_MASS .. G_FIN (flight columns 6..14) exceed tol  */
#define SCVX_MC_P_ANY 41   /* the share of flights with any of those nine above tol (a comparison with NaN is false)                */
#define SCVX_MC_OUT_LO 42  /* the share of the S K commanded node controls with Tmin - |u[1:3]| > tol; with SCVX_TRACK_CLAMP and      */
#define SCVX_MC_OUT_HI 43  /* tol = 0: the share that was clamped on that side.  OUT_HI: |u[1:3]| - Tmax > tol                       */
#define SCVX_MC_N_BAD 44   /* the number of flights whose GAP is not finite                                                         */
#define SCVX_MC_S 45       /* S                                                                                                     */
                           /* 46..47  0                                                                                             */
/* Landing statistics, about the PLANNED final node (not about zero, not about the target): xmean [B][14] = the mean of e; xcov
 * [B][14][14] = the sample covariance of e, divisor S - 1, from the accumulated sums of e and e e' (all zero for S = 1).
 * Optional dense outputs (NULL = not wanted): flights [B][S][SCVX_FLIGHT_NREP], xland [B][S][14] = x_fly[K], dx0 [B][S][14] = the
 * offsets the device formed.  A non-finite gain, plan or C0 entry poisons the rows of its own plan only (N_BAD = S, NaN statistics).
 * Limits: the law is fed the TRUTH -- the sampled loop flown on a navigation estimate is scvx_track_mc_nav_f64 below, and `reserved`
 * (must be NULL) keeps its place in the argument list; the draws are shared across plans, so the rows of one call are not independent experiments;
 * order statistics of the flight columns and of the per-node path functions are reduced on the device by scvx_track_mc_q_f64 below
 * (this call returns none); w is the per-segment lump of the analyses, here as an impulse.
 * x, u, sigma, gain, flags (SCVX_TRACK_CLAMP), nsub as scvx_track_fly_f64; tol >= 0.  The _f64 form takes device pointers (sw14 on
 * the host) and is asynchronous on the context's stream; its partial sums live in a workspace that belongs to the context, so two
 * calls on one context must not overlap on different streams.  SCVX_ERR_ARG for S < 1, B < 1 (or B > 65535), K != the problem's K,
 * nsub outside [1, 1000], unknown flag bits, a negative or non-finite sw or tol, eta without sw, a non-NULL reserved, a null x / u /
 * sigma / gain / C0 / xi0 / mcrep / xmean / xcov. */
int scvx_track_mc_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                      const double *gain_dev, const double *C0_dev, const double *xi0_dev, const double *eta_dev,
                      const double *sw14, const void *reserved, int nsub, int flags, double tol, double *mcrep_dev,
                      double *xmean_dev, double *xcov_dev, double *flights_dev, double *xland_dev, double *dx0_dev);
int scvx_track_mc_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                           const double *gain, const double *C0, const double *xi0, const double *eta, const double *sw14,
                           const void *reserved, int nsub, int flags, double tol, double *mcrep, double *xmean, double *xcov,
                           double *flights, double *xland, double *dx0);

/* ---- sampled closed-loop dispersion flown on a navigation ESTIMATE ---------------------------------------------------------------
 * scvx_track_mc_f64 feeds the law the truth; scvx_nav_cov_f64 is first order.  This call is the nonlinear, sampled counterpart of the
 * navigation analysis: the S flights per plan of scvx_track_mc_f64 with the law fed an estimate whose error eps is generated PER FLIGHT
 * on the device from the filter gains of the analysis, with measurement noise and with the process noise that hits the truth.
 * Model.  Flight (b, s) is scvx_track_mc_f64's flight, statement for statement (start, impulses, clamp, samples, counters), with the
 * law fed x_fly - eps+_k: the deviation is formed as in scvx_track_fly_nav_f64, z = [(x_fly - eps+_k) - xbar_k; u_k - ubar_k].  The
 * error eps (14 per flight) follows the linear recursion of the analysis:
 *     eps_0     = CN[b] xin[s]                                          (fma, ascending j from 0; CN [B][14][14] row-major, a factor
 *                                                                        of the analysis's N0 = CN CN')
 *     eps+_k    = eps_k - Kf[b][k] (H eps_k + sqrt(rm) (.) nud[s][k])     k = 0..K-1     (m = 0: eps+_k = eps_k)
 *     eps_{k+1} = A_k[b] eps+_k  (+ sqrt(w) (.) eta[s][k]  when eta is given)
 * with A_k the state block of the plan's derivative tile (deriv [B][K][14+2NU+1][14], column-major tiles: the first 14 columns), Kf
 * [B][K][14][m] the gains scvx_nav_cov_f64 writes (`kf`), H [m][14] and rm [m] HOST arrays as there, xin [S][14] and nud [S][K][m]
 * standard-normal draws shared by all plans like xi0 and eta.  The eta is THE SAME eta[s][k] that the truth receives as an impulse, with
 * the same sign: the filter propagates its estimate without the disturbance, so eps receives it -- the W "in all four blocks" of
 * scvx_nav_cov_f64.  w14 [14] >= 0 is the VARIANCE w, a host array, as the navigation call takes it (the library forms sqrt(w)), so one
 * w feeds the gains and the flights; eta = NULL, or w14 all zero: no process noise.  With CN = 0, m = 0 and no noise every output that
 * scvx_track_mc_f64 has is bitwise that call's; with eta = NULL a flight's 16 columns and x_fly[K] are bitwise those of
 * scvx_track_fly_nav_f64 fed the dx0 and the eps+ (`navfed`) this call formed.
 * Limits: the recursion for eps is LINEAR and does not depend on the flown state -- it is the analysis's error model with the truth
 * flown nonlinearly, not an EKF re-linearised on the flown state; the gains are the analysis's gains, not recomputed per flight; there
 * is no measurement at node K; the clamp acts on the command formed from the estimate; and the limits of scvx_track_mc_f64.
 * Outputs.  mcrep [B][SCVX_MC_NREP], xmean [B][14], xcov [B][14][14]: exactly as scvx_track_mc_f64 defines them.  jmean [B][28] and
 * jcov [B][28][28]: the mean and the sample covariance (divisor S - 1, zero for S = 1) of [e; eps_K], e = x_fly[K] - xbar_K, by the
 * accumulation of xcov: xcov is bitwise jcov[:, 0:14, 0:14].  mcnav [B][SCVX_NAV_NREP], the sampled counterpart of navrep: SCVX_NAV_M ..
 * SCVX_NAV_W the square roots of the block traces of the eps block of jcov; column 5 (where navrep has NAV_PEAK: per-node sums stay out
 * of the reduction) is MAX_FED, */
#define SCVX_MCNAV_MAX_FED 5 /* the largest |eps+_k|_inf fed to the law over all flights and nodes, NaN if any is NaN                  */
/* and SCVX_NAV_EST_R, SCVX_NAV_EST_V from Sigma_xx - C - C' + P of jcov, as navrep defines them.  Optional dense outputs (NULL = not
 * wanted): flights, xland, dx0 as scvx_track_mc_f64; navfed [B][S][K][14] = eps+_k; navK [B][S][14] = eps_K.  Without a dense output
 * the device memory of the call is O(B S), not O(B S K).  The reduction is deterministic as there: two calls agree bit for bit.  A
 * non-finite kf, deriv, CN, gain or plan entry poisons the rows of its own plan only (N_BAD = S, NaN statistics).
 * The _f64 form takes device pointers (w14, H, rm on the host), is asynchronous on the context's stream and shares the workspace of
 * scvx_track_mc_f64 (no two of these calls overlapping on different streams).  SCVX_ERR_ARG for everything scvx_track_mc_f64 and the
 * measurement model of scvx_nav_cov_f64 refuse (m outside [0, 14], m > 0 with a null H or rm, an rm <= 0 or non-finite, a non-finite
 * H), a negative or non-finite w14, eta without w14, a null deriv / CN / xin / jmean / jcov / mcnav, m > 0 with a null kf or nud. */
int scvx_track_mc_nav_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                          const double *gain_dev, const double *C0_dev, const double *xi0_dev, const double *eta_dev,
                          const double *w14, const double *deriv_dev, const double *kf_dev, const double *CN_dev,
                          const double *xin_dev, const double *nud_dev, int m, const double *H, const double *rm, int nsub, int flags,
                          double tol, double *mcrep_dev, double *xmean_dev, double *xcov_dev, double *jmean_dev, double *jcov_dev,
                          double *mcnav_dev, double *flights_dev, double *xland_dev, double *dx0_dev, double *navfed_dev,
                          double *navK_dev);
int scvx_track_mc_nav_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                               const double *gain, const double *C0, const double *xi0, const double *eta, const double *w14,
                               const double *deriv, const double *kf, const double *CN, const double *xin, const double *nud, int m,
                               const double *H, const double *rm, int nsub, int flags, double tol, double *mcrep, double *xmean,
                               double *xcov, double *jmean, double *jcov, double *mcnav, double *flights, double *xland, double *dx0,
                               double *navfed, double *navK);

/* ---- exact batched order statistics ------------------------------------------------------------------------------------------------
 * Row r is the S values v[r * ld + s * inc], s = 0..S-1; out[r][i] is its element of rank ranks[i] in ASCENDING order, ranks 0-based,
 * 0 <= rank < S (rank 0 the minimum, rank S - 1 the maximum), a HOST array of nq entries that need be neither sorted nor distinct,
 * 1 <= nq <= SCVX_Q_MAX.  The order is -inf < .. < -0 = +0 < .. < +inf < every NaN (NaNs last, as numpy.sort puts them).  The result
 * is a SELECTION, never an interpolation: the output is one of the inputs bit for bit; a NaN is returned as some NaN, and either zero
 * may be returned for +-0.  A probability p maps to the rank min(S - 1, max(0, ceil(p S) - 1)) -- numpy's method="inverted_cdf", p = 0
 * the minimum and p = 1 the maximum (montecarlo.quantile_ranks on the Python side).  Deterministic: integer histograms only, no
 * floating-point atomics; two launches give bitwise equal output.  One workgroup per row, a most-significant-digit radix select over
 * monotone 64-bit keys (csrc/scvx_quantile.hip); every S >= 1 is served.  The _f64 form takes device pointers (ranks on the host) and
 * is asynchronous on the context's stream.  SCVX_ERR_ARG for R < 1, S < 1, nq outside [1, SCVX_Q_MAX], a rank outside [0, S), inc < 1,
 * R > 1 with ld < (S - 1) inc + 1, a null v, ranks or out. */
#define SCVX_Q_MAX 16
int scvx_order_stats_f64(scvx_ctx *ctx, int R, int S, const double *v_dev, size_t ld, size_t inc, int nq, const int *ranks,
                         double *out_dev);
int scvx_order_stats_f64_host(scvx_ctx *ctx, int R, int S, const double *v, size_t ld, size_t inc, int nq, const int *ranks,
                              double *out);

/* ---- sampled closed-loop dispersion with order statistics and per-node samples ---------------------------------------------------
 * scvx_track_mc_f64 and scvx_track_mc_nav_f64 reduce every column over the whole flight to MAX, MEAN and shares above one tol.  The
 * _q forms take the argument list of the call they extend, verbatim, followed by
 *     int nq, const int *ranks (host), double *flightq [B][16][nq], double *pathq [B][K+1][5][nq], double *pathv [B][K+1][5][S]
 * Any of the three outputs may be NULL; all NULL with nq = 0 IS the call they extend (the old entry points are this path with nothing
 * requested, and launch the kernels they always launched).  Ranks as scvx_order_stats_f64 (0-based, ascending, a selection).
 * flightq: the order statistics over the S flights of each of the sixteen SCVX_FLIGHT_* columns of plan b.  A column that is -inf for
 * the model stays -inf; a poisoned plan gives NaN.
 * pathv: the five path functions of psig (SCVX_PSIG_*) sampled at EVERY node k = 0..K of every flight,
 *     pathv[((b (K + 1) + k) 5 + f) S + s]                      (the sample is the fastest index)
 * MASS = x[0], GLIDE = tan(gammaGs) |r[2:3]| - r[1], TILT = |q[3:4]|, RATE = |w|: the audit's own expressions, WITHOUT the constants the
 * audit subtracts for tilt (sqcm) and rate (omMax), taken of the flown state as node k's feedback sees it -- node 0 is xbar_0 + dx0,
 * node k >= 1 is after the impulse of segment k - 1.  In the navigation form this is the TRUTH, not the estimate: the constraints bind
 * the vehicle (psig is read off the truth block for the same reason).  THRUST = the norm |u[1:3]| of the control COMMANDED for node k,
 * BEFORE the clamp -- the quantity OUT_LO / OUT_HI test; at node 0 it is |ubar_0|; in the navigation form it is the command formed from
 * the estimate.  With SCVX_TRACK_CLAMP it is still the unclamped command.
 * pathq: the order statistics of each (b, k, f) row of pathv.
 * Limits.  A tail quantile from S flights is itself uncertain: under a normal model the standard error of the p-quantile estimate is
 * sqrt(p (1 - p) / S) / phi(z_p) standard deviations (0.26 sigma at p = 0.99865, S = 1,024 -- and at S (1 - p) < 1 the rank is the
 * maximum of the sample, whatever p says).  The draws are shared across plans (the _rng forms below: unless independent = 1).  A back-off formed from the glide quantile buys
 * tan(gammaGs) times what is written, as the covariance back-offs do.
 * Workspace.  When the caller passes no dense flights / pathv but asks for their quantiles, the values live in a workspace that belongs
 * to the context, grown on demand, beside the workspace of partial rows and under its rule: calls on one context must not overlap on
 * different streams.  Its size is B S 16 doubles for flightq and B (K + 1) 5 S doubles for pathq: 267 MB at B = 128, S = 1,024, K = 50.
 * The device-pointer forms are asynchronous on the context's stream (ranks on the host).  SCVX_ERR_ARG for everything the call extended
 * refuses, and, unless nq = 0 with flightq = pathq = NULL, for nq outside [1, SCVX_Q_MAX], null ranks, a rank outside [0, S). */
int scvx_track_mc_q_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                        const double *gain_dev, const double *C0_dev, const double *xi0_dev, const double *eta_dev,
                        const double *sw14, const void *reserved, int nsub, int flags, double tol, double *mcrep_dev,
                        double *xmean_dev, double *xcov_dev, double *flights_dev, double *xland_dev, double *dx0_dev, int nq,
                        const int *ranks, double *flightq_dev, double *pathq_dev, double *pathv_dev);
int scvx_track_mc_q_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                             const double *gain, const double *C0, const double *xi0, const double *eta, const double *sw14,
                             const void *reserved, int nsub, int flags, double tol, double *mcrep, double *xmean, double *xcov,
                             double *flights, double *xland, double *dx0, int nq, const int *ranks, double *flightq, double *pathq,
                             double *pathv);
int scvx_track_mc_nav_q_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                            const double *gain_dev, const double *C0_dev, const double *xi0_dev, const double *eta_dev,
                            const double *w14, const double *deriv_dev, const double *kf_dev, const double *CN_dev,
                            const double *xin_dev, const double *nud_dev, int m, const double *H, const double *rm, int nsub,
                            int flags, double tol, double *mcrep_dev, double *xmean_dev, double *xcov_dev, double *jmean_dev,
                            double *jcov_dev, double *mcnav_dev, double *flights_dev, double *xland_dev, double *dx0_dev,
                            double *navfed_dev, double *navK_dev, int nq, const int *ranks, double *flightq_dev, double *pathq_dev,
                            double *pathv_dev);
int scvx_track_mc_nav_q_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                                 const double *gain, const double *C0, const double *xi0, const double *eta, const double *w14,
                                 const double *deriv, const double *kf, const double *CN, const double *xin, const double *nud,
                                 int m, const double *H, const double *rm, int nsub, int flags, double tol, double *mcrep,
                                 double *xmean, double *xcov, double *jmean, double *jcov, double *mcnav, double *flights,
                                 double *xland, double *dx0, double *navfed, double *navK, int nq, const int *ranks,
                                 double *flightq, double *pathq, double *pathv);

/* ---- sampled closed-loop dispersion with the draws made on the device ------------------------------------------------------------
 * The calls above read standard-normal draws xi0, eta, xin, nud that the caller made and uploaded, shared by all plans.  In the _rng
 * forms every lane makes its own from a counter-based generator: nothing is generated or uploaded by the host, and the draws may be
 * independent per plan.  The stream, which a caller can reproduce word for word:
 * Generator.  Philox4x64-10 exactly as numpy's np.random.Philox: multipliers M0 = 0xD2E7470EE14C6C93, M1 = 0xCA5A826395121157, Weyl
 * constants 0x9E3779B97F4A7C15, 0xBB67AE8584CAA73B added to the key after every round; one round maps the counter c to
 *     [hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0)];
 * ten rounds, key [seed, 0].  Block j of the stream with base counter [0, c1, c2, c3] is the block of counter [1 + j, c1, c2, c3]
 * (numpy increments before its first block): np.random.Philox(key=seed, counter=[0, c1, c2, c3]).random_raw(4 n) are blocks 0..n-1.
 * Streams.  c1 = 6 for the truth (xi0, eta), c1 = 7 for the navigation error (xin, nud); c3 = s_lo + s for sample s of the call;
 * c2 = 0 with shared draws (independent = 0: every plan flies the same draws, as in the calls above), c2 = 1 + b_lo + b for plan b
 * with independent = 1: the B rows of one call are then independent experiments, and a statistic pooled over plans has B S flights.
 * Layout.  A group of 14 draws occupies 4 blocks = 16 normals, draw i is normal i & 3 of block i >> 2 (two are unused).  Group 0 is
 * the start (xi0 / xin), group 1 + k belongs to node k (eta[s][k][0:14] / nud[s][k][0:m], the first m of its 14).  So nud does not
 * depend on m, xi0 does not depend on the noise, nothing depends on K, any (s, k, i) is random access, and the flights of
 * s_lo = 64, S = 66 are flights 64..129 of s_lo = 0, S = 130.
 * Normals.  Box-Muller per block: u_j = ((w_j >> 11) + 0.5) 2^-53 in double arithmetic (never 0), (z0, z1) = sqrt(-2 log u0)
 * (cospi(2 u1), sinpi(2 u1)) and (z2, z3) likewise from u2, u3: the device's log and sincospi, a few ulp from the exact value.
 * scvx_mc_draws_f64 writes the draws themselves, the same bits the flying kernels consume: xi0, xin [P][S][14] and eta, nud
 * [P][S][K][14] (all 14 of a group), each NULL or wanted, for plans b = 0..P-1 (P = 1 with shared draws, B with independent ones).
 * A flight of an _rng call is bitwise the flight of the _q call fed these arrays.
 * scvx_track_mc_rng_f64 is scvx_track_mc_q_f64 with (xi0, eta) replaced by (rng, noise): noise != 0 is what eta != NULL is there (the
 * truth receives the impulses sw14 * eta; sw14 is then required).  scvx_track_mc_nav_rng_f64 is scvx_track_mc_nav_q_f64 with (xi0,
 * eta) replaced by (rng, noise) and (xin, nud) dropped -- the same rng defines them.  All outputs, dense outputs, quantile arguments
 * and workspace rules are those of the _q forms.  SCVX_ERR_ARG as those forms, and for a null rng, a non-zero reserved, or independent
 * outside {0, 1}; scvx_mc_draws_f64 also for P outside [1, 65535], S < 1 or K < 1. */
typedef struct scvx_mc_rng {
    uint64_t seed, s_lo, b_lo;
    int32_t independent, reserved; /* reserved must be 0 */
} scvx_mc_rng;
int scvx_mc_draws_f64(scvx_ctx *ctx, const scvx_mc_rng *rng, int P, int S, int K, double *xi0_dev, double *eta_dev, double *xin_dev,
                      double *nud_dev);
int scvx_mc_draws_f64_host(scvx_ctx *ctx, const scvx_mc_rng *rng, int P, int S, int K, double *xi0, double *eta, double *xin,
                           double *nud);
int scvx_track_mc_rng_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                          const double *gain_dev, const double *C0_dev, const scvx_mc_rng *rng, int noise, const double *sw14,
                          const void *reserved, int nsub, int flags, double tol, double *mcrep_dev, double *xmean_dev,
                          double *xcov_dev, double *flights_dev, double *xland_dev, double *dx0_dev, int nq, const int *ranks,
                          double *flightq_dev, double *pathq_dev, double *pathv_dev);
int scvx_track_mc_rng_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                               const double *gain, const double *C0, const scvx_mc_rng *rng, int noise, const double *sw14,
                               const void *reserved, int nsub, int flags, double tol, double *mcrep, double *xmean, double *xcov,
                               double *flights, double *xland, double *dx0, int nq, const int *ranks, double *flightq,
                               double *pathq, double *pathv);
int scvx_track_mc_nav_rng_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                              const double *gain_dev, const double *C0_dev, const scvx_mc_rng *rng, int noise, const double *w14,
                              const double *deriv_dev, const double *kf_dev, const double *CN_dev, int m, const double *H,
                              const double *rm, int nsub, int flags, double tol, double *mcrep_dev, double *xmean_dev,
                              double *xcov_dev, double *jmean_dev, double *jcov_dev, double *mcnav_dev, double *flights_dev,
                              double *xland_dev, double *dx0_dev, double *navfed_dev, double *navK_dev, int nq, const int *ranks,
                              double *flightq_dev, double *pathq_dev, double *pathv_dev);
int scvx_track_mc_nav_rng_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                                   const double *gain, const double *C0, const scvx_mc_rng *rng, int noise, const double *w14,
                                   const double *deriv, const double *kf, const double *CN, int m, const double *H,
                                   const double *rm, int nsub, int flags, double tol, double *mcrep, double *xmean, double *xcov,
                                   double *jmean, double *jcov, double *mcnav, double *flights, double *xland, double *dx0,
                                   double *navfed, double *navK, int nq, const int *ranks, double *flightq, double *pathq,
                                   double *pathv);

/* ---- sampled closed-loop dispersion with per-flight VEHICLE ERRORS ------------------------------------------------------------------
 * The calls above fly one vehicle, the nominal one: their flights differ in the start and in the impulses only.  The _veh forms add
 * errors of the vehicle itself that are CONSTANT over a flight, which neither S0 nor w can express:
 *     theta = mu + sp (.) zeta        (fma(sp_i, zeta_i, mu_i)),  zeta ~ N(0, I_6) per flight,  SCVX_VEH_N = 6 components: */
#define SCVX_VEH_N 6
#define SCVX_VEH_THRUST 0 /* relative thrust error:      ua[0:3] = (1 + th0) (uu[0:3] + d x uu[0:3]),  d = (0, th1, th2)                  */
#define SCVX_VEH_MIS_Y 1  /* misalignment of the thrust axis about body y and z, in radians: the d above.  A FIRST-ORDER rotation, kept  */
#define SCVX_VEH_MIS_Z 2  /* first order: |u + d x u| = |u| sqrt(1 + O(|d|^2)), so the applied thrust (and the mass flow) grow by O(|d|^2) */
#define SCVX_VEH_ISP 3    /* alpha -> alpha (1 + th3) in the mass equation, which sees |ua|                                              */
#define SCVX_VEH_AERO 4   /* force_scalar -> force_scalar (1 + th4), trq_scalar alike with SCVX_MODEL_AERO_TORQUE; aerodynamic models only */
#define SCVX_VEH_FIN 5    /* ua[3:5] = (1 + th5) uu[3:5]; fin models only                                                                */
/* uu is the commanded first-order hold at the RK stage, formed exactly as in the calls above; ua replaces it in the right-hand side of
 * the TRUTH and nowhere else.  The error lies BEHIND the command: the law's z, the clamp, OUT_LO / OUT_HI, the THRUST column of pathv
 * and G_TMAX, G_TMIN, G_GIMBAL, G_FIN see the command, as they do in the calls above; the state columns and the landing statistics see
 * the vehicle that flew.  In the navigation form the recursion of eps is unchanged (the analysis's A_k); the truth is flown with theta.
 * Limits: constant over the flight; no wind, centre-of-gravity or inertia errors; the rotation is first order (above); a 1 + th <= 0
 * is not refused (the model is meant for |th| << 1).
 * Each _veh form takes the argument list of the _q form it extends, verbatim, followed by
 *     const scvx_mc_rng *rng, int noise, const scvx_mc_vehicle *veh, const double *zeta [S][6], double *theta [B][S][6]
 * rng != NULL: the lanes make the draws as in the _rng forms, and the uploaded draws (xi0, eta, xin, nud, zeta) must all be NULL; zeta
 * is then the first six normals of group 0 of Philox stream c1 = 8, with c2 / c3 as for streams 6 and 7 (shards and `independent` work
 * unchanged).  rng == NULL: noise must be 0 (eta != NULL says it, as in the _q forms), and zeta, shared by all plans like xi0, is
 * required as soon as any sp > 0.  theta (optional, dense): the errors every flight flew.  veh == NULL IS the _q / _rng call (zeta and
 * theta must then be NULL) and launches the kernels those launch.  SCVX_ERR_ARG as the form extended and as the _rng forms for rng; for
 * a non-finite mu, a negative or non-finite sp, a non-zero reserved; for a non-zero mu or sp of AERO on a model without aerodynamics
 * or of FIN on a model without fins. */
typedef struct scvx_mc_vehicle {
    double mu[SCVX_VEH_N], sp[SCVX_VEH_N];
    int32_t reserved[2]; /* must be 0 */
} scvx_mc_vehicle;
int scvx_track_mc_veh_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                          const double *gain_dev, const double *C0_dev, const double *xi0_dev, const double *eta_dev,
                          const double *sw14, const void *reserved, int nsub, int flags, double tol, double *mcrep_dev,
                          double *xmean_dev, double *xcov_dev, double *flights_dev, double *xland_dev, double *dx0_dev, int nq,
                          const int *ranks, double *flightq_dev, double *pathq_dev, double *pathv_dev, const scvx_mc_rng *rng,
                          int noise, const scvx_mc_vehicle *veh, const double *zeta_dev, double *theta_dev);
int scvx_track_mc_veh_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                               const double *gain, const double *C0, const double *xi0, const double *eta, const double *sw14,
                               const void *reserved, int nsub, int flags, double tol, double *mcrep, double *xmean, double *xcov,
                               double *flights, double *xland, double *dx0, int nq, const int *ranks, double *flightq, double *pathq,
                               double *pathv, const scvx_mc_rng *rng, int noise, const scvx_mc_vehicle *veh, const double *zeta,
                               double *theta);
int scvx_track_mc_nav_veh_f64(scvx_ctx *ctx, int B, int K, int S, const double *x_dev, const double *u_dev, const double *sigma_dev,
                              const double *gain_dev, const double *C0_dev, const double *xi0_dev, const double *eta_dev,
                              const double *w14, const double *deriv_dev, const double *kf_dev, const double *CN_dev,
                              const double *xin_dev, const double *nud_dev, int m, const double *H, const double *rm, int nsub,
                              int flags, double tol, double *mcrep_dev, double *xmean_dev, double *xcov_dev, double *jmean_dev,
                              double *jcov_dev, double *mcnav_dev, double *flights_dev, double *xland_dev, double *dx0_dev,
                              double *navfed_dev, double *navK_dev, int nq, const int *ranks, double *flightq_dev, double *pathq_dev,
                              double *pathv_dev, const scvx_mc_rng *rng, int noise, const scvx_mc_vehicle *veh,
                              const double *zeta_dev, double *theta_dev);
int scvx_track_mc_nav_veh_f64_host(scvx_ctx *ctx, int B, int K, int S, const double *x, const double *u, const double *sigma,
                                   const double *gain, const double *C0, const double *xi0, const double *eta, const double *w14,
                                   const double *deriv, const double *kf, const double *CN, const double *xin, const double *nud,
                                   int m, const double *H, const double *rm, int nsub, int flags, double tol, double *mcrep,
                                   double *xmean, double *xcov, double *jmean, double *jcov, double *mcnav, double *flights,
                                   double *xland, double *dx0, double *navfed, double *navK, int nq, const int *ranks,
                                   double *flightq, double *pathq, double *pathv, const scvx_mc_rng *rng, int noise,
                                   const scvx_mc_vehicle *veh, const double *zeta, double *theta);

/* ---- VEHICLE ERRORS in the first-order analyses (consider parameters) -----------------------------------------------------------------
 * scvx_cov_propagate_f64, scvx_cov_path_sigma_f64, scvx_nav_cov_f64 and scvx_nav_path_sigma_f64 analyse the nominal vehicle.  The forms
 * below add the six vehicle errors of the sampled calls above, theta = sp (.) zeta, zeta ~ N(0, I_6), constant over the flight and
 * independent of the handover, of the process noise and of the navigation error.  With J_k = d z_k / d theta (n x 6, n = 14 + NU):
 *     J_0 = 0,   J_{k+1} = M_k J_k + [Gamma_k; 0],   M_k = F_k + G_k L_k (the M of scvx_cov_propagate_f64),
 *     Sigma_k^tot = Sigma_k + J_k diag(sp^2) J_k'
 * and every output of the call extended (report, psig, sig, covK, cov) is read off Sigma_k^tot; the recursion of Sigma_k itself is that
 * of the plain call.  In the navigation form the same J_k diag(sp^2) J_k' is added to the truth block Xi_k[z, z] of the joint
 * wherever report, psig, sig and joint read it; the z-eps and eps-eps blocks, NAV_*, navsig and kf are those of the plain call (the
 * recursion of eps does not see theta).  SCVX_NAV_EST_R / EST_V, the trace of Cov(xhat_K - xbar_K) = Xi[x,x] - C - C' + P, receive
 * J P J' in their Xi[x,x] term alone: xhat = x - eps moves with the truth, and eps is independent of theta.
 * Gamma_k = d x_{k+1} / d theta (14 x 6) about the plan at theta = 0 and the context's nsub.  Four columns are in the derivative tiles
 * (the applied control is linear in the first-order hold and RK4 is linear in the forcing; d x u as above):
 *     Gamma[:, THRUST] = B-_k ubar_k[0:3] + B+_k ubar_{k+1}[0:3]
 *     Gamma[:, MIS_Y]  = B-_k (e_y x ubar_k[0:3]) + B+_k (e_y x ubar_{k+1}[0:3])          (MIS_Z with e_z)
 *     Gamma[:, FIN]    = B-_k[:, 3:5] ubar_k[3:5] + B+_k[:, 3:5] ubar_{k+1}[3:5]           (fin models)
 * and two are not: scvx_vehicle_tiles_f64 integrates them, vtile [B][K][SCVX_VTILE_N][14], */
#define SCVX_VTILE_N 2
#define SCVX_VTILE_ISP 0  /* d x_{k+1} / d theta_ISP:  c' = sigma (A c + e_0 (-alpha |uu|)),  c(0) = 0                                     */
#define SCVX_VTILE_AERO 1 /* d x_{k+1} / d theta_AERO: forcing F_aero / m in the v rows, + Jinv tau_aero in the w rows with                 */
                          /* SCVX_MODEL_AERO_TORQUE (what scales with force_scalar; not the fin force); all zeros without aerodynamics     */
/* beside the state from the planned node x_k under the planned hold, with the integrator, nsub and dt = 1 / (K + 1) of
 * scvx_propagate_f64: the derivative of the discrete flow the derivative tiles differentiate.  Refusals as scvx_propagate_f64.
 * The _vehicle forms take the argument list of scvx_cov_path_sigma_f64 (of scvx_nav_path_sigma_f64 followed by the dense outputs
 * sig, navsig, kf, joint of scvx_nav_cov_f64) with psig OPTIONAL, followed by
 *     double *sig, double *covK, double *cov (covariance form only: the dense outputs of scvx_cov_propagate_f64, optional),
 *     const double *vtile, const double *sp6 (HOST, the six standard deviations), double *sens [B][K+1][n][6] or NULL (J_k, unscaled)
 * vtile may be NULL only when sp[ISP] = sp[AERO] = 0.  SCVX_ERR_ARG for everything the call extended refuses, for a NULL sp6, a negative
 * or non-finite sp, sp[AERO] != 0 on a model without aerodynamics, sp[FIN] != 0 on a model without fins.  With sp = 0 every output is
 * that of the call extended.
 * There is NO mu: the analysis is about the nominal vehicle, theta = 0 in the mean.
 * Limits: first order about the plan; errors constant over the flight; the filter does not know theta (kf is the analysis's optimal
 * gain for the stated model, which has no theta); the [u, u] block, hence S_THRUST, N_TMIN, N_TMAX and the THRUST column of psig, is
 * the dispersion of the COMMAND, as in the sampled forms (the bottom NU rows of the forcing are zero: the command sees theta only
 * through the feedback).  Out of scope: a mean shift for mu != 0, time-varying errors, wind, centre-of-gravity and inertia errors, an
 * estimator that solves for theta. */
int scvx_vehicle_tiles_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *sigma_dev,
                           double *vtile_dev);
int scvx_vehicle_tiles_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *sigma, double *vtile);
int scvx_cov_vehicle_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                         const double *gain_dev, const double *S0_dev, const double *w14, double *report_dev, double *psig_dev,
                         double *sig_dev, double *covK_dev, double *cov_dev, const double *vtile_dev, const double *sp6,
                         double *sens_dev);
int scvx_cov_vehicle_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv, const double *gain,
                              const double *S0, const double *w14, double *report, double *psig, double *sig, double *covK,
                              double *cov, const double *vtile, const double *sp6, double *sens);
int scvx_nav_cov_vehicle_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                             const double *gain_dev, const double *S0_dev, const double *N0_dev, int m, const double *H,
                             const double *rm, const double *w14, double *report_dev, double *navrep_dev, double *psig_dev,
                             double *sig_dev, double *navsig_dev, double *kf_dev, double *joint_dev, const double *vtile_dev,
                             const double *sp6, double *sens_dev);
int scvx_nav_cov_vehicle_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv,
                                  const double *gain, const double *S0, const double *N0, int m, const double *H, const double *rm,
                                  const double *w14, double *report, double *navrep, double *psig, double *sig, double *navsig,
                                  double *kf, double *joint, const double *vtile, const double *sp6, double *sens);

/* ---- CLAMP-AWARE covariance analysis by statistical linearisation (no counterpart in the reference) --------------------------------
 * scvx_cov_propagate_f64 does not model the clamp of SCVX_TRACK_CLAMP, and the plans this solver produces ride Tmin: a clamped flight
 * loses authority at 12 to 49 of 100 node controls.  This call is the classical CADET (covariance analysis with random-input
 * describing functions): the thrust clamp is replaced, node by node, by the gain that fits it best in the mean square for a Gaussian
 * input, and a mean is carried beside the covariance.  It is an APPROXIMATION; the only statistically exact clamp-aware evidence
 * remains scvx_track_mc_f64.  Notation is that of scvx_cov_propagate_f64; z_k = [x_k - xbar_k; u_k - ubar_k] with u the APPLIED
 * control, the z that the law of scvx_track_fly_f64 with SCVX_TRACK_CLAMP sees.  A mean mu_k (n) and a central covariance Sigma_k
 * (n x n) are carried from mu_0 = 0, Sigma_0 = blockdiag((S0 + S0') / 2, 0).  Step k = 0..K-1, with the band (Tlo, Thi) = (Tmin,
 * Tmax) of the problem or the caller's band2:
 *   1. mean command  chat = ubar_{k+1} + L_k mu_k  (NU)
 *   2. That = |chat[0:3]|,  e = chat[0:3] / That
 *   3. g = L_k[0:3,:]' e  (n),  s = sqrt(max(g' Sigma_k g, 0)): one sigma of the commanded thrust norm, to first order about chat
 *   4. a = (Tlo - That) / s,  b = (Thi - That) / s,  P_lo = erfc(-a / sqrt 2) / 2,  P_hi = erfc(b / sqrt 2) / 2,  gamma = 1 - P_lo - P_hi
 *   5. E = Tlo P_lo + Thi P_hi + That gamma + s (phi(a) - phi(b)),  phi the standard normal density, evaluated as E = That + dE with
 *      dE = s (a P_lo + b P_hi + phi(a) - phi(b)), the same number without a difference of large terms (a term with P_hi is 0 where
 *      P_hi == 0, so Thi = +inf is allowed; with Tlo == 0 there is no lower clamp -- a norm is never below 0, and the flight's clamp
 *      does nothing there -- so P_lo = 0 and phi(a) is dropped, the mass a Gaussian puts below 0 being the linearisation's own):
 *      E = E[sat(t)] for t ~ N(That, s^2), and gamma = E[sat(t) (t - That)] / s^2 is the
 *      random-input describing-function gain of the clamp
 *   6. N = I_NU with the thrust block N[0:3,0:3] = gamma e e' + (E / That)(I - e e');  applied mean ahat = chat with ahat[0:3] = E e
 *   7. mu_{k+1} = F_k mu_k + G_k (ahat - ubar_{k+1})   (evaluated as L_k mu_k, plus dE e on the thrust rows of a saturated node: the
 *      same vector without the round trip through the plan's control)
 *   8. Ltilde_k = N L_k,  Mtilde_k = F_k + G_k Ltilde_k
 *   9. Sigma_{k+1} = sym(Mtilde_k Sigma_k Mtilde_k') + blockdiag(diag(w), 0), symmetrised exactly as the plain call does.
 * Special cases, part of the contract.  UNSATURATED NODE: P_lo == 0 and P_hi == 0 exactly in double -> N = I, ahat = chat and the rows
 * of L_k are left untouched: with a band nobody reaches Sigma_k is BITWISE scvx_cov_propagate_f64's and mu_k is exactly 0.  s == 0:
 * gamma = 1 if Tlo <= That <= Thi, else 0; E = min(max(That, Tlo), Thi); P_lo = (That < Tlo), P_hi = (That > Thi).  That == 0: no
 * clamp at that node (the flight's clamp leaves a zero thrust alone): P_lo = P_hi = s = 0, gamma = 1.  A non-finite tile, gain, S0 or
 * planned control makes its own trajectory's report and satrep NaN, and its dense rows from the node it enters, and touches no other.
 * Limits: FIRST ORDER about the plan in the dynamics; QUASI-LINEAR in the clamp (Gaussian input, the norm linearised about the mean
 * command, the remnant Var(sat) - gamma^2 s^2 dropped); the covariances live at the nodes; w is the per-segment lump; the fin-norm
 * clamp of SCVX_MODEL_FINS is NOT modelled (N's fin block is I: a mean fin command of zero has no direction to linearise along); the
 * gimbal cone is not projected, as in the flight.  Expect a factor of about 2 in standard deviation; this is not a statistical match.
 * Measured with the CPU reference (tests/cov_clamp_reference.py against 2,048 clamped flights of the C oracle per case; the two golden
 * plans, handover factor scaled by 0.1, 0.3 and 1; SL this call, LIN scvx_cov_propagate_f64), ranges over the six cases:
 *     trace of the landing v block, LIN / sampled 0.017 - 0.115     SL / sampled 0.28 - 1.64
 *     trace of the landing r block, LIN / sampled 0.012 - 0.90      SL / sampled 0.30 - 1.60
 *     SL / sampled: mass variance 0.76 - 0.99, q block 0.70 - 0.99, w block 0.93 - 1.03
 *     landing bias (LIN predicts none): cosine with the sampled mean 0.949 - 0.998, norm SL / sampled 0.98 - 2.38
 *     share of commands clamped (LIN predicts none): P_LO / sampled OUT_LO 1.28 - 1.46,  P_HI / sampled OUT_HI 1.10 - 1.22
 *
 * satrep, SCVX_SAT_NREP doubles per trajectory: */
#define SCVX_SAT_NREP 16
#define SCVX_SAT_SIG_M 0       /* SIG_M .. SIG_W as SCVX_COV_SIG_M .. SIG_W, from Sigma_K                                       */
#define SCVX_SAT_SIG_R 1
#define SCVX_SAT_SIG_V 2
#define SCVX_SAT_SIG_Q 3
#define SCVX_SAT_SIG_W 4
#define SCVX_SAT_BIAS_M 5      /* |mu_K[0]|, and the norms of the r, v, q, w blocks of mu_K: the predicted landing bias          */
#define SCVX_SAT_BIAS_R 6
#define SCVX_SAT_BIAS_V 7
#define SCVX_SAT_BIAS_Q 8
#define SCVX_SAT_BIAS_W 9
#define SCVX_SAT_RMS_R 10      /* sqrt(SIG_R^2 + BIAS_R^2): the root mean square landing miss about the planned node              */
#define SCVX_SAT_RMS_V 11      /* the same for v                                                                                  */
#define SCVX_SAT_P_LO 12       /* mean over k of P_lo, of P_hi: the predicted shares of node commands clamped from below, from    */
#define SCVX_SAT_P_HI 13       /* above -- the counterparts of SCVX_MC_OUT_LO / OUT_HI of a flight with the clamp                 */
#define SCVX_SAT_GAIN_MIN 14   /* min over k of gamma_k: 1 = the law keeps its authority everywhere, 0 = a node where it has none */
#define SCVX_SAT_BIAS_PEAK 15  /* max over nodes 0..K of |mu_k[0:14]|_2                                                           */
/* Arguments up to w14 as scvx_cov_propagate_f64.  band2: a HOST array (Tlo, Thi) in both forms, or NULL for the problem's (Tmin,
 * Tmax).  report [B][SCVX_COV_NREP]: the plain report read off Sigma_k by the code of scvx_cov_propagate_f64; its N_TMAX / N_TMIN /
 * S_THRUST then describe the APPLIED control about the planned one and are not headroom figures.  satrep [B][SCVX_SAT_NREP].
 * Optional dense outputs (NULL = not wanted): mean [B][K+1][n] = mu_k; sig, covK, cov as the plain call; satk [B][K][4] = (That, s,
 * P_lo, P_hi) of node k + 1.  The _f64 form is asynchronous on the context's stream.  SCVX_ERR_ARG for everything
 * scvx_cov_propagate_f64 refuses, a null satrep, and a band2 with a non-finite Tlo, a NaN Thi, Tlo < 0 or Tlo > Thi. */
int scvx_cov_clamp_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *deriv_dev,
                       const double *gain_dev, const double *S0_dev, const double *w14, const double *band2, double *report_dev,
                       double *satrep_dev, double *mean_dev, double *sig_dev, double *covK_dev, double *cov_dev, double *satk_dev);
int scvx_cov_clamp_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *deriv, const double *gain,
                            const double *S0, const double *w14, const double *band2, double *report, double *satrep, double *mean,
                            double *sig, double *covK, double *cov, double *satk);

/* fp32 forms of the two discretisation entry points (SURVEY.md 8b "_f64/_f32"; BASELINE configs[3-4] name fp32): the
 * same layouts in float, float arithmetic throughout (RK4 state + sensitivity columns), tables read from the same
 * double coefficients.  Stated tolerance against the fp64 path: 2e-5 relative on endpoint, 2e-4 on derivative at
 * npts = 10 (tests/test_gpu_discretize.py).  The conic solve has no fp32 form: its block-tridiagonal factor needs double
 * (cond(S) * eps_float ~ 1, DESIGN.md "fp32"), so the SCvx loop itself always runs in fp64. */
int scvx_linearize_f32(scvx_ctx *ctx, int B, int K, const float *x_dev, const float *u_dev,
                       const float *sigma_dev, float dt, float *endpoint_dev, float *deriv_dev);
int scvx_linearize_f32_host(scvx_ctx *ctx, int B, int K, const float *x, const float *u,
                            const float *sigma, float dt, float *endpoint, float *deriv);
int scvx_propagate_f32(scvx_ctx *ctx, int B, int K, const float *x_dev, const float *u_dev,
                       const float *sigma_dev, float dt, float *xnext_dev);
int scvx_propagate_f32_host(scvx_ctx *ctx, int B, int K, const float *x, const float *u,
                            const float *sigma, float dt, float *xnext);

/* ---- FirstRound.solve_initial: the 3-DoF lossless-convexification landing SOCP, batched --------
 * (initial_solve.jl:17-110, inside a block comment at HEAD; BASELINE configs[0]).  Per node k = 0..K: position r,
 * velocity v, mass ma, thrust T, thrust bound ga, virtual acceleration ar and its bound kaR; one global nkaR >= |kaR|;
 * minimise -ma_K + 100 nkaR under the trapezoidal point-mass recursions with the fixed mass profile of :24, the
 * boundary values of :59-65 and the cones of :69-70, :80-88.  The problem's K, alpha, tf_guess, mwet, mdry, g, Tmin,
 * Tmax, thetaMax, gammaGs are read from the context; rIi, vIi per trajectory.
 * A device interior-point solve, one wavefront per trajectory (csrc/scvx_threedof_core.hpp). */
typedef struct scvx_threedof_opts {
    int32_t max_iter;   /* 60 */
    int32_t refine;     /* refinement passes per Newton solve on the uncondensed residual: 1 */
    double tol;         /* primal / dual residual and relative gap: 1e-9 */
    double delta;       /* static regularisation of the quasi-definite KKT matrix: 1e-9 */
    int32_t attitude;   /* scvx_batch_init_threedof only.  0 (default) = the reference's rotation_between(e1, -T_k)
                         * (initial_solve.jl:98); 1 = rotation_between(e1, +T_k): the body axis the engine pushes along
                         * points along the 3-DoF thrust, which is what the 6-DoF model (control (|T|,0,0) in body axes)
                         * means -- the reference's sign makes the start fly backwards (tools/init_compare.py) */
    int32_t reserved;
} scvx_threedof_opts;
int scvx_threedof_default_opts(scvx_threedof_opts *o);
/* doubles per trajectory of a solution record: (K+1)*15 + 1 -- per node r(3) v(3) ma T(3) ga kaR ar(3), then nkaR */
int32_t scvx_threedof_record_doubles(int K);
/* ic [B][6] host = per-trajectory (rIi, vIi), NULL = the problem's own; opts NULL = defaults.  Outputs (host):
 * sol [B][record_doubles]; status [B] (0 optimal: residuals and relative gap below tol -- or, when the KKT system breaks
 * down at the numerical floor, below 10 tol / 100 tol, the band the oracle's solver reports as optimal too; 1 iteration
 * cap, 2 stalled, 3 non-finite, 4 almost optimal: breakdown with residuals and relative gap below 1e-6, 5 infeasible: the primal residual stopped falling while the gap closed); info [B][5] = iterations, objective, gap, primal and dual residual
 * (status and info may be NULL). */
int scvx_threedof_solve(scvx_ctx *ctx, int B, const double *ic, const scvx_threedof_opts *opts, double *sol,
                        int32_t *status, double *info);
/* The same on device arrays, enqueued on the context's stream: info_dev [B][6] = status, iterations, objective, gap,
 * primal and dual residual. */
int scvx_threedof_solve_dev(scvx_ctx *ctx, int B, const double *ic_dev, const scvx_threedof_opts *opts,
                            double *sol_dev, double *info_dev);

/* ---- batched SCvx: create_initial / solve_step / solve_problem ------------------------------ */
int scvx_solver_default_opts(scvx_solver_opts *o);
int scvx_batch_create(scvx_ctx *ctx, int B, scvx_batch **out);
void scvx_batch_destroy(scvx_batch *b);
int scvx_batch_set_solver(scvx_batch *b, const scvx_solver_opts *o);
/* ic [B][6] = per-trajectory (rIi, vIi) overriding the problem's (Monte-Carlo dispersions); NULL =
 * every trajectory uses the problem's own.  Builds the straight-line guess (initial_solve.jl:113-129),
 * linearises it and sets rk=100, cost=Inf, iter=0 (rocketland.jl:38). */
int scvx_batch_init(scvx_batch *b, const double *ic);
/* create_initial from FirstRound.solve_initial instead of the straight line: scvx_batch_init(b, ic), then every
 * trajectory whose 3-DoF solve is optimal starts from its LinPoints (initial_solve.jl:90-105: state (ma, r, v,
 * rotation_between(e1, -T), 0), control (|T|, 0, 0), sigma = tf_guess); the others keep the straight line.
 * status3 [B] (host, may be NULL) = the 3-DoF solver statuses.  scvx_batch_reset returns to this start. */
int scvx_batch_init_threedof(scvx_batch *b, const double *ic, const scvx_threedof_opts *opts, int32_t *status3);
/* create_initial again for the same initial conditions, entirely on the device and asynchronous on the stream: the
 * straight-line guess kept from scvx_batch_init is restored, rk=100, cost=Inf, iter=0, flags cleared, and the guess is
 * re-linearised.  (A Monte-Carlo driver that re-runs solve_problem, or a benchmark loop, needs no host round trip.) */
int scvx_batch_reset(scvx_batch *b);
/* One Rocketland.solve_step for every trajectory of the batch.  Outputs are host arrays of
 * length B (any may be NULL): status codes above, ||nu||_F and dJ (Inf on rejection).
 * Like the reference's solve_step this has no notion of convergence: SCVX_ST_CONVERGED reports that the
 * loop test of solve_problem (rocketland.jl:436) holds after this step, and the next call steps the
 * trajectory again.  A trajectory whose conic solve failed (SCVX_ST_SOLVER / SCVX_ST_NONFINITE -- where the
 * reference raises an error) is frozen: later calls skip it, its status keeps the failure code and its
 * nu_norm / dJ stay those of the failing step. */
int scvx_solve_step(scvx_batch *b, int32_t *status, double *nu_norm, double *dJ);
/* Asynchronous form for timing loops: enqueue one solve_step on the stream, no host read-back. */
int scvx_solve_step_async(scvx_batch *b);
/* Rocketland.solve_problem from the batch's current state: every trajectory is stepped until it converges
 * (then it is left alone, as the reference's loop exits), fails, or has taken imax-1 steps; iters[B] = total
 * solve_step calls applied to the trajectory since scvx_batch_init. */
int scvx_solve(scvx_batch *b, int32_t *status, int32_t *iters, double *nu_norm, double *dJ);

/* ---- iterate access (the batched ProblemIteration) ------------------------------------------ */
/* traj [B][(K+1)*(14+NU) + 1]: per trajectory x[K+1][14], u[K+1][NU], sigma  (NU = 3: 17 per node).  */
int scvx_batch_get_trajectory(scvx_batch *b, double *traj);
int scvx_batch_set_trajectory(scvx_batch *b, const double *traj);
/* device pointer to the same layout (zero-copy views; scvx_allgather_trajectories gathers it); valid until destroy */
int scvx_batch_trajectory_dev(scvx_batch *b, double **traj_dev, int64_t *n_doubles);
int scvx_batch_get_linearization(scvx_batch *b, double *endpoint, double *deriv);
/* Mixed precision (BASELINE configs[3-4] "fp32"; SURVEY 8b `_f64/_f32`, H7): keep the derivative tiles `dynam[k].derivative`
 * (LinRes, master.jl:91-93) in float.  The discretisation still integrates in double and rounds each entry once, at the
 * store; the conic solve widens on load and keeps its arithmetic, workspace, norms and pivots in double; the endpoint stays
 * double.  Halves the bytes of the one input every pass of the solve re-reads.  on = 1 / 0; an initialised batch is
 * re-linearised at once.  scvx_batch_get_linearization then returns the float values, widened. */
int scvx_batch_set_linearization_f32(scvx_batch *b, int on);
int scvx_batch_get_scalars(scvx_batch *b, double *rk, double *cost, int32_t *iter);
int scvx_batch_set_scalars(scvx_batch *b, const double *rk, const double *cost, const int32_t *iter);
/* per-trajectory flags, the rest of a checkpoint (trajectory + scalars + flags restore a batch after
 * scvx_batch_init with the same ic): status as above; active = 0 once failed (never stepped again);
 * live = active and not yet converged inside scvx_solve.  Any pointer may be NULL.
 * The conic solver's own warm-start state is NOT part of a checkpoint: scvx_batch_set_scalars / set_flags / set_trajectory
 * drop it, so the first solve of a restored (or edited) batch starts cold.  After an ACCEPTED step that is what an
 * uninterrupted run does too (bit-identical continuation); after a REJECTED step the uninterrupted run would have
 * warm-started, so the continuation agrees to the solver tolerance, not bit for bit.
 * The thrust back-offs (scvx_batch_set_thrust_margins below) ARE part of a checkpoint: scvx_batch_init clears them, so a restored
 * batch must be given them again (scvx_batch_get_thrust_margins reads them). */
int scvx_batch_get_flags(scvx_batch *b, int32_t *status, int32_t *active, int32_t *live);
int scvx_batch_set_flags(scvx_batch *b, const int32_t *status, const int32_t *active, const int32_t *live);
/* last SOCP solve, per trajectory: solver status (0 optimal: merit < tol; 4 almost optimal: numerical floor with
 * tol <= merit < accept_tol; 1 iteration cap; 2 numerical floor / KKT breakdown at merit >= accept_tol; 3 non-finite;
 * 5 infeasible: a fixed boundary value (rIi, vIi, wBi) violates the glideslope / rate / dynamic-pressure cone of node 1),
 * interior-point iterations, final merit max(pres, dres, relgap) of the returned iterate, its objective */
int scvx_batch_get_solver_stats(scvx_batch *b, int32_t *status, int32_t *iters, double *merit, double *pobj);

/* The flight check above on the batch's current accepted iterate: report [B][SCVX_FLIGHT_NREP] and xfly [B][K+1][14] (or NULL)
 * are host arrays; nsub = 0 takes the context's.  Reads the iterate and leaves the batch untouched (trajectory, scalars, flags,
 * linearisation, solver workspace): a solve_step after it equals the one without it bit for bit.  Synchronises. */
int scvx_batch_flight_check(scvx_batch *b, int nsub, int mode, double *report, double *xfly);

/* Plan tracking on the batch's current accepted iterate and its own derivative tiles (float tiles are widened on load when
 * scvx_batch_set_linearization_f32 is on): the gains, and the closed-loop flight under them from x[0] + dx0.  Host outputs;
 * any output pointer may be NULL; nsub = 0 takes the context's.  The gains live in scratch that is allocated on first use and
 * freed with the batch; the batch itself is left untouched, as by scvx_batch_flight_check.  Synchronises. */
int scvx_batch_track_gains(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, double *gain, double *p0);
int scvx_batch_track_fly(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *dx0, int nsub,
                         int flags, double *report, double *xfly, double *ufly);

/* The covariance analysis above on the batch's current accepted iterate and its own derivative tiles (float tiles are widened on
 * load), under the gains of the weights q14 / rNU / qf14 (computed into the scratch of scvx_batch_track_gains).  S0 [B][14][14],
 * w14 [14] or NULL and every output are host arrays; report, sig, covK, cov may each be NULL.  The batch is left untouched, as by
 * scvx_batch_flight_check.  Synchronises. */
int scvx_batch_cov(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0, const double *w14,
                   double *report, double *sig, double *covK, double *cov);

/* The two navigation calls above on the batch's current accepted iterate and its own derivative tiles (float tiles are widened on
 * load), under the gains of the weights q14 / rNU / qf14.  S0, N0 [B][14][14], H, rm, w14, nav [B][K][14], dx0 and every output are
 * host arrays; any output may be NULL.  The batch is left untouched, as by scvx_batch_flight_check.  Synchronises. */
int scvx_batch_nav_cov(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0, const double *N0,
                       int m, const double *H, const double *rm, const double *w14, double *report, double *navrep, double *sig,
                       double *navsig, double *kf, double *joint);
int scvx_batch_track_fly_nav(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *dx0,
                             const double *nav, int nsub, int flags, double *report, double *xfly, double *ufly);

/* The sampled dispersion above on the batch's current accepted iterate, under the gains of the weights q14 / rNU / qf14 computed
 * from the batch's own derivative tiles (float tiles are widened on load), as scvx_batch_track_fly does.  C0 [B][14][14], xi0
 * [S][14], eta [S][K][14] or NULL, sw14 and every output are host arrays; any output may be NULL; nsub = 0 takes the context's.  The
 * batch is left untouched, as by scvx_batch_flight_check.  Synchronises. */
int scvx_batch_track_mc(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                        const double *xi0, const double *eta, const double *sw14, const void *reserved, int nsub, int flags,
                        double tol, double *mcrep, double *xmean, double *xcov, double *flights, double *xland, double *dx0);

/* scvx_track_mc_nav_f64 on the batch's current accepted iterate, its own derivative tiles (float tiles are widened on load) and the
 * gains of the weights q14 / rNU / qf14.  N0 [B][14][14] is the handover covariance of the navigation error and CN [B][14][14] a factor
 * of it (N0 = CN CN'; the caller's responsibility): the call first runs the navigation launch on the device with N0, H, rm and w14 (and
 * S0 = 0: the filter gains do not depend on it) to obtain Kf, then the flights.  C0, xi0, eta, w14, xin, nud, H, rm and every output are
 * host arrays; any output may be NULL; nsub = 0 takes the context's.  The batch is left untouched, as by scvx_batch_flight_check.
 * Synchronises.  SCVX_ERR_ARG as scvx_track_mc_nav_f64, and for a null N0. */
int scvx_batch_track_mc_nav(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                            const double *xi0, const double *eta, const double *w14, const double *N0, const double *CN,
                            const double *xin, const double *nud, int m, const double *H, const double *rm, int nsub, int flags,
                            double tol, double *mcrep, double *xmean, double *xcov, double *jmean, double *jcov, double *mcnav,
                            double *flights, double *xland, double *dx0, double *navfed, double *navK);

/* The two calls above with the order statistics and the per-node samples of scvx_track_mc_q_f64 / scvx_track_mc_nav_q_f64: their
 * argument lists, verbatim, followed by nq, ranks, flightq [B][16][nq], pathq [B][K+1][5][nq] and pathv [B][K+1][5][S], all host
 * arrays, each output NULL or wanted; nq = 0 with all three NULL is the call above.  Synchronises.  SCVX_ERR_ARG as the call extended,
 * and as scvx_track_mc_q_f64 for nq and ranks. */
int scvx_batch_track_mc_q(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                          const double *xi0, const double *eta, const double *sw14, const void *reserved, int nsub, int flags,
                          double tol, double *mcrep, double *xmean, double *xcov, double *flights, double *xland, double *dx0,
                          int nq, const int *ranks, double *flightq, double *pathq, double *pathv);
int scvx_batch_track_mc_nav_q(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                              const double *xi0, const double *eta, const double *w14, const double *N0, const double *CN,
                              const double *xin, const double *nud, int m, const double *H, const double *rm, int nsub, int flags,
                              double tol, double *mcrep, double *xmean, double *xcov, double *jmean, double *jcov, double *mcnav,
                              double *flights, double *xland, double *dx0, double *navfed, double *navK, int nq, const int *ranks,
                              double *flightq, double *pathq, double *pathv);

/* The two calls above with the draws made on the device (scvx_track_mc_rng_f64 / scvx_track_mc_nav_rng_f64): their argument lists with
 * (xi0, eta) replaced by (rng, noise) and, in the navigation form, (xin, nud) dropped.  Nothing but C0 (and N0, CN) is uploaded.
 * Synchronises.  SCVX_ERR_ARG as the calls above and as scvx_track_mc_rng_f64 for rng. */
int scvx_batch_track_mc_rng(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                            const scvx_mc_rng *rng, int noise, const double *sw14, const void *reserved, int nsub, int flags,
                            double tol, double *mcrep, double *xmean, double *xcov, double *flights, double *xland, double *dx0,
                            int nq, const int *ranks, double *flightq, double *pathq, double *pathv);
int scvx_batch_track_mc_nav_rng(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                                const scvx_mc_rng *rng, int noise, const double *w14, const double *N0, const double *CN, int m,
                                const double *H, const double *rm, int nsub, int flags, double tol, double *mcrep, double *xmean,
                                double *xcov, double *jmean, double *jcov, double *mcnav, double *flights, double *xland,
                                double *dx0, double *navfed, double *navK, int nq, const int *ranks, double *flightq, double *pathq,
                                double *pathv);

/* The two _q calls above with per-flight vehicle errors (scvx_track_mc_veh_f64 / scvx_track_mc_nav_veh_f64): their argument lists,
 * verbatim, followed by rng, noise, veh, zeta [S][6] and theta [B][S][6] (host arrays).  veh == NULL is the _q call (rng == NULL) or
 * the _rng call.  Synchronises.  SCVX_ERR_ARG as the call extended and as scvx_track_mc_veh_f64 for the five. */
int scvx_batch_track_mc_veh(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                            const double *xi0, const double *eta, const double *sw14, const void *reserved, int nsub, int flags,
                            double tol, double *mcrep, double *xmean, double *xcov, double *flights, double *xland, double *dx0,
                            int nq, const int *ranks, double *flightq, double *pathq, double *pathv, const scvx_mc_rng *rng,
                            int noise, const scvx_mc_vehicle *veh, const double *zeta, double *theta);
int scvx_batch_track_mc_nav_veh(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, int S, const double *C0,
                                const double *xi0, const double *eta, const double *w14, const double *N0, const double *CN,
                                const double *xin, const double *nud, int m, const double *H, const double *rm, int nsub, int flags,
                                double tol, double *mcrep, double *xmean, double *xcov, double *jmean, double *jcov, double *mcnav,
                                double *flights, double *xland, double *dx0, double *navfed, double *navK, int nq, const int *ranks,
                                double *flightq, double *pathq, double *pathv, const scvx_mc_rng *rng, int noise,
                                const scvx_mc_vehicle *veh, const double *zeta, double *theta);

/* ---- thrust-band back-offs and covariance-driven replanning (no counterpart in the reference) ---------------------------------
 * Per-trajectory, per-node back-offs of the thrust band, read by the conic solve alone:
 *     Tmin + lo_k <= |u_k[1:3]| <= Tmax - hi_k        (the lower side through its linearised row, rocketland.jl:199)
 * the chance-constraint tightening lo_k = hi_k = n s_T(k) once the covariance analysis has the s_T(k).  Every conic solve of the batch
 * reads them (scvx_socp_solve, scvx_solve_step, scvx_solve); the discretisation, the trust-region update, the flight check and the
 * tracking calls keep auditing against the true Tmin / Tmax, so a margined plan shows its headroom as negative G_TMIN / G_TMAX.
 * With no back-offs set, or with all of them zero, every result is bitwise that of a batch that never heard of them.
 * lo, hi: host [B][K+1] each; both NULL clears.  SCVX_ERR_ARG for a negative or non-finite entry, for only one NULL pointer, and
 * for any node with lo + hi >= Tmax - Tmin.  Setting or clearing drops the conic solver's warm-start state and the
 * reuse_inactive_tr shortcut, as scvx_batch_set_trajectory does.  scvx_batch_init clears the back-offs; scvx_batch_reset keeps them.
 * scvx_batch_get_thrust_margins: zeros when none are set; either pointer may be NULL. */
int scvx_batch_set_thrust_margins(scvx_batch *b, const double *lo, const double *hi);
int scvx_batch_get_thrust_margins(scvx_batch *b, double *lo, double *hi);
/* The back-offs from the covariance analysis of the batch's current accepted iterate, on the device: the gains of q14 / rNU / qf14,
 * scvx_cov_path_sigma_f64 on the batch's own tiles, then lo_k = hi_k = min(nsigma s_T(k), cap (Tmax - Tmin)) into the batch's
 * back-off buffer.  S0 [B][14][14] and w14 [14] or NULL are host arrays; psig [B][K+1][SCVX_PSIG_N] (host, or NULL: then nothing
 * returns to the host and the call is asynchronous on the stream).  A trajectory whose psig rows are NaN gets zero back-offs.
 * SCVX_ERR_ARG for nsigma < 0 (or not finite), cap outside (0, 0.5), a null S0, a bad w or weight.
 * Limits: the analysis is FIRST ORDER, and the back-offs are only as good as Sigma_k; s_T depends on the plan, so the plan that
 * is solved under the back-offs of its predecessor has other s_T, and one round reaches about 2.5 - 3 sigma of headroom for
 * nsigma = 3 rather than exactly n (repeat the round to tighten it). */
int scvx_batch_thrust_margins_from_cov(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0,
                                       const double *w14, double nsigma, double cap, double *psig);
/* Start the SCvx loop again FROM THE CURRENT ITERATE: every active trajectory keeps its iterate and its tiles and gets rk = 100,
 * cost = Inf, iter = 0 (the values of create_initial, rocketland.jl:38), status RUNNING and live = 1; failed trajectories stay
 * frozen; the conic solver's warm-start state is dropped.  On the device, asynchronous.  The first step after it is accepted
 * through the reference's rho = NaN branch.  A replan may land in another local optimum than a solve from the straight-line guess
 * under the same back-offs. */
int scvx_batch_replan(scvx_batch *b);

/* ---- path-constraint back-offs: mass, glide slope, tilt, rate (no counterpart in the reference) --------------------------------
 * Before these, back-offs existed for the thrust band only; the covariance analysis writes the per-node 1 sigma of four more path
 * functions (psig, SCVX_PSIG_MASS .. SCVX_PSIG_RATE), and these calls bring them back into the conic solve.  Per trajectory and node
 * pm [B][K+1][SCVX_PMARG_N] = (mass, glide, tilt, rate), read by the conic solve alone:
 *     m_k            >= mdry + pm[k][MASS]                      k = 1..K
 *     |(r2, r3)_k|   <= r1_k / tan(gammaGs) - pm[k][GLIDE]      k = 0..K-1
 *     |(q2, q3)_k|   <= sqcm - pm[k][TILT]                      k = 0..K-1      (sqcm = sqrt((1 - cos thetaMax) / 2))
 *     |w_k|          <= omMax - pm[k][RATE]                     k = 0..K-1
 * Every conic solve of the batch reads them; the discretisation, the trust-region update, the flight check, the tracking, covariance
 * and navigation calls keep auditing against the true constants, so a margined plan shows its headroom at the nodes (the audit's tilt
 * function at a node is below minus that node's back-off, and so on; a report's G_TILT is a maximum over ALL its samples, node 0 --
 * which has no sigma and so gets no back-off from the covariance -- and the stretches between nodes included), and psig is what it
 * was.  With none set, all of them zero, or set and cleared, every result is bitwise that of a batch that never had any (of the same
 * build of the library: against a build from before these calls, device results agree to the solver's tolerance, not bit for bit).
 * The entries: finite and >= 0; tilt < sqcm, rate < omMax, mass < mwet - mdry; an entry whose node has no row must be 0 (glide, tilt
 * and rate at node K, mass at node 0), and so must glide and rate at node 0, where r and w are fixed: a back-off there either does
 * nothing or makes the subproblem infeasible.  Tilt at node 0 is allowed (q_0 is free).  Anything else is SCVX_ERR_ARG and leaves the
 * batch as it was.  pm is a host array; NULL clears.  Setting or clearing drops the conic solver's warm-start state and the
 * reuse_inactive_tr shortcut, as scvx_batch_set_thrust_margins does.  scvx_batch_init clears them, scvx_batch_reset keeps them, and
 * like the thrust ones they ARE part of a checkpoint that the caller must carry (scvx_batch_get_path_margins reads them: zeros when
 * none are set).
 * OUT OF SCOPE: back-offs of the gimbal cone, the dynamic-pressure cone and the fin cone (psig has no column for them), and back-offs
 * on the constraints of the ESTIMATE.  Back-offs taken from the navigation analysis exist: scvx_batch_margins_from_nav below. */
#define SCVX_PMARG_N 4
#define SCVX_PMARG_MASS 0
#define SCVX_PMARG_GLIDE 1
#define SCVX_PMARG_TILT 2
#define SCVX_PMARG_RATE 3
int scvx_batch_set_path_margins(scvx_batch *b, const double *pm);
int scvx_batch_get_path_margins(scvx_batch *b, double *pm);
/* scvx_batch_thrust_margins_from_cov for any subset of the five constraints: one covariance launch on the batch's own tiles, then one
 * small kernel that writes min(nsigma s(k), cap width_k) for the constraints selected in `which` and leaves the others as they are
 * (a batch without path back-offs has zeros there).  Widths: Tmax - Tmin (thrust, lo_k = hi_k), mwet - mdry (mass), sqcm (tilt),
 * omMax (rate) and max(xbar_k[1], 0) / tan(gammaGs) of the current iterate (glide: the tightened cone always contains its axis).
 * The entries that must be 0 (above) are written as 0; a trajectory with a NaN in a selected psig column gets zeros there.
 * The glide s(k) is that of the audit's function tan(gammaGs) |(r2, r3)_k| - r1_k (SCVX_PSIG_GLIDE), while the back-off is subtracted from
 * r1_k / tan(gammaGs): n s(k) of back-off buys n tan(gammaGs) sigma of N_GLIDE.
 * Arguments and refusals as scvx_batch_thrust_margins_from_cov, which is this call with which = SCVX_MARGIN_THRUST and leaves the
 * path back-offs alone; SCVX_ERR_ARG also for which = 0 or an unknown bit.  The limits are the same: FIRST ORDER, only as good as
 * Sigma_k, and s(k) depends on the plan. */
#define SCVX_MARGIN_THRUST 1u
#define SCVX_MARGIN_MASS 2u
#define SCVX_MARGIN_GLIDE 4u
#define SCVX_MARGIN_TILT 8u
#define SCVX_MARGIN_RATE 16u
#define SCVX_MARGIN_ALL 31u
int scvx_batch_margins_from_cov(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0,
                                const double *w14, double nsigma, double cap, unsigned which, double *psig);
/* scvx_batch_margins_from_cov with the s(k) of the NAVIGATION analysis of the batch's current accepted iterate: the law is fed an
 * estimate, and under navigation errors the truth disperses more than scvx_cov_path_sigma_f64 says (with N0 = S0 and position alone
 * measured, s_T is about twice as large on the golden plans: a plan backed off 3 sigma by the covariance analysis keeps 1.3).  One
 * navigation launch (scvx_nav_path_sigma_f64) on the batch's own tiles (double or float) and gains, then the same small kernel:
 * the same widths and caps, the same forced zeros, zeros for a trajectory with a NaN in a selected psig column; the constraints
 * that are not selected stay as they are (zeros on a batch that had no path back-offs).  N0 [B][14][14], H [m][14] and rm [m] are
 * host arrays as in scvx_batch_nav_cov; everything else, psig = NULL and the dropped warm-start state included, as
 * scvx_batch_margins_from_cov.  Every check comes before anything is enqueued: SCVX_ERR_ARG for what that call refuses and for what
 * scvx_batch_nav_cov refuses of N0, m, H and rm, and the batch and its back-offs are then as they were.
 * Limits: FIRST ORDER about the plan; Kf is the optimal gain for the stated model (a mismodelled filter disperses more); no
 * measurement at node K, and no sigma at node 0 (the handover is where the plan starts: no back-off there); the glide back-off
 * buys tan(gammaGs) times as many sigma, as above; s(k) depends on the plan, so one round reaches about 2.7 - 3 sigma of headroom
 * under the navigation report for nsigma = 3 rather than exactly n (repeat the round to tighten it). */
int scvx_batch_margins_from_nav(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0,
                                const double *N0, int m, const double *H, const double *rm, const double *w14, double nsigma,
                                double cap, unsigned which, double *psig);

/* The batch-level analyses with VEHICLE ERRORS as consider parameters ("VEHICLE ERRORS in the first-order analyses" above): each takes
 * the argument list of the call it extends followed by const double *sp6 (host, the six standard deviations; there is no mu).  Each
 * runs scvx_vehicle_tiles_f64 on the batch's current accepted iterate in front of the analysis, on the same stream: nothing returns
 * to the host between that launch and the analysis or the back-off kernel.  SCVX_ERR_ARG as the call extended and as
 * scvx_cov_vehicle_f64 for sp6. */
int scvx_batch_cov_veh(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0, const double *w14,
                       double *report, double *sig, double *covK, double *cov, const double *sp6);
int scvx_batch_nav_cov_veh(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0,
                           const double *N0, int m, const double *H, const double *rm, const double *w14, double *report,
                           double *navrep, double *sig, double *navsig, double *kf, double *joint, const double *sp6);
int scvx_batch_margins_from_cov_veh(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0,
                                    const double *w14, double nsigma, double cap, unsigned which, double *psig, const double *sp6);
int scvx_batch_margins_from_nav_veh(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0,
                                    const double *N0, int m, const double *H, const double *rm, const double *w14, double nsigma,
                                    double cap, unsigned which, double *psig, const double *sp6);

/* scvx_cov_clamp_f64 on the batch's current accepted iterate, its own derivative tiles (float tiles are widened on load) and the gains
 * of q14 / rNU / qf14, as scvx_batch_cov: S0, w14, band2 and every output are host arrays, and every output may be NULL.  The batch is
 * left untouched.  SCVX_ERR_ARG as scvx_batch_cov and for the band2 that scvx_cov_clamp_f64 refuses. */
int scvx_batch_cov_clamp(scvx_batch *b, const double *q14, const double *rNU, const double *qf14, const double *S0, const double *w14,
                         const double *band2, double *report, double *satrep, double *mean, double *sig, double *covK, double *cov,
                         double *satk);

/* ---- segment audit: the plan's path constraints segment by segment, and back-offs from it (no counterpart in the reference) ------
 * The flight check keeps ONE maximum per column over the whole flight.  In SCVX_FLIGHT_PLAN mode the state restarts at every planned
 * node, so the K segments of a plan are independent: this call audits each on a lane of its own (one lane per (b, k), the integrator,
 * the hold, the nsub + 1 sample points and the path functions of scvx_flight_check_f64) and says WHERE a constraint fails between
 * the nodes.  seg [B][K][SCVX_SEG_N], per segment k (from node k to node k + 1):
 *   DEFECT   |x_end - x[k+1]|_inf, the scvx_propagate_f64 defect of the segment;
 *   G_MASS .. G_FIN   the maxima of the flight report's path functions over the segment's nsub + 1 samples, in the report's order
 *            (G_DP / G_FIN: -inf where the model has no such constraint);
 *   QNORM    max of | |q| - 1 |.
 * A non-finite sampled state makes the DEFECT, the state G_* and the QNORM of THAT segment NaN and cannot disturb another segment (a
 * non-finite node k is also what segment k - 1 ends against: that one shows it in its DEFECT alone).
 * report [B][SCVX_FLIGHT_NREP] or NULL: the SCVX_FLIGHT_PLAN report, reduced on the device from seg in a fixed order (two launches
 * agree bit for bit): GAP and every G_* / QNORM are bitwise the maxima over k of seg's columns, the MISS_* and MASS_END are those of the
 * last segment's end (MISS_* NaN when GAP is).  nsub = 0 takes the context's (scvx_set_nsub).  dt = 1 / (K + 1); asynchronous on the
 * context's stream.  SCVX_ERR_ARG for nsub outside [1, 1000], B < 1, K != the problem's K, a null x / u / sigma / seg.
 * Limits: the samples are the substep boundaries only (RK stage points and the stretch between two samples are not looked at; on the
 * golden plans nsub = 40 moves the figures of nsub = 10 in the third digit). */
#define SCVX_SEG_N 11
#define SCVX_SEG_DEFECT 0
#define SCVX_SEG_G_MASS 1
#define SCVX_SEG_G_GLIDE 2
#define SCVX_SEG_G_TILT 3
#define SCVX_SEG_G_RATE 4
#define SCVX_SEG_G_TMAX 5
#define SCVX_SEG_G_TMIN 6
#define SCVX_SEG_G_GIMBAL 7
#define SCVX_SEG_G_DP 8
#define SCVX_SEG_G_FIN 9
#define SCVX_SEG_QNORM 10
int scvx_segment_audit_f64(scvx_ctx *ctx, int B, int K, const double *x_dev, const double *u_dev, const double *sigma_dev, int nsub,
                           double *seg_dev, double *report_dev);
int scvx_segment_audit_f64_host(scvx_ctx *ctx, int B, int K, const double *x, const double *u, const double *sigma, int nsub,
                                double *seg, double *report);
/* The same on the batch's current accepted iterate; seg and report are host arrays (report may be NULL).  The batch is left untouched. */
int scvx_batch_segment_audit(scvx_batch *b, int nsub, double *seg, double *report);
/* Back-offs from the audit, on the device: the segment audit of the batch's current accepted iterate, then one small kernel on the
 * batch's own back-off buffers.  Per node k and constraint selected in `which` (SCVX_MARGIN_*), with G the constraint's seg column,
 *     e_k = max(excess(k - 1), excess(k)),  excess = G where G > tol, else 0       (node 0: segment 0 alone, node K: segment K - 1)
 *     new = min(old + gain e_k, cap width_k)
 * with the widths and the forced zeros of scvx_batch_margins_from_cov (glide, tilt and rate 0 at node K, glide and rate 0 at node 0,
 * the glide width from the current iterate).  SCVX_MARGIN_THRUST reads G_TMIN and raises lo alone (|u| is convex along a hold, so hi
 * needs nothing between the nodes); GLIDE, TILT and RATE act on pm.  SCVX_MARGIN_MASS is refused: mass is monotone, a bound held at
 * the nodes holds between them.  The back-offs ACCUMULATE: the audit is against the true constants, so back-offs that are already
 * there (scvx_batch_margins_from_cov, a previous round) show as negative G and nothing is added on top of them; a batch without
 * back-offs starts from zeros.  A trajectory with a NaN in a selected seg column is left as it is.  The warm-start state is dropped,
 * as by the other setters.  seg [B][K][SCVX_SEG_N] (host, or NULL: then nothing returns to the host and the call is asynchronous).
 * SCVX_ERR_ARG for gain not finite or < 1, tol < 0, cap outside (0, 0.5), which = 0, an unknown bit or SCVX_MARGIN_MASS, a bad nsub.
 * Limits: gain is a starting point (the violation can move to a neighbouring segment of the next plan: repeat the round); the
 * dynamic-pressure, gimbal and fin cones are audited but have no back-off. */
int scvx_batch_audit_margins(scvx_batch *b, int nsub, unsigned which, double gain, double tol, double cap, double *seg);

/* Running totals over every solve_step enqueued since the last call with reset != 0 (what a timed region really executed):
 * out8 = {trajectory-steps, conic solves run, interior-point iterations summed over them, solves that were warm-started,
 * solves skipped by reuse_inactive_tr, steps REJECTED, steps that failed (SOLVER / NONFINITE / INFEASIBLE), steps that ended
 * CONVERGED}.  Synchronises the stream. */
int scvx_batch_get_step_stats(scvx_batch *b, double *out8, int reset);

/* ---- per-kernel device time of the solve_step chain (HIP events on the stream a step, or a part of it, runs on) ------ */
int scvx_batch_set_profiling(scvx_batch *b, int enable);
/* ms[5] = {socp (K4), propagate (K2), tr_update (K5), linearize (K1), glue (K3: candidate/unpack)}
 * over the `steps` solve_steps enqueued since the last call; synchronises and resets.  Steps on the context's stream: the sum of
 * each class's intervals, and the classes add up to the steps.  Steps that ran as parts on side streams: per class the length of
 * the UNION of its intervals over all parts (socp = the time during which some conic solve was running); the parts overlap, so
 * the classes do not add up to the steps. */
int scvx_batch_get_profile(scvx_batch *b, double *ms, int64_t *steps);

/* ---- multi-GPU: the single exchange step of the path (no counterpart in the reference) ---- */
/* One process per GPU, one context per process, contiguous shards of the Monte-Carlo batch; nothing inside the
 * SCvx iteration communicates.  The final records are all-gathered over RCCL (xGMI inside a node) on the
 * context's stream.  Bootstrap as with NCCL: rank 0 calls scvx_comm_unique_id, the host language ships the
 * SCVX_COMM_ID_BYTES to every rank by whatever channel it has, every rank calls scvx_comm_create. */
#define SCVX_COMM_ID_BYTES 128
/* Non-collective: 0 when the RCCL library can be bound in this process (SCVX_RCCL_LIB overrides the soname), else
 * SCVX_ERR_COMM.  Ranks exchange this BEFORE scvx_comm_create, whose ncclCommInitRank blocks until every rank arrives. */
int scvx_comm_probe(void);
int scvx_comm_unique_id(void *id_out /* SCVX_COMM_ID_BYTES */);
int scvx_comm_create(scvx_ctx *ctx, const void *unique_id, int rank, int world);
int scvx_comm_destroy(scvx_ctx *ctx);
int scvx_comm_info(const scvx_ctx *ctx, int *rank, int *world); /* world = 0: no communicator */
/* out_dev [world][B][(K+1)*(14+NU)+1]: every rank's trajectory records (all ranks hold the same B), asynchronous on the
 * context's stream; status_out_dev / iters_out_dev [world][B] (either may be NULL). */
int scvx_allgather_trajectories(scvx_batch *b, double *out_dev);
int scvx_allgather_status(scvx_batch *b, int32_t *status_out_dev, int32_t *iters_out_dev);
/* raw collectives on the context's communicator and stream (count elements per rank) */
int scvx_allgather_f64(scvx_ctx *ctx, const double *send_dev, double *recv_dev, int64_t count);
int scvx_allgather_i32(scvx_ctx *ctx, const int32_t *send_dev, int32_t *recv_dev, int64_t count);

/* ---- the conic subproblem alone (replaces MOI.optimize!, rocketland.jl:271) ------------------ */
/* Solves the trust-region SOCP at the batch's current (about, dynam, rk).  sol [B][(K+1)*(14+NU)+1] as
 * the trajectory layout but sigma slot holds sigma + dsigma; nu [B][K][14] (nu_2..nu_{K+1}). */
int scvx_socp_solve(scvx_batch *b, double *sol, double *nu);

#ifdef __cplusplus
}
#endif
#endif /* SCVX_H */
