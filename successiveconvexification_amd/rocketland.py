"""Rocketland — the reference's SCvx driver API (rocketland.jl), one trajectory at a time, over the HIP path.

    create_initial(problem, cache) -> ProblemIteration            rocketland.jl:34-39
    run_iters(iprob, niters, cache) -> (trajectories, tfs)        rocketland.jl:420-430
    plot_solution_data(ip) / dump_solution(ip, path)              rocketland.jl:454-478 (the arrays plot_solution draws)
    solve_step(iteration, cache) -> (ProblemIteration, |nu|, dJ)  rocketland.jl:226-321
    solve_problem(iprob, cache) -> (ProblemIteration, cnu, cdel)  rocketland.jl:432-443
    fly(iteration, cache) -> FlightReport                         (new: open-loop flight + path audit of a plan)
    track(iteration, cache, dx0) -> FlightReport                  (new: closed-loop flight under LQR gains about the plan)
    covariance(iteration, cache, S0) -> CovReport                 (new: closed-loop covariance analysis of the tracked plan)
    robustify(iteration, cache, S0) -> (ProblemIteration, lo, hi) (new: replan under thrust back-offs taken from that analysis)
The recipe of rocketland.jl:26-32 reads the same here:
    cache = IntegratorCache(prob, ProbInfo.from_problem(prob), make_dynamics_module(...))
    pi = create_initial(prob, cache); pi, cnu, cdel = solve_step(pi, cache)
`ProblemIteration.model` holds the device batch (B = 1) instead of MOI handles; everything numeric runs in
libscvx_hip.so (batch.py is the batched form the GPU exists for).
"""
import numpy as np

from .batch import ScvxBatch
from .defns import DescentProblem, LinPoint, LinRes, ProblemIteration
from .dynamics import IntegratorCache


def _snapshot(problem, cache, batch) -> ProblemIteration:
    x, u, s = batch.trajectory()
    e, d = batch.linearization()
    rk, cost, it = batch.scalars()
    K = problem.K
    about = [LinPoint(x[0, k].copy(), u[0, k].copy()) for k in range(K + 1)]
    dynam = [LinRes(e[0, k].copy(), d[0, k].T.copy()) for k in range(K)]
    return ProblemIteration(problem, cache, float(s[0]), about, dynam, batch, int(it[0]), float(rk[0]), float(cost[0]))


def create_initial(problem: DescentProblem, linear_cache: IntegratorCache) -> ProblemIteration:
    batch = ScvxBatch(linear_cache, 1).init(None)
    return _snapshot(problem, linear_cache, batch)


def solve_step(iteration: ProblemIteration, linear_cache: IntegratorCache):
    batch = iteration.model
    st, nu, dj = batch.solve_step()
    if st[0] in (3, 4, 5):  # rocketland.jl:273-276
        raise RuntimeError("Non-optimal result %s exiting" % {3: "SLOW_PROGRESS", 4: "NUMERICAL_ERROR", 5: "INFEASIBLE"}[int(st[0])])
    return _snapshot(iteration.problem, linear_cache, batch), float(nu[0]), float(dj[0])


def solve_problem(iprob: DescentProblem, cache: IntegratorCache):
    prob = create_initial(iprob, cache)
    cnu = np.inf
    cdel = np.inf
    it = 1
    while (iprob.nuTol < cnu or iprob.delTol < cdel) and it < iprob.imax:
        prob, cnu, cdel = solve_step(prob, cache)
        it += 1
    return prob, cnu, cdel


def fly(iteration: ProblemIteration, cache: IntegratorCache = None, nsub=None, mode="shoot", dense=False):
    """Open-loop flight of an iterate's plan (`about`, `sigma`) and the audit of its path constraints between the nodes -- what the
    reference never does: its constraints hold at the nodes (rocketland.jl:136-209).  Returns a dynamics.FlightReport of one row."""
    from .dynamics import flight_check_batch
    cache = cache if cache is not None else iteration.cache
    x = np.stack([pt.state for pt in iteration.about])[None]
    u = np.stack([pt.control for pt in iteration.about])[None]
    return flight_check_batch(cache, x, u, np.array([float(iteration.sigma)]), nsub=nsub, mode=mode, dense=dense)


def track(iteration: ProblemIteration, cache: IntegratorCache = None, dx0=None, q=None, r=None, qf=None, nsub=None, clamp=False,
          dense=False):
    """Closed-loop flight of an iterate's plan from `about[0].state + dx0` (dx0 [14] or None) under the time-varying LQR gains about
    it (dynamics.track_gains_batch on the plan's own linearisation, dynamics.track_fly_batch).  A dynamics.FlightReport of one row."""
    from .dynamics import linearize_batch, track_fly_batch, track_gains_batch
    cache = cache if cache is not None else iteration.cache
    x = np.stack([pt.state for pt in iteration.about])[None]
    u = np.stack([pt.control for pt in iteration.about])[None]
    sigma = np.array([float(iteration.sigma)])
    _, deriv = linearize_batch(cache, x, u, sigma, 1.0 / x.shape[1])
    gain = track_gains_batch(cache, deriv, q, r, qf)
    d0 = None if dx0 is None else np.asarray(dx0, np.float64).reshape(1, 14)
    return track_fly_batch(cache, x, u, sigma, gain, d0, nsub=nsub, clamp=clamp, dense=dense)


def track_mc(iteration: ProblemIteration, cache: IntegratorCache = None, S0=None, samples=256, seed=0, w=None, q=None, r=None, qf=None,
             nsub=None, clamp=False, tol=0.0, dense=(), nav=None, quantiles=None, per_node=False, rng="host", independent=False,
             sample_lo=0, plan_lo=0, vehicle=None):
    """Sampled closed-loop dispersion of an iterate's plan tracked under the time-varying LQR gains about it: `samples` flights from
    Gaussian starts of covariance S0 ([14][14], or a [14] vector of standard deviations), with the per-segment process noise w as an
    impulse at the nodes (dynamics.track_gains_batch on the plan's own linearisation, dynamics.track_mc_batch).  A dynamics.McReport of
    one row.  nav = (N0, H, rm), navigation()'s model: the flights are flown on a navigation estimate (dynamics.track_mc_nav_batch on
    the same linearisation), a dynamics.McNavReport of one row.  quantiles, per_node and the dense name "pathv" as
    dynamics.track_mc_batch: order statistics over the samples, reduced on the device.  rng="device", independent, sample_lo and
    plan_lo as dynamics.track_mc_batch: the draws are made on the device.  vehicle = (mu, sp) (montecarlo.vehicle_errors) and the dense
    name "theta" as dynamics.track_mc_batch: per-flight vehicle errors."""
    from .dynamics import linearize_batch, track_gains_batch, track_mc_batch
    if S0 is None:
        raise ValueError("track_mc: S0 (the handover covariance) is required")
    cache = cache if cache is not None else iteration.cache
    x = np.stack([pt.state for pt in iteration.about])[None]
    u = np.stack([pt.control for pt in iteration.about])[None]
    sigma = np.array([float(iteration.sigma)])
    _, deriv = linearize_batch(cache, x, u, sigma, 1.0 / x.shape[1])
    gain = track_gains_batch(cache, deriv, q, r, qf)
    if nav is not None:
        from .dynamics import _nav_arg, track_mc_nav_batch
        n0, _, Hm, rv = _nav_arg(nav, 1)
        return track_mc_nav_batch(cache, x, u, sigma, deriv, gain, S0, n0, Hm, rv, samples, seed=seed, w=w, nsub=nsub, clamp=clamp,
                                  tol=tol, dense=dense, quantiles=quantiles, per_node=per_node, rng=rng, independent=independent,
                                  sample_lo=sample_lo, plan_lo=plan_lo, vehicle=vehicle)
    return track_mc_batch(cache, x, u, sigma, gain, S0, samples, seed=seed, w=w, nsub=nsub, clamp=clamp, tol=tol, dense=dense,
                          quantiles=quantiles, per_node=per_node, rng=rng, independent=independent, sample_lo=sample_lo, plan_lo=plan_lo,
                          vehicle=vehicle)


def covariance(iteration: ProblemIteration, cache: IntegratorCache = None, S0=None, w=None, q=None, r=None, qf=None, dense=False,
               vehicle=None, clamp=False, band=None):
    """Closed-loop covariance analysis of an iterate's plan tracked under the time-varying LQR gains about it, from the handover
    covariance S0 ([14][14], or a [14] vector of standard deviations) with the per-segment process noise w (dynamics.track_gains_batch
    on the plan's own linearisation, dynamics.cov_propagate_batch).  A dynamics.CovReport of one row.  vehicle = (mu, sp) of
    montecarlo.vehicle_errors, mu = 0: the vehicle errors as consider parameters (dynamics.vehicle_tiles_batch on the plan).
    clamp=True: the clamp-aware analysis by statistical linearisation, a dynamics.SatCovReport (band, dense: cov_propagate_batch's);
    not together with vehicle."""
    from .dynamics import cov_propagate_batch, linearize_batch, track_gains_batch, vehicle_tiles_batch
    if S0 is None:
        raise ValueError("covariance: S0 (the handover covariance) is required")
    if clamp and vehicle is not None:
        raise ValueError("clamp=True has no vehicle-error form: vehicle= must be None")
    cache = cache if cache is not None else iteration.cache
    x = np.stack([pt.state for pt in iteration.about])[None]
    u = np.stack([pt.control for pt in iteration.about])[None]
    sigma = np.array([float(iteration.sigma)])
    _, deriv = linearize_batch(cache, x, u, sigma, 1.0 / x.shape[1])
    gain = track_gains_batch(cache, deriv, q, r, qf)
    kw = {} if vehicle is None else dict(vehicle=vehicle, vtile=vehicle_tiles_batch(cache, x, u, sigma))
    if clamp or band is not None:
        kw.update(clamp=clamp, band=band)
    return cov_propagate_batch(cache, x, u, deriv, gain, S0, w, dense=dense, **kw)


def robustify(iteration: ProblemIteration, cache: IntegratorCache = None, S0=None, nsigma=3.0, rounds=1, cap=0.25, w=None, q=None,
              r=None, qf=None, constraints=("thrust",), nav=None, mc=None, vehicle=None):
    """Replan an iterate under back-offs of the thrust band taken from its own covariance analysis (ScvxBatch.robustify on the
    iterate's device batch): Tmin + n s_T(k) <= |u_k| <= Tmax - n s_T(k).  Returns (the new ProblemIteration, lo [K+1], hi [K+1]);
    raises like solve_step when the conic solve fails.  The limits are those of ScvxBatch.robustify.  constraints: any subset of
    ("thrust", "mass", "glide", "tilt", "rate") or "all"; the path back-offs that were used are iteration.model.path_margins().
    nav = (N0, H, rm): the back-offs come from the navigation analysis of the iterate (navigation()'s model), the law fed an estimate.
    mc = dict(p=, samples=, seed=, clamp=): they come from the sampled closed loop instead (ScvxBatch.margins_from_mc, its limits);
    with nav the flights are flown on the estimate.  vehicle = (mu, sp), mu = 0: the covariance or navigation path with the vehicle
    errors as consider parameters (ScvxBatch.robustify's keyword; not with mc, which has its own)."""
    if S0 is None:
        raise ValueError("robustify: S0 (the handover covariance) is required")
    cache = cache if cache is not None else iteration.cache
    batch = iteration.model
    st, it, nu, dj, lo, hi = batch.robustify(S0, nsigma=nsigma, rounds=rounds, cap=cap, w=w, q=q, r=r, qf=qf, constraints=constraints,
                                             nav=nav, mc=mc, vehicle=vehicle)
    if st[0] in (3, 4, 5):  # rocketland.jl:273-276
        raise RuntimeError("Non-optimal result %s exiting" % {3: "SLOW_PROGRESS", 4: "NUMERICAL_ERROR", 5: "INFEASIBLE"}[int(st[0])])
    return _snapshot(iteration.problem, cache, batch), lo[0], hi[0]


def harden(iteration: ProblemIteration, cache: IntegratorCache = None, constraints=("thrust", "glide", "tilt", "rate"), rounds=3, gain=1.5,
           tol=1e-7, restart="replan", nsub=None):
    """Replan an iterate under back-offs taken from its own segment audit until it holds its constraints between the nodes
    (ScvxBatch.harden on the iterate's device batch).  Returns (the new ProblemIteration, the dynamics.SegmentReport of its plan, the
    rounds used); raises like solve_step when the conic solve fails.  The limits are those of ScvxBatch.harden."""
    cache = cache if cache is not None else iteration.cache
    batch = iteration.model
    st, it, nu, dj, rep, used = batch.harden(constraints=constraints, rounds=rounds, gain=gain, tol=tol, restart=restart, nsub=nsub)
    if st[0] in (3, 4, 5):  # rocketland.jl:273-276
        raise RuntimeError("Non-optimal result %s exiting" % {3: "SLOW_PROGRESS", 4: "NUMERICAL_ERROR", 5: "INFEASIBLE"}[int(st[0])])
    return _snapshot(iteration.problem, cache, batch), rep, used


def navigation(iteration: ProblemIteration, cache: IntegratorCache = None, S0=None, N0=None, H=None, rm=None, w=None, q=None, r=None,
               qf=None, dense=False, vehicle=None, clamp=False):
    """Navigation-error covariance analysis of an iterate's plan flown on an estimate under the time-varying LQR gains about it: S0 the
    handover covariance of the truth, N0 that of the navigation error, H [m][14] and rm the measurement taken at every node but the
    last (H None: inertial propagation only), w the per-segment process noise (dynamics.track_gains_batch on the plan's own
    linearisation, dynamics.nav_cov_batch).  A dynamics.NavReport of one row.  vehicle = (mu, sp), mu = 0: as covariance()."""
    from .dynamics import linearize_batch, nav_cov_batch, track_gains_batch, vehicle_tiles_batch
    if clamp:
        raise ValueError("clamp=True: the clamp-aware analysis has no navigation form (covariance(clamp=True) feeds the law the truth)")
    if S0 is None or N0 is None:
        raise ValueError("navigation: S0 and N0 (the handover covariances of the truth and of the navigation error) are required")
    cache = cache if cache is not None else iteration.cache
    x = np.stack([pt.state for pt in iteration.about])[None]
    u = np.stack([pt.control for pt in iteration.about])[None]
    sigma = np.array([float(iteration.sigma)])
    _, deriv = linearize_batch(cache, x, u, sigma, 1.0 / x.shape[1])
    gain = track_gains_batch(cache, deriv, q, r, qf)
    kw = {} if vehicle is None else dict(vehicle=vehicle, vtile=vehicle_tiles_batch(cache, x, u, sigma))
    return nav_cov_batch(cache, x, u, deriv, gain, S0, N0, H, rm, w, dense=dense, **kw)


def run_iters(iprob: DescentProblem, niters: int, cache: IntegratorCache = None):
    """rocketland.jl:420-430: niters solve_steps, keeping the position history r[3][K+1] and sigma of every iterate
    (the reference's version calls 1-argument create_initial/solve_step that do not exist at HEAD; the cache is
    explicit here)."""
    cache = cache if cache is not None else IntegratorCache(iprob)
    ip = create_initial(iprob, cache)
    trjs, tfs = [], []
    for _ in range(niters):
        ip, _, _ = solve_step(ip, cache)
        tfs.append(ip.sigma)
        trjs.append(np.stack([pt.state[1:4] for pt in ip.about], axis=1))
    return trjs, tfs


# ---- plot_solution (rocketland.jl:454-478) without a plotting library ------------------------------------------------
def body_axis(q):
    """Dynamics.DCM(q) * [1, 0, 0] (dynamics.jl:29-44): first column of the body->inertial rotation, q scalar-first."""
    q0, q1, q2, q3 = (np.asarray(q, float)[..., i] for i in range(4))
    return np.stack([1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 + q0 * q3), 2 * (q1 * q3 - q0 * q2)], axis=-1)


def plot_solution_data(ip: ProblemIteration) -> dict:
    """Everything Rocketland.plot_solution computes before it calls Plots.jl, under the names it uses:
        xs [K+1][2] = (r_y, r_z), ys [K+1][2] = (r_up, r_up)      the two trajectory panels (layout = 2)
        xlims = (tmin, tmax), pmin, pmax                           its axis limits (tmin/tmax over r_up and r_y, pmin/pmax over r_up and r_z)
        thr [K+1] = |u| / Tmax                                      the throttle it prints
        dp [K+1] = (C(q) e1) . v / |v|                              the cos(angle of attack) it prints per node
        xls, yls [K+1][2][2]                                        the attitude tick of every node: from r to r + C(q) e1 / 3
    """
    X = np.stack([pt.state for pt in ip.about])
    U = np.stack([pt.control for pt in ip.about])
    up, ry, rz = X[:, 1], X[:, 2], X[:, 3]
    dv = body_axis(X[:, 7:11])
    v = X[:, 4:7]
    with np.errstate(invalid="ignore", divide="ignore"):
        dp = np.sum(dv * v, axis=1) / np.linalg.norm(v, axis=1)
    xls = np.stack([np.stack([ry, rz], 1), np.stack([ry + dv[:, 1] / 3, rz + dv[:, 2] / 3], 1)], axis=1)
    yls = np.stack([np.stack([up, up], 1), np.stack([up + dv[:, 0] / 3, up + dv[:, 0] / 3], 1)], axis=1)
    return dict(xs=np.stack([ry, rz], 1), ys=np.stack([up, up], 1),
                xlims=(float(min(up.min(), ry.min())), float(max(up.max(), ry.max()))),
                pmin=float(min(up.min(), rz.min())), pmax=float(max(up.max(), rz.max())),
                thr=np.linalg.norm(U, axis=1) / ip.problem.Tmax, dp=dp, xls=xls, yls=yls, sigma=float(ip.sigma))


def dump_solution(ip: ProblemIteration, path: str) -> str:
    """Writes plot_solution_data(ip) to `path`: .npz (all arrays) or .csv (one row per node: k, r_up, r_y, r_z, thr, dp and
    the attitude tick end points) -- enough to redraw the reference's figure with any tool."""
    d = plot_solution_data(ip)
    if path.endswith(".npz"):
        np.savez(path, **{k: np.asarray(v) for k, v in d.items()})
    else:
        K1 = d["xs"].shape[0]
        tab = np.column_stack([np.arange(K1), d["ys"][:, 0], d["xs"][:, 0], d["xs"][:, 1], d["thr"], d["dp"],
                               d["yls"][:, 1, 0], d["xls"][:, 1, 0], d["xls"][:, 1, 1]])
        np.savetxt(path, tab, delimiter=",", comments="",
                   header="k,r_up,r_y,r_z,thr,cos_aoa,tick_up,tick_y,tick_z   # sigma=%.17g xlims=%s" % (d["sigma"], d["xlims"]))
    return path
