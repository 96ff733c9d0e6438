"""Batched SCvx driver over libscvx_hip.so (new relative to the reference, which solves one trajectory
serially): B independent DescentProblem instances that differ in their initial condition, advanced by
Rocketland.solve_step in lock-step on one GPU; `solve_sharded` spreads a Monte-Carlo batch over the GPUs
of a node, one process per GPU, and all-gathers the final trajectories over RCCL."""
import ctypes as C
import numpy as np

from . import _calls, _lib
from .dynamics import IntegratorCache

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)


def _p(a):
    return a.ctypes.data_as(_dp)


def _pi(a):
    return a.ctypes.data_as(_ip)


STATUS = {0: "converged", 1: "running", 2: "rejected", 3: "solver", 4: "nonfinite", 5: "infeasible"}


class ScvxBatch:
    """The batched ProblemIteration (master.jl:122-134) living in HBM."""

    def __init__(self, cache: IntegratorCache, B: int, tol: float = None, max_iter: int = None, refine: int = None,
                 accept_tol: float = None, reuse_inactive_tr: bool = None, warm_start: bool = None, retries: int = None):
        self.cache = cache
        self.B = int(B)
        self.K = cache.problem.K
        self.nu = cache.nu                               # control_dim: 3, or 5 with the fin extension
        self.nrec = (self.K + 1) * (14 + self.nu) + 1
        self._L = cache._L
        h = C.c_void_p()
        _lib.check(cache.handle, self._L.scvx_batch_create(cache.handle, self.B, C.byref(h)), "scvx_batch_create")
        self.handle = h
        if any(v is not None for v in (tol, max_iter, refine, accept_tol, reuse_inactive_tr, warm_start, retries)):
            o = _lib.ScvxSolverOpts()
            self._L.scvx_solver_default_opts(C.byref(o))
            if tol is not None:
                o.tol = tol
                o.accept_tol = tol   # the default band is empty (accept_tol = tol), whatever tol is
            if max_iter is not None:
                o.max_iter = max_iter
            if refine is not None:
                o.refine = refine
            if accept_tol is not None:
                o.accept_tol = accept_tol
            if reuse_inactive_tr is not None:
                o.reuse_inactive_tr = 1 if reuse_inactive_tr else 0
            if warm_start is not None:
                o.warm_start = 1 if warm_start else 0
            if retries is not None:
                o.retries = int(retries)   # scvx_solver_opts.retries: the ladder of step rules behind a failed solve (0 = one attempt)
            _lib.check(cache.handle, self._L.scvx_batch_set_solver(h, C.byref(o)), "scvx_batch_set_solver")

    def _chk(self, rc, what):
        _lib.check(self.cache.handle, rc, what)

    # create_initial (rocketland.jl:34-39) for every trajectory
    def init(self, ic=None):
        if ic is not None:
            ic = np.ascontiguousarray(ic, np.float64)
            if ic.shape != (self.B, 6):
                raise ValueError("ic must be [B][6] = (rIi, vIi)")
        self._chk(self._L.scvx_batch_init(self.handle, _p(ic) if ic is not None else None), "scvx_batch_init")
        return self

    def init_threedof(self, ic=None, **opts):
        """create_initial from FirstRound.solve_initial (initial_solve.jl:17-110) instead of the straight line: the 3-DoF
        landing SOCP is solved on the device for every trajectory; those whose solve is optimal start from its LinPoints,
        the others keep the straight line.  Returns the 3-DoF solver statuses [B] (0 = optimal)."""
        from .first_round import threedof_opts
        if ic is not None:
            ic = np.ascontiguousarray(ic, np.float64)
            if ic.shape != (self.B, 6):
                raise ValueError("ic must be [B][6] = (rIi, vIi)")
        o = threedof_opts(self._L, **opts)
        st3 = np.zeros(self.B, np.int32)
        self._chk(self._L.scvx_batch_init_threedof(self.handle, _p(ic) if ic is not None else None, C.byref(o), _pi(st3)),
                  "scvx_batch_init_threedof")
        return st3

    def reset(self):
        """create_initial again on the device for the same initial conditions (asynchronous)."""
        self._chk(self._L.scvx_batch_reset(self.handle), "scvx_batch_reset")
        return self

    # solve_step (rocketland.jl:226-321)
    def solve_step(self):
        st = np.zeros(self.B, np.int32)
        nu = np.zeros(self.B)
        dj = np.zeros(self.B)
        self._chk(self._L.scvx_solve_step(self.handle, _pi(st), _p(nu), _p(dj)), "scvx_solve_step")
        return st, nu, dj

    def solve_step_async(self):
        self._chk(self._L.scvx_solve_step_async(self.handle), "scvx_solve_step_async")

    # solve_problem (rocketland.jl:432-443)
    def solve(self):
        st = np.zeros(self.B, np.int32)
        it = np.zeros(self.B, np.int32)
        nu = np.zeros(self.B)
        dj = np.zeros(self.B)
        self._chk(self._L.scvx_solve(self.handle, _pi(st), _pi(it), _p(nu), _p(dj)), "scvx_solve")
        return st, it, nu, dj

    def socp_solve(self):
        """The conic subproblem alone at the current iterate: returns (x, u, sigma_new, nu)."""
        sol = np.zeros((self.B, self.nrec))
        nu = np.zeros((self.B, self.K, 14))
        self._chk(self._L.scvx_socp_solve(self.handle, _p(sol), _p(nu)), "scvx_socp_solve")
        x, u, s = self._split(sol)
        return x, u, s, nu

    def _split(self, rec):
        K, B = self.K, self.B
        nx = (K + 1) * 14
        return (rec[:, :nx].reshape(B, K + 1, 14).copy(), rec[:, nx:nx + (K + 1) * self.nu].reshape(B, K + 1, self.nu).copy(),
                rec[:, -1].copy())

    def trajectory(self):
        rec = np.zeros((self.B, self.nrec))
        self._chk(self._L.scvx_batch_get_trajectory(self.handle, _p(rec)), "scvx_batch_get_trajectory")
        return self._split(rec)

    def trajectory_record(self):
        rec = np.zeros((self.B, self.nrec))
        self._chk(self._L.scvx_batch_get_trajectory(self.handle, _p(rec)), "scvx_batch_get_trajectory")
        return rec

    def set_trajectory(self, x, u, sigma):
        rec = np.concatenate([np.asarray(x, float).reshape(self.B, -1), np.asarray(u, float).reshape(self.B, -1),
                              np.asarray(sigma, float).reshape(self.B, 1)], axis=1)
        rec = np.ascontiguousarray(rec)
        assert rec.shape == (self.B, self.nrec)
        self._chk(self._L.scvx_batch_set_trajectory(self.handle, _p(rec)), "scvx_batch_set_trajectory")

    def trajectory_dev(self):
        ptr = C.c_void_p()
        n = C.c_int64()
        self._chk(self._L.scvx_batch_trajectory_dev(self.handle, C.byref(ptr), C.byref(n)), "scvx_batch_trajectory_dev")
        return ptr.value, n.value

    def linearization(self):
        e = np.zeros((self.B, self.K, 14))
        d = np.zeros((self.B, self.K, 14 + 2 * self.nu + 1, 14))
        self._chk(self._L.scvx_batch_get_linearization(self.handle, _p(e), _p(d)), "scvx_batch_get_linearization")
        return e, d

    def set_linearization_f32(self, on=True):
        """Keep the derivative tiles in float (double arithmetic in K1, rounded at the store; the conic solve widens on load
        and stays double): the mixed-precision form of BASELINE configs[3-4].  Re-linearises an initialised batch."""
        self._chk(self._L.scvx_batch_set_linearization_f32(self.handle, 1 if on else 0), "scvx_batch_set_linearization_f32")
        return self

    def scalars(self):
        rk = np.zeros(self.B)
        cost = np.zeros(self.B)
        it = np.zeros(self.B, np.int32)
        self._chk(self._L.scvx_batch_get_scalars(self.handle, _p(rk), _p(cost), _pi(it)), "scvx_batch_get_scalars")
        return rk, cost, it

    def set_scalars(self, rk=None, cost=None, it=None):
        rk = None if rk is None else np.ascontiguousarray(np.broadcast_to(np.asarray(rk, float), (self.B,)))
        cost = None if cost is None else np.ascontiguousarray(np.broadcast_to(np.asarray(cost, float), (self.B,)))
        it = None if it is None else np.ascontiguousarray(np.broadcast_to(np.asarray(it, np.int32), (self.B,)))
        self._chk(self._L.scvx_batch_set_scalars(self.handle, _p(rk) if rk is not None else None,
                                                 _p(cost) if cost is not None else None,
                                                 _pi(it) if it is not None else None), "scvx_batch_set_scalars")

    def flags(self):
        """(status, active, live) per trajectory — with trajectory_record() and scalars() the full checkpoint."""
        st = np.zeros(self.B, np.int32)
        ac = np.zeros(self.B, np.int32)
        lv = np.zeros(self.B, np.int32)
        self._chk(self._L.scvx_batch_get_flags(self.handle, _pi(st), _pi(ac), _pi(lv)), "scvx_batch_get_flags")
        return st, ac, lv

    def set_flags(self, status=None, active=None, live=None):
        a = [None if v is None else np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.int32), (self.B,)))
             for v in (status, active, live)]
        self._chk(self._L.scvx_batch_set_flags(self.handle, *[_pi(v) if v is not None else None for v in a]),
                  "scvx_batch_set_flags")

    def solver_stats(self):
        st = np.zeros(self.B, np.int32)
        it = np.zeros(self.B, np.int32)
        merit = np.zeros(self.B)
        pobj = np.zeros(self.B)
        self._chk(self._L.scvx_batch_get_solver_stats(self.handle, _pi(st), _pi(it), _p(merit), _p(pobj)),
                  "scvx_batch_get_solver_stats")
        return st, it, merit, pobj

    def step_stats(self, reset: bool = True):
        """Totals over the solve_steps enqueued since the last reset (scvx_batch_get_step_stats); synchronises."""
        o = np.zeros(8)
        self._chk(self._L.scvx_batch_get_step_stats(self.handle, _p(o), 1 if reset else 0), "scvx_batch_get_step_stats")
        return dict(zip(("traj_steps", "solves", "ipm_iters", "warm_started", "skipped", "rejected", "failed", "converged"), o.tolist()))

    def flight_check(self, nsub=None, mode="shoot", dense=False):
        """Fly the batch's current accepted iterate open loop and audit its path constraints between the nodes
        (scvx_batch_flight_check): a dynamics.FlightReport.  The batch is left untouched."""
        from .dynamics import FlightReport, _flight_mode
        rep = np.empty((self.B, _lib.FLIGHT_NREP))
        xfly = np.empty((self.B, self.K + 1, 14)) if dense else None
        self._chk(self._L.scvx_batch_flight_check(self.handle, int(nsub or 0), int(_flight_mode(mode)), _p(rep),
                                                  _p(xfly) if dense else None), "scvx_batch_flight_check")
        return FlightReport(rep, xfly, mode)

    def track_gains(self, q=None, r=None, qf=None, cost=False):
        """LQR gains about the batch's current accepted iterate from its own derivative tiles (scvx_batch_track_gains; weights as
        dynamics.track_gains_batch): gain [B][K][nu][14+nu], with cost=True also p0 [B][14+nu][14+nu].  The batch is left untouched."""
        from .dynamics import _track_weights
        nu = self.cache.nu
        qv, rv, qfv = _track_weights(nu, q, r, qf)
        gain = np.empty((self.B, self.K, nu, 14 + nu))
        p0 = np.empty((self.B, 14 + nu, 14 + nu)) if cost else None
        self._chk(self._L.scvx_batch_track_gains(self.handle, _p(qv), _p(rv), _p(qfv), _p(gain), _p(p0) if cost else None),
                  "scvx_batch_track_gains")
        return (gain, p0) if cost else gain

    def track(self, dx0=None, q=None, r=None, qf=None, nsub=None, clamp=False, dense=False, nav=None):
        """Fly the batch's current accepted iterate closed loop under its LQR gains from x[0] + dx0 (scvx_batch_track_fly): a
        dynamics.FlightReport of mode "track" (dense: xfly and ufly).  nav [B][K][14]: the law is fed an estimate whose error at
        node k is nav[:, k] (scvx_batch_track_fly_nav); None: the true state.  The batch is left untouched."""
        from .dynamics import FlightReport, _track_weights
        nu = self.cache.nu
        qv, rv, qfv = _track_weights(nu, q, r, qf)
        if dx0 is not None:
            dx0 = np.ascontiguousarray(dx0, np.float64)
            if dx0.shape != (self.B, 14):
                raise ValueError("shape mismatch: dx0 [B][14]")
        rep = np.empty((self.B, _lib.FLIGHT_NREP))
        xfly = np.empty((self.B, self.K + 1, 14)) if dense else None
        ufly = np.empty((self.B, self.K + 1, nu)) if dense else None
        if nav is not None:
            nav = np.ascontiguousarray(nav, np.float64)
            if nav.shape != (self.B, self.K, 14):
                raise ValueError("shape mismatch: nav [B][K][14]")
            self._chk(self._L.scvx_batch_track_fly_nav(self.handle, _p(qv), _p(rv), _p(qfv), _p(dx0) if dx0 is not None else None, _p(nav),
                                                       int(nsub or 0), _lib.TRACK_CLAMP if clamp else 0, _p(rep),
                                                       _p(xfly) if dense else None, _p(ufly) if dense else None),
                      "scvx_batch_track_fly_nav")
            return FlightReport(rep, xfly, "track", ufly)
        self._chk(self._L.scvx_batch_track_fly(self.handle, _p(qv), _p(rv), _p(qfv), _p(dx0) if dx0 is not None else None,
                                               int(nsub or 0), _lib.TRACK_CLAMP if clamp else 0, _p(rep),
                                               _p(xfly) if dense else None, _p(ufly) if dense else None), "scvx_batch_track_fly")
        return FlightReport(rep, xfly, "track", ufly)

    def track_mc(self, S0, samples=256, seed=0, w=None, q=None, r=None, qf=None, nsub=None, clamp=False, tol=0.0, dense=(), draws=None,
                 nav=None, quantiles=None, per_node=False, rng="host", independent=False, sample_lo=0, plan_lo=0, vehicle=None):
        """Sampled closed-loop dispersion of the batch's current accepted iterate under its LQR gains: `samples` flights per plan on
        the device, one dynamics.McReport row per plan (scvx_batch_track_mc; S0 -- a [14] vector of standard deviations, one [14][14]
        or [B][14][14] --, seed, w, clamp, tol, dense and draws as dynamics.track_mc_batch, weights as track_gains).  The batch is left
        untouched.  nav = (N0, H, rm), the model of navigation(): the flights are flown on a navigation estimate whose error is
        generated per flight on the device from the filter gains of that analysis (scvx_batch_track_mc_nav; dense and draws as
        dynamics.track_mc_nav_batch): a dynamics.McNavReport.  quantiles (probabilities), per_node and the dense name "pathv" as
        dynamics.track_mc_batch: order statistics of the flight columns and of the per-node path functions, reduced on the device
        (scvx_batch_track_mc_q / scvx_batch_track_mc_nav_q); at their defaults the call is the one it was.  rng="device", independent,
        sample_lo and plan_lo as dynamics.track_mc_batch: the lanes make the draws, per plan if asked (scvx_batch_track_mc_rng /
        scvx_batch_track_mc_nav_rng); rng="host" is the call it was.  vehicle = (mu, sp) and the dense name "theta" as
        dynamics.track_mc_batch: per-flight vehicle errors (scvx_batch_track_mc_veh / scvx_batch_track_mc_nav_veh); None is the call it
        was."""
        from .dynamics import _mc_call, _mc_inputs, _mc_keywords, _mc_nav_inputs, _nav_arg
        rg, vh, mq = _mc_keywords(rng, draws, independent, seed, sample_lo, plan_lo, vehicle, dense, quantiles, per_node)
        f = self._record(q, r, qf)
        f.update(nsub=nsub or 0, flags=_lib.TRACK_CLAMP if clamp else 0, tol=tol)
        if nav is not None:
            n0, m, Hm, rmv = _nav_arg(nav, self.B)
            c0, cn, n0, xi0, eta, xin, nud, wv = _mc_nav_inputs(S0, n0, self.B, self.K, m, samples, seed, w, draws, sample_lo,
                                                                rg is not None)
            f.update(C0=c0, xi0=xi0, eta=eta, w14=wv, N0=n0, CN=cn, xin=xin, nud=nud, m=m, H=Hm, rm=rmv)
        else:
            c0, xi0, eta, sw = _mc_inputs(S0, self.B, self.K, samples, seed, w, draws, sample_lo, rg is not None)
            f.update(C0=c0, xi0=xi0, eta=eta, sw14=sw, reserved=None)
        return _mc_call(self._L, self.cache.handle, f, self.B, self.K, samples, rg, vh, mq, seed, sample_lo)

    def _record(self, q, r, qf):
        """the head of a record of a scvx_batch_ call of _calls.TABLE: the batch and the LQR weights (dynamics._track_weights)"""
        from .dynamics import _track_weights
        qv, rv, qfv = _track_weights(self.cache.nu, q, r, qf)
        return dict(handle=self.handle, q14=qv, rNU=rv, qf14=qfv)

    def _analysis(self, f, names):
        """the shared end of the first-order analyses and their back-offs: allocate the outputs `names`, choose the entry point, call"""
        f.update(_calls.analysis_outputs(self.B, self.K, self.cache.nu, names, f.get("m", 0)))
        _calls.call(self._L, self.cache.handle, _calls.analysis_entry(f), f)
        return f

    def _vehicle_sp(self, vehicle):
        """sp [6] of vehicle = (mu, sp) for the first-order analyses (dynamics._cov_vehicle's refusals; the tiles are the batch's own)"""
        from .dynamics import _cov_vehicle
        return _cov_vehicle(self.cache, vehicle, np.zeros((self.B, self.K, _lib.VTILE_N, 14)), (), self.B, self.K)[0]

    def covariance(self, S0, w=None, q=None, r=None, qf=None, dense=False, vehicle=None, clamp=False, band=None):
        """Closed-loop covariance analysis of the batch's current accepted iterate under its LQR gains (scvx_batch_cov; S0, w and
        dense as dynamics.cov_propagate_batch, weights as track_gains): a dynamics.CovReport.  The batch is left untouched.
        vehicle = (mu, sp) of montecarlo.vehicle_errors, mu = 0: the report and the dense outputs of Sigma_k + J_k diag(sp^2) J_k', the
        vehicle errors as consider parameters (scvx_batch_cov_veh: the vehicle tiles of the iterate, then the analysis).
        clamp=True: the clamp-aware analysis by statistical linearisation (scvx_batch_cov_clamp; band and dense as
        dynamics.cov_propagate_batch with clamp=True): a dynamics.SatCovReport.  Not together with vehicle."""
        from .dynamics import CovReport, SatCovReport, _cov_band, _cov_noise, _cov_s0
        if clamp and vehicle is not None:
            raise ValueError("clamp=True has no vehicle-error form: vehicle= must be None")
        if not clamp and band is not None:
            raise ValueError("band= needs clamp=True")
        f = self._record(q, r, qf)
        f.update(S0=_cov_s0(S0, self.B), w14=_cov_noise(w))
        if clamp:
            f["band2"] = _cov_band(band)
            self._analysis(f, _calls.dense_names(dense, _calls.CLAMP_DENSE) | {"report", "satrep"})
            return SatCovReport(f["report"], f["satrep"], f["mean"], f["sig"], f["covK"], f["cov"], f["satk"])
        want = _calls.dense_names(dense, _calls.COV_DENSE)
        if vehicle is not None:
            f["sp6"] = self._vehicle_sp(vehicle)
        self._analysis(f, want | {"report"})
        return CovReport(f["report"], f["sig"], f["covK"], f["cov"])

    def set_thrust_margins(self, lo=None, hi=None):
        """Per-node back-offs of the thrust band for every conic solve that follows: Tmin + lo[b, k] <= |u_k| <= Tmax - hi[b, k]
        (scvx_batch_set_thrust_margins; lo, hi [B][K+1], [K+1] for all or a scalar; both None clears).  init() clears them, reset()
        keeps them.  The flight check and the tracking calls keep auditing against the true Tmin / Tmax."""
        if (lo is None) != (hi is None):
            raise ValueError("set_thrust_margins: give lo and hi, or neither (clear)")
        if lo is None:
            self._chk(self._L.scvx_batch_set_thrust_margins(self.handle, None, None), "scvx_batch_set_thrust_margins")
            return self
        a = [np.ascontiguousarray(np.broadcast_to(np.asarray(v, np.float64), (self.B, self.K + 1))) for v in (lo, hi)]
        self._chk(self._L.scvx_batch_set_thrust_margins(self.handle, _p(a[0]), _p(a[1])), "scvx_batch_set_thrust_margins")
        return self

    def thrust_margins(self):
        """(lo, hi) [B][K+1] each: the back-offs the conic solve reads (zeros when none are set)."""
        lo, hi = np.empty((self.B, self.K + 1)), np.empty((self.B, self.K + 1))
        self._chk(self._L.scvx_batch_get_thrust_margins(self.handle, _p(lo), _p(hi)), "scvx_batch_get_thrust_margins")
        return lo, hi

    def set_path_margins(self, mass=None, glide=None, tilt=None, rate=None):
        """Per-node back-offs of four path constraints for every conic solve that follows (scvx_batch_set_path_margins):
        m_k >= mdry + mass[b, k], |r_k[2:3]| <= r_k[1] / tan(gammaGs) - glide[b, k], |q_k[2:3]| <= sqcm - tilt[b, k] and
        |w_k| <= omMax - rate[b, k].  Each is [B][K+1], [K+1] for all or a scalar, None for zeros; a [K+1] or scalar value is broadcast
        and the entries that must be 0 are zeroed (glide, tilt, rate at node K; mass, glide, rate at node 0), a [B][K+1] array is
        passed as it is.  All None clears.  init() clears them, reset() keeps them; the flight check, the tracking and the covariance
        calls keep auditing against the true constants."""
        vals = (mass, glide, tilt, rate)
        if all(v is None for v in vals):
            self._chk(self._L.scvx_batch_set_path_margins(self.handle, None), "scvx_batch_set_path_margins")
            return self
        pm = np.zeros((self.B, self.K + 1, _lib.PMARG_N))
        for c, v in enumerate(vals):
            if v is None:
                continue
            a = np.asarray(v, np.float64)
            pm[:, :, c] = np.broadcast_to(a, (self.B, self.K + 1))
            if a.ndim < 2:   # a broadcast value: the forced zeros are applied
                pm[:, 0 if c == _lib.PMARG_INDEX["MASS"] else self.K, c] = 0.0
                if c in (_lib.PMARG_INDEX["GLIDE"], _lib.PMARG_INDEX["RATE"]):
                    pm[:, 0, c] = 0.0
        self._chk(self._L.scvx_batch_set_path_margins(self.handle, _p(pm)), "scvx_batch_set_path_margins")
        return self

    def path_margins(self):
        """pm [B][K+1][4] = (mass, glide, tilt, rate): the path back-offs the conic solve reads (zeros when none are set)."""
        pm = np.empty((self.B, self.K + 1, _lib.PMARG_N))
        self._chk(self._L.scvx_batch_get_path_margins(self.handle, _p(pm)), "scvx_batch_get_path_margins")
        return pm

    @staticmethod
    def _margin_mask(constraints):
        names = tuple(_lib.MARGIN_BITS) if isinstance(constraints, str) and constraints == "all" else constraints
        if isinstance(names, str) or len(tuple(names)) == 0 or any(n not in _lib.MARGIN_BITS for n in names):
            raise ValueError('constraints: a non-empty subset of %s, or "all"' % (tuple(_lib.MARGIN_BITS),))
        mask = 0
        for n in names:
            mask |= _lib.MARGIN_BITS[n]
        return mask

    def _margins_from_cov(self, S0, w, q, r, qf, nsigma, cap, want_psig, mask=None, vehicle=None):
        from .dynamics import _cov_noise, _cov_s0
        f = self._record(q, r, qf)
        f.update(S0=_cov_s0(S0, self.B), w14=_cov_noise(w), nsigma=nsigma, cap=cap, which=mask)
        if vehicle is not None:   # the _veh form has no thrust-only twin: the thrust bit says the same
            f.update(sp6=self._vehicle_sp(vehicle), which=mask if mask is not None else _lib.MARGIN_BITS["thrust"])
        return self._analysis(f, {"psig"} if want_psig else ())["psig"]

    def margins_from_cov(self, S0, constraints="all", nsigma=3.0, cap=0.25, w=None, q=None, r=None, qf=None, vehicle=None):
        """The back-offs min(nsigma s(k), cap width_k) of `constraints` from the covariance analysis of the current accepted iterate
        (scvx_batch_margins_from_cov; the others stay as they are): returns psig [B][K+1][5].  vehicle = (mu, sp), mu = 0: the s(k) of
        Sigma_k + J_k diag(sp^2) J_k' (scvx_batch_margins_from_cov_veh)."""
        return self._margins_from_cov(S0, w, q, r, qf, nsigma, cap, True, self._margin_mask(constraints), vehicle)

    def _margins_from_nav(self, S0, nav, w, q, r, qf, nsigma, cap, want_psig, mask, vehicle=None):
        from .dynamics import _cov_noise, _cov_s0, _nav_arg
        n0, m, Hm, rmv = _nav_arg(nav, self.B)
        f = self._record(q, r, qf)
        f.update(S0=_cov_s0(S0, self.B), N0=n0, m=m, H=Hm, rm=rmv, w14=_cov_noise(w), nsigma=nsigma, cap=cap, which=mask)
        if vehicle is not None:
            f["sp6"] = self._vehicle_sp(vehicle)
        return self._analysis(f, {"psig"} if want_psig else ())["psig"]

    def margins_from_nav(self, S0, N0, H, rm, constraints="all", nsigma=3.0, cap=0.25, w=None, q=None, r=None, qf=None, vehicle=None):
        """margins_from_cov with the per-node s(k) of the NAVIGATION analysis of the current accepted iterate, the closed loop flown on
        an estimate (scvx_batch_margins_from_nav; N0, H, rm as navigation()): the same widths, caps and forced zeros, the constraints
        that are not selected stay as they are.  Returns psig [B][K+1][5], read off the truth block of the joint covariance.
        vehicle = (mu, sp), mu = 0: with J_k diag(sp^2) J_k' on the truth block (scvx_batch_margins_from_nav_veh)."""
        return self._margins_from_nav(S0, (N0, H, rm), w, q, r, qf, nsigma, cap, True, self._margin_mask(constraints), vehicle)

    def margins_from_mc(self, S0, p=0.99865, samples=1024, constraints="all", cap=0.25, seed=0, w=None, clamp=False, nav=None, q=None,
                        r=None, qf=None, nsub=None, tol=0.0, draws=None, rng="host", independent=False, sample_lo=0, plan_lo=0,
                        vehicle=None):
        """Back-offs from the SAMPLED closed loop of the current accepted iterate -- nonlinear and aware of the clamp, where
        margins_from_cov / margins_from_nav are first order: one track_mc call (truth-fed, or flown on an estimate with nav = (N0, H,
        rm)) with the ranks of 1 - p and p and the per-node order statistics, montecarlo.margins_from_quantiles on them (the formulas,
        caps and forced zeros are there; the thrust pair is asymmetric), and set_thrust_margins / set_path_margins for the kinds in
        `constraints` (the others stay as they are).  Returns (rep, lo, hi, pm): the report (rep.pathq [B][K+1][5][2]) and the back-offs
        as set.  Limits: the glide back-off buys tan(gammaGs) times what is written; a tail quantile from `samples` flights carries the
        standard error montecarlo.quantile_stderr(p, samples) (0.26 sigma at the defaults, and beyond samples (1 - p) < 1 the rank is the
        sample's extreme); the draws are shared across plans unless `independent=True` (with rng="device": the lanes make the draws,
        track_mc's keywords); with clamp=True the thrust function is still the unclamped command.  vehicle = (mu, sp): the flights
        carry per-flight vehicle errors (track_mc's keyword); the thrust pair still comes from the COMMAND, which only sees them through
        the feedback."""
        from .montecarlo import margins_from_quantiles
        mask = self._margin_mask(constraints)
        names = [n for n, bit in _lib.MARGIN_BITS.items() if mask & bit]
        rep = self.track_mc(S0, samples=samples, seed=seed, w=w, q=q, r=r, qf=qf, nsub=nsub, clamp=clamp, tol=tol, draws=draws, nav=nav,
                            quantiles=(1.0 - p, p), per_node=True, rng=rng, independent=independent, sample_lo=sample_lo,
                            plan_lo=plan_lo, vehicle=vehicle)
        x, u, _ = self.trajectory()
        cur = self.thrust_margins() + (self.path_margins(),)
        lo, hi, pm = margins_from_quantiles(self.cache.problem, x, u, rep.pathq[..., 0], rep.pathq[..., 1], names, cap, current=cur)
        if mask & _lib.MARGIN_BITS["thrust"]:
            self.set_thrust_margins(lo, hi)
        if mask & ~_lib.MARGIN_BITS["thrust"]:
            self._chk(self._L.scvx_batch_set_path_margins(self.handle, _p(np.ascontiguousarray(pm))), "scvx_batch_set_path_margins")
        return rep, lo, hi, pm

    def path_sigma(self, S0, w=None, q=None, r=None, qf=None, nav=None, vehicle=None):
        """psig [B][K+1][5]: per node, one standard deviation of the mass, glide-slope, tilt, rate and thrust-norm path functions
        of the batch's current accepted iterate under its LQR gains (dynamics.cov_path_sigma_batch on the batch's own tiles).  The
        batch's iterate, scalars and flags are left untouched and so are its thrust back-offs.  nav = (N0, H, rm): the same of the
        navigation analysis, the law fed an estimate (dynamics.nav_path_sigma_batch).  vehicle = (mu, sp), mu = 0: the s(k) with the
        vehicle errors as consider parameters, the vehicle tiles from dynamics.vehicle_tiles_batch on the iterate."""
        from .dynamics import _nav_arg, cov_path_sigma_batch, nav_path_sigma_batch, vehicle_tiles_batch
        if nav is not None:
            n0, _, Hm, rmv = _nav_arg(nav, self.B)   # a malformed model is refused before anything is read back
        x, u, sg = self.trajectory()
        kw = {} if vehicle is None else dict(vehicle=vehicle, vtile=vehicle_tiles_batch(self.cache, x, u, sg))
        if nav is not None:
            return nav_path_sigma_batch(self.cache, x, u, self.linearization()[1], self.track_gains(q, r, qf), S0, n0, Hm, rmv, w, **kw)[1]
        return cov_path_sigma_batch(self.cache, x, u, self.linearization()[1], self.track_gains(q, r, qf), S0, w, **kw)[1]

    def replan(self):
        """Start the SCvx loop again from the current iterate (scvx_batch_replan: rk = 100, cost = Inf, iter = 0, RUNNING, live for
        every active trajectory; failed ones stay frozen); on the device, asynchronous."""
        self._chk(self._L.scvx_batch_replan(self.handle), "scvx_batch_replan")
        return self

    def robustify(self, S0, nsigma=3.0, rounds=1, cap=0.25, w=None, q=None, r=None, qf=None, constraints=("thrust",), nav=None, mc=None,
                  vehicle=None):
        """Covariance-driven replanning.  Per round: the back-offs lo_k = hi_k = min(nsigma s_T(k), cap (Tmax - Tmin)) from the
        covariance analysis of the current iterate (scvx_batch_thrust_margins_from_cov, nothing returns to the host), replan(),
        solve().  Returns the last solve()'s (status, iters, nu_norm, dJ) plus (lo, hi).  First order, and only as good as Sigma_k;
        s_T depends on the plan, so one round reaches about 2.5 - 3 sigma of headroom for nsigma = 3, not exactly n; a replan may
        land in another local optimum than a solve from the straight-line guess.
        constraints: which rows are tightened, any subset of ("thrust", "mass", "glide", "tilt", "rate") or "all"; the path ones
        get min(nsigma s(k), cap width_k) with the widths of scvx_batch_margins_from_cov, and path_margins() reads them afterwards.
        The return value is the same six for every choice; the default is the call it always was.
        nav = (N0, H, rm): the s(k) come from the navigation analysis instead (scvx_batch_margins_from_nav per round), the closed loop
        flown on an estimate with the measurement H, rm at every node but the last; under navigation errors the covariance analysis'
        s(k) are too small, and a plan backed off by them keeps less than it shows.  Same limits, and the filter gain is the optimal
        one for the stated model.
        mc = dict(p=..., samples=..., seed=..., clamp=..., rng=..., independent=..., sample_lo=..., plan_lo=..., vehicle=...): the back-offs of each round come from the SAMPLED closed loop instead
        (margins_from_mc: per-node order statistics Q_{1-p}, Q_p of `samples` flights, nonlinear and clamp-aware; nsigma is then not
        used).  mc and nav combine: the flights are flown on the estimate.  Limits as margins_from_mc; mc=None is the call it was.
        vehicle = (mu, sp) of montecarlo.vehicle_errors, mu = 0: the s(k) of the covariance or (with nav) the navigation path carry the
        vehicle errors as consider parameters (scvx_batch_margins_from_cov_veh / _nav_veh per round; first order, the thrust row is the
        command's).  The sampled path has its own: mc=dict(vehicle=...); giving both is refused."""
        if int(rounds) < 1:
            raise ValueError("robustify: rounds >= 1")
        if vehicle is not None:
            if mc is not None:
                raise ValueError("robustify: vehicle= belongs to the covariance and navigation paths; the sampled path takes "
                                 "mc=dict(vehicle=...)")
            self._vehicle_sp(vehicle)   # refused before the first round
        mask = self._margin_mask(constraints)
        thrust_only = mask == _lib.MARGIN_BITS["thrust"]
        out = None
        if mc is not None:
            if not isinstance(mc, dict) or not set(mc) <= {"p", "samples", "seed", "clamp", "rng", "independent", "sample_lo", "plan_lo",
                                                           "vehicle"}:
                raise ValueError("robustify: mc = dict(p=, samples=, seed=, clamp=, rng=, independent=, sample_lo=, plan_lo=, vehicle=)")
            if nav is not None:
                from .dynamics import _nav_arg
                _nav_arg(nav, self.B)
            for _ in range(int(rounds)):
                self.margins_from_mc(S0, constraints=constraints, cap=cap, w=w, q=q, r=r, qf=qf, nav=nav, **mc)
                self.replan()
                out = self.solve()
            return out + self.thrust_margins()
        if nav is not None:
            from .dynamics import _nav_arg
            _nav_arg(nav, self.B)   # a malformed model is refused before the first round
            for _ in range(int(rounds)):
                self._margins_from_nav(S0, nav, w, q, r, qf, nsigma, cap, False, mask, vehicle)
                self.replan()
                out = self.solve()
            return out + self.thrust_margins()
        for _ in range(int(rounds)):
            self._margins_from_cov(S0, w, q, r, qf, nsigma, cap, False, None if thrust_only else mask, vehicle)
            self.replan()
            out = self.solve()
        return out + self.thrust_margins()

    AUDIT_COLUMN = {"thrust": "G_TMIN", "glide": "G_GLIDE", "tilt": "G_TILT", "rate": "G_RATE"}   # the seg column a back-off answers

    def audit(self, nsub=None):
        """The segment audit of the batch's current accepted iterate (scvx_batch_segment_audit): a dynamics.SegmentReport, the path
        functions of the PLAN-mode flight check per segment.  The batch is left untouched."""
        from .dynamics import SegmentReport
        f = dict(handle=self.handle, nsub=nsub or 0, seg=np.empty((self.B, self.K, _lib.SEG_N)), report=np.empty((self.B, _lib.FLIGHT_NREP)))
        _calls.call(self._L, self.cache.handle, "scvx_batch_segment_audit", f)
        return SegmentReport(f["seg"], f["report"])

    def _audit_mask(self, constraints):
        mask = self._margin_mask(constraints)
        if mask & _lib.MARGIN_BITS["mass"]:
            raise ValueError("the audit has no mass back-off: mass is monotone, a bound held at the nodes holds between them")
        return mask

    def margins_from_audit(self, constraints=("thrust", "tilt"), gain=1.5, tol=1e-7, cap=0.25, nsub=None, want_seg=True):
        """Back-offs from the segment audit of the current accepted iterate, on the device (scvx_batch_audit_margins): per node,
        new = min(old + gain e_k, cap width_k) with e_k the larger excess over tol of the two segments that meet at the node.  They
        ACCUMULATE on what the batch carries; "thrust" raises lo alone.  constraints: a subset of ("thrust", "glide", "tilt", "rate").
        Returns seg [B][K][11] of the audit the back-offs were taken from (None with want_seg=False: nothing returns to the host)."""
        f = dict(handle=self.handle, nsub=nsub or 0, which=self._audit_mask(constraints), gain=gain, tol=tol, cap=cap,
                 seg=np.empty((self.B, self.K, _lib.SEG_N)) if want_seg else None)
        _calls.call(self._L, self.cache.handle, "scvx_batch_audit_margins", f)
        return f["seg"]

    def harden(self, constraints=("thrust", "glide", "tilt", "rate"), rounds=3, gain=1.5, tol=1e-7, restart="replan", nsub=None, cap=0.25):
        """Make the converged plans hold their own constraints BETWEEN the nodes.  Per round: margins_from_audit, then replan() (or,
        with restart="guess", reset(): the straight-line guess again, the back-offs kept), then solve().  It stops as soon as no
        converged plan has a selected G > tol in its audit, and after `rounds` at the latest.  Returns (status, iters, nu_norm, dJ) of
        the last solve() (iters 0 and NaN norms when the first audit was already clean), the SegmentReport of the final plans and the
        rounds used.  Limits: the samples are the substep boundaries; gain is a starting point (a violation can move to a
        neighbouring segment); a replan may land in another local optimum than a solve from the guess."""
        if restart not in ("replan", "guess"):
            raise ValueError('harden: restart must be "replan" or "guess", not %r' % (restart,))
        if int(rounds) < 1:
            raise ValueError("harden: rounds >= 1")
        mask = self._audit_mask(constraints)
        cols = [c for n, c in self.AUDIT_COLUMN.items() if mask & _lib.MARGIN_BITS[n]]
        rep, st = self.audit(nsub), self.flags()[0]
        out, used = (st, np.zeros(self.B, np.int32), np.full(self.B, np.nan), np.full(self.B, np.nan)), 0
        for _ in range(int(rounds)):
            conv = st == 0
            if not any((getattr(rep, c)[conv] > tol).any() for c in cols):
                break
            self.margins_from_audit(constraints, gain, tol, cap, nsub, want_seg=False)
            self.replan() if restart == "replan" else self.reset()
            out = self.solve()
            st, rep, used = out[0], self.audit(nsub), used + 1
        return out + (rep, used)

    def navigation(self, S0, N0, H, rm, w=None, q=None, r=None, qf=None, dense=False, vehicle=None, clamp=False):
        """Navigation-error covariance analysis of the batch's current accepted iterate flown on an estimate under its LQR gains
        (scvx_batch_nav_cov; S0, N0, H, rm, w and dense as dynamics.nav_cov_batch, weights as track_gains): a dynamics.NavReport.
        The batch is left untouched.  vehicle = (mu, sp), mu = 0: J_k diag(sp^2) J_k' on the truth block (scvx_batch_nav_cov_veh); the
        filter does not know theta, so navsig, kf and NAV_* are those of the call without it."""
        from .dynamics import NavReport, _cov_noise, _cov_s0, _nav_model
        if clamp:
            raise ValueError("clamp=True: the clamp-aware analysis has no navigation form (covariance(clamp=True) feeds the law the truth)")
        f = self._record(q, r, qf)
        f.update(S0=_cov_s0(S0, self.B), N0=_cov_s0(N0, self.B))
        f["m"], f["H"], f["rm"] = _nav_model(H, rm)
        f["w14"] = _cov_noise(w)
        want = _calls.dense_names(dense, _calls.NAV_DENSE)
        if vehicle is not None:
            f["sp6"] = self._vehicle_sp(vehicle)
        self._analysis(f, want | {"report", "navrep"})
        return NavReport(f["report"], f["navrep"], f["sig"], f["navsig"], f["kf"], f["joint"])

    def set_profiling(self, on: bool):
        self._chk(self._L.scvx_batch_set_profiling(self.handle, 1 if on else 0), "scvx_batch_set_profiling")

    def profile(self):
        """(dict of summed ms per kernel, steps) since the last call; synchronises."""
        ms = np.zeros(5)
        n = C.c_int64()
        self._chk(self._L.scvx_batch_get_profile(self.handle, _p(ms), C.byref(n)), "scvx_batch_get_profile")
        return dict(zip(("socp", "propagate", "tr_update", "linearize", "glue"), ms.tolist())), n.value

    def close(self):
        if getattr(self, "handle", None):
            self._L.scvx_batch_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- multi-GPU: see montecarlo.py (kept importable from here) -------------------------------------------
from .montecarlo import gather_records, shard_range  # noqa: E402,F401


def gather_trajectories(rec, group=None):
    """All-gather of the per-rank trajectory records [B][n] over the (default) torch.distributed process group into
    [world][B][n]; without an initialised group: [1][B][n].  Thin wrapper over montecarlo.gather_records."""
    import torch.distributed as dist
    if not (dist.is_available() and dist.is_initialized()):
        return rec.unsqueeze(0).clone()
    if group is None:
        return gather_records(rec, dist=dist)

    class _G:  # the module's collectives bound to `group`
        is_initialized = staticmethod(dist.is_initialized)
        get_world_size = staticmethod(lambda: dist.get_world_size(group))
        all_gather_into_tensor = staticmethod(lambda o, i: dist.all_gather_into_tensor(o, i, group=group))
        all_gather = staticmethod(lambda o, i: dist.all_gather(o, i, group=group))
    return gather_records(rec, dist=_G)
