"""Dynamics — host-side mirror of the reference's discretisation interface over the HIP path.

Same names and argument meaning as dynamics.jl of BenChung/SuccessiveConvexification:
    make_dynamics_module(info)                 dynamics.jl:141   (code generation; a no-op here — the
                                                                 Jacobians are analytic in the kernel)
    IntegratorCache(prob, info, lin_mod)       dynamics.jl:258   (owns the device context)
    linearize_dynamics(states, tf, dt, cache)  dynamics.jl:321
    predict_state(x, uk, up, sigma, dt, pinfo, cache)   dynamics.jl:315
plus the batched forms the GPU path exists for.  Everything computes in libscvx_hip.so.
"""
import ctypes as C
import numpy as np

from . import _calls, _lib
from .defns import AtmosphericData, DescentProblem, LinPoint, LinRes, ProbInfo

_dp = C.POINTER(C.c_double)


def _p(a):
    return a.ctypes.data_as(_dp)


def make_dynamics_module(info: ProbInfo):
    """The reference generates and evals a `Linearizer` module here; nothing to generate on this path."""
    return None


class IntegratorCache:
    """Holds the scvx_ctx (device, stream, problem constants, aero tables) for one DescentProblem."""

    def __init__(self, prob: DescentProblem, info: ProbInfo = None, lin_mod=None, device: int = 0, npts: int = 10):
        self.problem = prob
        self.info = info if info is not None else ProbInfo.from_problem(prob)
        self._L = _lib.lib()
        self._c_prob = prob.to_c()
        h = C.c_void_p()
        rc = self._L.scvx_ctx_create(C.byref(self._c_prob), int(device), C.byref(h))
        if rc != 0:
            raise _lib.ScvxError(f"scvx_ctx_create failed ({rc}): is a HIP device visible? (rc -1: bad problem, e.g. fins without finmxf > 0, "
                                  "the aerodynamic torque (model_flags 4) without AtmosphericData, or an unknown model_flags bit)")
        self.handle = h
        self.device = device
        self.nu = int(self._L.scvx_control_dim(h))        # 3, or 5 with the fin extension (SCVX_MODEL_FINS)
        self.np = 14 + 2 * self.nu + 1
        self.set_npts(npts)
        if isinstance(prob.aero, AtmosphericData):
            a = prob.aero
            d = np.ascontiguousarray(a.drag_itrp, float)
            l = np.ascontiguousarray(a.lift_itrp, float)
            t = np.ascontiguousarray(a.trq_itrp, float)
            nm, na = d.shape
            _lib.check(h, self._L.scvx_set_aero_table(h, _p(d), _p(l), _p(t), na, nm, a.aoa0, a.daoa, a.mach0, a.dmach),
                       "scvx_set_aero_table")

    def cproblem(self):
        """The flat struct scvx_problem this context was created from (what a ccall caller passes by pointer)."""
        return self._c_prob

    def set_npts(self, npts: int):
        _lib.check(self.handle, self._L.scvx_set_nsub(self.handle, int(npts)), "scvx_set_nsub")

    @property
    def npts(self) -> int:
        return self._L.scvx_get_nsub(self.handle)

    def set_stream(self, stream_handle):
        _lib.check(self.handle, self._L.scvx_set_stream(self.handle, C.c_void_p(stream_handle or 0)), "scvx_set_stream")

    def synchronize(self):
        _lib.check(self.handle, self._L.scvx_synchronize(self.handle), "scvx_synchronize")

    def close(self):
        if getattr(self, "handle", None):
            self._L.scvx_ctx_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def linearize_batch(cache: IntegratorCache, x, u, sigma, dt):
    """x [B][K+1][14], u [B][K+1][nu], sigma [B] (host) -> endpoint [B][K][14], deriv [B][K][14+2nu+1][14]  (nu = cache.nu)."""
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    B, K1, nx = x.shape
    K = K1 - 1
    if nx != 14 or u.shape != (B, K1, cache.nu) or sigma.shape != (B,):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    e = np.empty((B, K, 14))
    d = np.empty((B, K, cache.np, 14))
    _lib.check(cache.handle, cache._L.scvx_linearize_f64_host(cache.handle, B, K, _p(x), _p(u), _p(sigma), float(dt),
                                                              _p(e), _p(d)), "scvx_linearize_f64_host")
    return e, d


def propagate_batch(cache: IntegratorCache, x, u, sigma, dt):
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    B, K1, nx = x.shape
    K = K1 - 1
    if nx != 14 or u.shape != (B, K1, cache.nu) or sigma.shape != (B,):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    e = np.empty((B, K, 14))
    _lib.check(cache.handle, cache._L.scvx_propagate_f64_host(cache.handle, B, K, _p(x), _p(u), _p(sigma), float(dt),
                                                              _p(e)), "scvx_propagate_f64_host")
    return e


class FlightReport:
    """The report of a flight check (scvx_flight_check_f64, include/scvx.h): `raw` [B][16], one named numpy view per column
    (report.GAP, report.G_TMIN, ... -- _lib.FLIGHT_COLUMNS), `xfly` [B][K+1][14] (the flown node states) or None, and `mode`.
    g <= 0 means satisfied, in the problem's own units.  G_TMIN > 0 between nodes that sit on the bound belongs to the reference's
    formulation (lower bound linearised at the nodes, first-order-hold control), not to the solver."""

    G_COLUMNS = tuple(n for n in _lib.FLIGHT_COLUMNS if n.startswith("G_"))

    def __init__(self, raw, xfly=None, mode="shoot", ufly=None):
        self.raw = np.asarray(raw, np.float64).reshape(-1, _lib.FLIGHT_NREP)
        self.xfly = xfly
        self.mode = mode
        self.ufly = ufly   # mode "track" with dense=True: the applied node controls [B][K+1][nu]
        for name, i in _lib.FLIGHT_INDEX.items():
            setattr(self, name, self.raw[:, i])

    def __len__(self):
        return self.raw.shape[0]

    def active(self):
        """Names of the G_* columns the model enforces (G_DP / G_FIN are -inf in every row when their flag is clear)."""
        return tuple(n for n in self.G_COLUMNS if not np.all(np.isneginf(getattr(self, n))))

    def worst(self):
        """[B]: the largest G_* of each trajectory (NaN if any is NaN)."""
        g = self.raw[:, [_lib.FLIGHT_INDEX[n] for n in self.G_COLUMNS]]
        return np.where(np.isnan(g).any(axis=1), np.nan, np.max(np.nan_to_num(g, nan=-np.inf), axis=1))

    def ok(self, tol=0.0):
        """[B] bool: every active G_* <= tol (a NaN row is not ok)."""
        return self.worst() <= tol


def _flight_mode(mode):
    if isinstance(mode, str):
        if mode not in ("shoot", "plan"):
            raise ValueError("mode must be 'shoot' or 'plan' (or SCVX_FLIGHT_SHOOT / SCVX_FLIGHT_PLAN), not %r" % (mode,))
        return _lib.FLIGHT_SHOOT if mode == "shoot" else _lib.FLIGHT_PLAN
    return int(mode)   # an unknown number goes to the library, which refuses it with its own message


def flight_check_batch(cache: IntegratorCache, x, u, sigma, nsub=None, mode="shoot", dense=False) -> FlightReport:
    """Fly the plans x [B][K+1][14], u [B][K+1][nu], sigma [B] open loop on the device and audit the path constraints between the
    nodes (scvx_flight_check_f64_host).  mode "shoot": single shooting from x[:, 0]; "plan": restart at every planned node.
    nsub: RK4 substeps per segment (None = the cache's); dense: also return the flown node states."""
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    if x.ndim != 3 or x.shape[2] != 14 or u.shape != (x.shape[0], x.shape[1], cache.nu) or sigma.shape != (x.shape[0],):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    B, K1, _ = x.shape
    rep = np.empty((B, _lib.FLIGHT_NREP))
    xfly = np.empty((B, K1, 14)) if dense else None
    _lib.check(cache.handle, cache._L.scvx_flight_check_f64_host(
        cache.handle, B, K1 - 1, _p(x), _p(u), _p(sigma), int(cache.npts if nsub is None else nsub), int(_flight_mode(mode)),
        _p(rep), _p(xfly) if dense else None), "scvx_flight_check_f64_host")
    return FlightReport(rep, xfly, mode)


class SegmentReport:
    """The segment audit of a batch of plans (scvx_segment_audit_f64, include/scvx.h): `seg` [B][K][11], one named [B][K] numpy view per
    column (rep.DEFECT, rep.G_TMIN, ... -- _lib.SEG_COLUMNS), and `flight`, the PLAN-mode FlightReport reduced from seg on the device.
    g <= 0 means satisfied, in the problem's own units; segment k runs from node k to node k + 1."""

    def __init__(self, seg, flight_raw):
        self.seg = np.asarray(seg, np.float64)
        self.flight = FlightReport(flight_raw, None, "plan")
        for name, i in _lib.SEG_INDEX.items():
            setattr(self, name, self.seg[:, :, i])

    def __len__(self):
        return self.seg.shape[0]

    def worst(self, name):
        """(value [B], segment [B]) of the largest entry of column `name` in every plan; a NaN entry wins."""
        g = getattr(self, name)
        k = np.where(np.isnan(g).any(axis=1), np.isnan(g).argmax(axis=1), np.nan_to_num(g, nan=-np.inf).argmax(axis=1))
        return g[np.arange(g.shape[0]), k], k


def segment_audit_batch(cache: IntegratorCache, x, u, sigma, nsub=None) -> SegmentReport:
    """Audit the plans x [B][K+1][14], u [B][K+1][nu], sigma [B] segment by segment on the device (scvx_segment_audit_f64_host): the
    path functions of the PLAN-mode flight check, one row per segment.  nsub: RK4 substeps per segment (None = the cache's)."""
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    if x.ndim != 3 or x.shape[2] != 14 or u.shape != (x.shape[0], x.shape[1], cache.nu) or sigma.shape != (x.shape[0],):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    B, K = x.shape[0], x.shape[1] - 1
    f = dict(handle=cache.handle, B=B, K=K, x=x, u=u, sigma=sigma, nsub=cache.npts if nsub is None else nsub,
             seg=np.empty((B, K, _lib.SEG_N)), report=np.empty((B, _lib.FLIGHT_NREP)))
    _calls.call(cache._L, cache.handle, "scvx_segment_audit_f64_host", f)
    return SegmentReport(f["seg"], f["report"])


TRACK_DEFAULT_WEIGHTS = (1.0, 1.0, 100.0)   # q, r, qf on every component: a starting point, not tuning advice


def _track_weights(nu, q, r, qf):
    """scalars broadcast to the weight vectors q[14], r[nu], qf[14]; None = TRACK_DEFAULT_WEIGHTS"""
    out = []
    for v, d, m, name in ((q, TRACK_DEFAULT_WEIGHTS[0], 14, "q"), (r, TRACK_DEFAULT_WEIGHTS[1], nu, "r"),
                          (qf, TRACK_DEFAULT_WEIGHTS[2], 14, "qf")):
        a = np.asarray(d if v is None else v, np.float64)
        if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != m):
            raise ValueError("%s must be a scalar or have %d components" % (name, m))
        out.append(np.ascontiguousarray(np.broadcast_to(a, (m,)), np.float64))
    return out


def track_gains_batch(cache: IntegratorCache, deriv, q=None, r=None, qf=None, cost=False):
    """Time-varying LQR gains about plans from their derivative tiles deriv [B*K][14+2nu+1][14] (or [B][K][...]; what
    linearize_batch returns), on the device (scvx_track_gains_f64_host; the recursion is in include/scvx.h).  q, r, qf: diagonal
    weights in the problem's normalised units, scalars broadcast; defaults 1, 1, 100 -- a starting point, not tuning advice (the
    quaternion and mass directions are nearly uncontrollable).  Returns gain [B][K][nu][14+nu]: du_{k+1} = gain[b, k] @ [dx_k; du_k];
    with cost=True also p0 [B][14+nu][14+nu]: z0' p0 z0 is the predicted cost of an initial deviation z0."""
    nu, K = cache.nu, cache.problem.K
    deriv = np.ascontiguousarray(deriv, np.float64)
    if deriv.size == 0 or deriv.size % (K * 14 * (15 + 2 * nu)) or deriv.shape[-2:] != (15 + 2 * nu, 14):
        raise ValueError("shape mismatch: deriv [B*K][%d][14] with K = %d" % (15 + 2 * nu, K))
    B = deriv.size // (K * 14 * (15 + 2 * nu))
    qv, rv, qfv = _track_weights(nu, q, r, qf)
    gain = np.empty((B, K, nu, 14 + nu))
    p0 = np.empty((B, 14 + nu, 14 + nu)) if cost else None
    _lib.check(cache.handle, cache._L.scvx_track_gains_f64_host(cache.handle, B, K, _p(deriv), _p(qv), _p(rv), _p(qfv), _p(gain),
                                                                _p(p0) if cost else None), "scvx_track_gains_f64_host")
    return (gain, p0) if cost else gain


def track_fly_batch(cache: IntegratorCache, x, u, sigma, gain, dx0=None, nsub=None, clamp=False, dense=False, nav=None) -> FlightReport:
    """Fly the plans x [B][K+1][14], u [B][K+1][nu], sigma [B] closed loop under the gains gain [B][K][nu][14+nu] from
    x[:, 0] + dx0 (dx0 [B][14] or None = 0) on the device (scvx_track_fly_f64_host).  The report has the flight check's 16 columns
    (G_* on the flown state and the applied control; GAP against the planned nodes); mode "track".  clamp: rescale the commanded
    thrust norm into [Tmin, Tmax] (and the fin norm below finmxf); off by default: a plan that rides Tmin saturates on one side at
    most nodes and the law loses most of its authority, and without it G_TMIN / G_TMAX show what the law asked for.
    dense: also xfly [B][K+1][14] and ufly [B][K+1][nu].  nav [B][K][14]: the law is fed an estimate whose error at node k is
    nav[:, k] (scvx_track_fly_nav_f64_host; zeros reproduce the flight without it bit for bit); None: the true state."""
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    gain = np.ascontiguousarray(gain, np.float64)
    if x.ndim != 3 or x.shape[2] != 14 or u.shape != (x.shape[0], x.shape[1], cache.nu) or sigma.shape != (x.shape[0],):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    B, K1, _ = x.shape
    if gain.shape != (B, K1 - 1, cache.nu, 14 + cache.nu):
        raise ValueError("shape mismatch: gain [B][K][%d][%d]" % (cache.nu, 14 + cache.nu))
    if dx0 is not None:
        dx0 = np.ascontiguousarray(dx0, np.float64)
        if dx0.shape != (B, 14):
            raise ValueError("shape mismatch: dx0 [B][14]")
    rep = np.empty((B, _lib.FLIGHT_NREP))
    xfly = np.empty((B, K1, 14)) if dense else None
    ufly = np.empty((B, K1, cache.nu)) if dense else None
    if nav is not None:
        nav = np.ascontiguousarray(nav, np.float64)
        if nav.shape != (B, K1 - 1, 14):
            raise ValueError("shape mismatch: nav [B][K][14]")
        _lib.check(cache.handle, cache._L.scvx_track_fly_nav_f64_host(
            cache.handle, B, K1 - 1, _p(x), _p(u), _p(sigma), _p(gain), _p(dx0) if dx0 is not None else None, _p(nav),
            int(cache.npts if nsub is None else nsub), _lib.TRACK_CLAMP if clamp else 0, _p(rep), _p(xfly) if dense else None,
            _p(ufly) if dense else None), "scvx_track_fly_nav_f64_host")
        return FlightReport(rep, xfly, "track", ufly)
    _lib.check(cache.handle, cache._L.scvx_track_fly_f64_host(
        cache.handle, B, K1 - 1, _p(x), _p(u), _p(sigma), _p(gain), _p(dx0) if dx0 is not None else None,
        int(cache.npts if nsub is None else nsub), _lib.TRACK_CLAMP if clamp else 0, _p(rep), _p(xfly) if dense else None,
        _p(ufly) if dense else None), "scvx_track_fly_f64_host")
    return FlightReport(rep, xfly, "track", ufly)


def vehicle_tiles_batch(cache: IntegratorCache, x, u, sigma):
    """The two per-segment sensitivities to the vehicle errors that the derivative tiles do not hold (scvx_vehicle_tiles_f64_host,
    include/scvx.h): vtile [B][K][2][14], row 0 = d x_{k+1} / d theta_ISP, row 1 = d x_{k+1} / d theta_AERO (zeros without
    aerodynamics), about the plan x [B][K+1][14], u [B][K+1][nu], sigma [B] at theta = 0, with the context's npts and dt = 1 / (K + 1).
    What vtile= of the first-order analyses takes when ISP or AERO is dispersed."""
    x = np.ascontiguousarray(x, np.float64)
    u = np.ascontiguousarray(u, np.float64)
    sigma = np.ascontiguousarray(sigma, np.float64)
    if x.ndim != 3 or x.shape[2] != 14 or u.shape != (x.shape[0], x.shape[1], cache.nu) or sigma.shape != (x.shape[0],):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    B, K = x.shape[0], x.shape[1] - 1
    vt = np.empty((B, K, _lib.VTILE_N, 14))
    _lib.check(cache.handle, cache._L.scvx_vehicle_tiles_f64_host(cache.handle, B, K, _p(x), _p(u), _p(sigma), _p(vt)),
               "scvx_vehicle_tiles_f64_host")
    return vt


def _cov_vehicle(cache, vehicle, vtile, dense, B, K):
    """vehicle= of the first-order analyses: None, or (mu [6], sp [6]) as montecarlo.vehicle_errors returns them; vtile: what
    vehicle_tiles_batch returns, needed when sp[ISP] or sp[AERO] is not 0; dense: the call's, "sens" among its names asks for J_k
    -> (sp or None, vtile or None, sens [B][K+1][n][6] or None, dense without "sens").  Every refusal of the library is a ValueError here."""
    want, rest = _calls.split_dense(dense, ("sens",))
    if vehicle is None:
        if want or vtile is not None:
            raise ValueError('dense "sens" and vtile= need vehicle=')
        return None, None, None, rest
    if not isinstance(vehicle, (tuple, list)) or len(vehicle) != 2:
        raise ValueError("vehicle = (mu [6], sp [6]): montecarlo.vehicle_errors")
    mu, sp = (np.ascontiguousarray(v, np.float64) for v in vehicle)
    if mu.shape != (6,) or sp.shape != (6,):
        raise ValueError("vehicle = (mu [6], sp [6]): montecarlo.vehicle_errors")
    if np.any(mu != 0.0):
        raise ValueError("vehicle: the first-order analyses are about the nominal vehicle, mu must be 0 (a mean shift is out of scope; "
                         "the sampled calls fly one)")
    if not (np.all(np.isfinite(sp)) and np.all(sp >= 0.0)):
        raise ValueError("vehicle: sp must be finite and >= 0")
    if sp[_lib.VEH_INDEX["FIN"]] != 0.0 and cache.nu != 5:
        raise ValueError("vehicle: sp[FIN] != 0 on a model without fins")
    if sp[_lib.VEH_INDEX["AERO"]] != 0.0 and not isinstance(cache.problem.aero, AtmosphericData):
        raise ValueError("vehicle: sp[AERO] != 0 on a model without aerodynamics")
    vt = None
    if vtile is not None:
        vt = np.ascontiguousarray(vtile, np.float64)
        if vt.shape != (B, K, _lib.VTILE_N, 14):
            raise ValueError("shape mismatch: vtile [B][K][%d][14] (vehicle_tiles_batch)" % _lib.VTILE_N)
    elif sp[_lib.VEH_INDEX["ISP"]] != 0.0 or sp[_lib.VEH_INDEX["AERO"]] != 0.0:
        raise ValueError("vehicle: sp[ISP] or sp[AERO] != 0 needs vtile= (vehicle_tiles_batch)")
    sens = np.empty((B, K + 1, 14 + cache.nu, _lib.VEH_N)) if want else None
    return sp, vt, sens, rest


class CovReport:
    """The dispersion report of a covariance analysis (scvx_cov_propagate_f64, include/scvx.h): `raw` [B][16], one named numpy view
    per column (report.SIG_R, report.N_TMIN, ... -- _lib.COV_COLUMNS), and the optional dense outputs `sig` [B][K+1][14+nu] (the
    1 sigma corridor about the plan), `covK` [B][n][n] (the final covariance) and `cov` [B][K+1][n][n], or None.  SIG_* / ELL_* /
    S_THRUST are standard deviations in the problem's own units; N_* are margins to the path constraints in standard deviations
    (+inf: no node had one; negative: the plan itself violates).  First order about the plan; the clamp is not modelled."""

    N_COLUMNS = tuple(n for n in _lib.COV_COLUMNS if n.startswith("N_"))

    def __init__(self, raw, sig=None, covK=None, cov=None, sens=None):
        self.raw = np.asarray(raw, np.float64).reshape(-1, _lib.COV_NREP)
        self.sig = sig
        self.covK = covK
        self.cov = cov
        self.sens = sens   # vehicle= with dense "sens": J_k = d z_k / d theta [B][K+1][n][6], else None
        for name, i in _lib.COV_INDEX.items():
            setattr(self, name, self.raw[:, i])

    def __len__(self):
        return self.raw.shape[0]

    def tightest(self):
        """[B]: the smallest N_* margin of each trajectory (NaN if any is NaN)."""
        g = self.raw[:, [_lib.COV_INDEX[n] for n in self.N_COLUMNS]]
        return np.where(np.isnan(g).any(axis=1), np.nan, np.min(np.nan_to_num(g, nan=np.inf), axis=1))


class SatCovReport(CovReport):
    """The two reports of a clamp-aware covariance analysis (scvx_cov_clamp_f64, include/scvx.h): everything a CovReport has, read off
    the statistically linearised Sigma_k (N_TMAX / N_TMIN / S_THRUST then describe the applied control and are no headroom figures),
    plus `satraw` [B][16] with one named view per column (report.BIAS_R, report.P_LO, report.GAIN_MIN, ... -- _lib.SAT_COLUMNS; the SIG_*
    views are the CovReport's, which hold the same values) and the optional dense outputs `mean` [B][K+1][14+nu] = mu_k and `satk`
    [B][K][4] = (That, s, P_lo, P_hi) of node k + 1, or None.  An approximation: expect a factor of about 2 in standard deviation."""

    def __init__(self, raw, satraw, mean=None, sig=None, covK=None, cov=None, satk=None):
        super().__init__(raw, sig, covK, cov)
        self.satraw = np.asarray(satraw, np.float64).reshape(-1, _lib.SAT_NREP)
        self.mean = mean
        self.satk = satk
        for name, i in _lib.SAT_INDEX.items():
            if not name.startswith("SIG_"):
                setattr(self, name, self.satraw[:, i])


def _cov_band(band):
    """band of the clamp-aware analysis: None (the problem's Tmin, Tmax) or (Tlo, Thi) -> None or a contiguous [2]; what the library
    refuses is a ValueError here"""
    if band is None:
        return None
    a = np.ascontiguousarray(band, np.float64)
    if a.shape != (2,) or not np.isfinite(a[0]) or np.isnan(a[1]) or a[0] < 0.0 or a[0] > a[1]:
        raise ValueError("band = (Tlo, Thi) with a finite Tlo >= 0 and Tlo <= Thi (Thi may be inf), not %r" % (band,))
    return a


def _cov_s0(S0, B):
    """S0 as [B][14][14], one [14][14] for all, or a [14] vector of standard deviations (S0 = diag(sd^2)) -> contiguous [B][14][14]"""
    a = np.asarray(S0, np.float64)
    if a.shape == (14,):
        a = np.diag(a * a)
    if a.shape == (14, 14):
        a = np.broadcast_to(a, (B, 14, 14))
    if a.shape != (B, 14, 14):
        raise ValueError("S0 must be [B][14][14], [14][14] or a [14] vector of standard deviations (B = %d)" % B)
    return np.ascontiguousarray(a, np.float64)


def _cov_noise(w):
    """process-noise variances: None, a scalar or [14] -> None or a contiguous [14]"""
    if w is None:
        return None
    a = np.asarray(w, np.float64)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != 14):
        raise ValueError("w must be a scalar or have 14 components")
    return np.ascontiguousarray(np.broadcast_to(a, (14,)), np.float64)


def _analysis(cache, f, names):
    """the shared end of the four first-order analyses: allocate the outputs `names`, choose the entry point from the record f, call"""
    f.update(_calls.analysis_outputs(f["B"], f["K"], cache.nu, names, f.get("m", 0)), handle=cache.handle)
    _calls.call(cache._L, cache.handle, _calls.analysis_entry(f), f)


def cov_propagate_batch(cache: IntegratorCache, x, u, deriv, gain, S0, w=None, dense=False, vehicle=None, vtile=None, clamp=False,
                        band=None) -> CovReport:
    """Closed-loop covariance of the plans x [B][K+1][14], u [B][K+1][nu] tracked under the gains gain [B][K][nu][14+nu] (what
    track_gains_batch returns) from the derivative tiles deriv [B][K][14+2nu+1][14] (what linearize_batch returns), on the device
    (scvx_cov_propagate_f64_host; the recursion and its limits are in include/scvx.h).  S0: the handover covariance, [B][14][14], one
    [14][14] for all, or a [14] vector of standard deviations; only its symmetric part is used.  w: process-noise variance added per
    segment, a scalar or [14] (None = 0).  dense: True for sig, covK and cov, or a subset of those names.
    vehicle: (mu, sp) of montecarlo.vehicle_errors with mu = 0 -- every output is then read off Sigma_k + J_k diag(sp^2) J_k'
    (scvx_cov_vehicle_f64_host; first order, the thrust columns are the command's), vtile: vehicle_tiles_batch's, needed when ISP or
    AERO is dispersed; dense may then name "sens" (report.sens = J_k).  Without vehicle the call is the one it was.
    clamp: True for the clamp-aware analysis by statistical linearisation (scvx_cov_clamp_f64_host: the thrust clamp of
    track_fly_batch(clamp=True) as a random-input describing function, a mean beside the covariance; an approximation, see
    include/scvx.h) -- a SatCovReport; band: (Tlo, Thi) in place of the problem's (Tmin, Tmax); dense then: True or names out of
    "mean", "sig", "covK", "cov", "satk".  Not together with vehicle.  With clamp=False the call is the one it was."""
    if clamp and (vehicle is not None or vtile is not None):
        raise ValueError("clamp=True has no vehicle-error form: vehicle= and vtile= must be None")
    if not clamp and band is not None:
        raise ValueError("band= needs clamp=True")
    f = _calls.plan_shapes(cache.nu, x, u, gain, deriv)
    f.update(S0=_cov_s0(S0, f["B"]), w14=_cov_noise(w))
    if clamp:
        f["band2"] = _cov_band(band)
        _analysis(cache, f, _calls.dense_names(dense, _calls.CLAMP_DENSE) | {"report", "satrep"})
        return SatCovReport(f["report"], f["satrep"], f["mean"], f["sig"], f["covK"], f["cov"], f["satk"])
    f["sp6"], f["vtile"], f["sens"], dense = _cov_vehicle(cache, vehicle, vtile, dense, f["B"], f["K"])
    _analysis(cache, f, _calls.dense_names(dense, _calls.COV_DENSE) | {"report"})
    return CovReport(f["report"], f["sig"], f["covK"], f["cov"], f["sens"])


def cov_path_sigma_batch(cache: IntegratorCache, x, u, deriv, gain, S0, w=None, vehicle=None, vtile=None, dense=()):
    """What the margins of cov_propagate_batch are made of (scvx_cov_path_sigma_f64_host; same arguments): (CovReport, psig) with psig
    [B][K+1][5] = s = sqrt(c' Sigma_k c) at every node for the path functions of the mass, glide-slope, tilt and rate margins and of the
    thrust norm (_lib.PSIG_COLUMNS).  Node 0 and a node its margin skips are 0; a non-finite tile, gain or S0 entry makes the rows of
    its own trajectory NaN.  psig[:, :, 4] is the s_T(k) that ScvxBatch.robustify turns into back-offs of the thrust band.
    vehicle, vtile: as cov_propagate_batch (psig and the report are then read off Sigma_k^tot); dense: () or ("sens",)."""
    f = _calls.plan_shapes(cache.nu, x, u, gain, deriv)
    f.update(S0=_cov_s0(S0, f["B"]), w14=_cov_noise(w))
    f["sp6"], f["vtile"], f["sens"], dense = _cov_vehicle(cache, vehicle, vtile, dense, f["B"], f["K"])
    if dense:
        raise ValueError('dense: () or ("sens",), not %r' % (dense,))
    _analysis(cache, f, {"report", "psig"})
    return CovReport(f["report"], sens=f["sens"]), f["psig"]


class McReport:
    """The report of a sampled dispersion (scvx_track_mc_f64, include/scvx.h): `raw` [B][48], one named numpy view per column
    (report.MAX_GAP, report.MEAN_MISS_R, report.P_TMIN, report.P_ANY, report.OUT_LO, report.N_BAD, ... -- _lib.MC_COLUMNS), the landing
    statistics `xmean` [B][14] and `xcov` [B][14][14] of x_fly[K] - xbar_K over the samples, and the optional dense outputs `flights`
    [B][S][16], `xland` [B][S][14] and `dx0` [B][S][14], or None.  The draws are shared by all plans unless the call was made with independent=True.  With `quantiles=` / `per_node=`
    (the _q forms of the call): `probs` and `ranks` (montecarlo.quantile_ranks), `q` [B][16][nq] the order statistics of the sixteen
    flight columns over the samples -- rep.quantile("MISS_R", 0.99) --, `pathq` [B][K+1][5][nq] those of the five path functions
    (_lib.PSIG_COLUMNS) at every node, and the dense `pathv` [B][K+1][5][S]; each None when not asked for.  A quantile is a selection
    of one flight's value, with the sampling error of montecarlo.quantile_stderr."""

    probs = ranks = q = pathq = pathv = theta = None

    def __init__(self, raw, xmean, xcov, flights=None, xland=None, dx0=None):
        self.raw = np.asarray(raw, np.float64).reshape(-1, _lib.MC_NREP)
        self.xmean, self.xcov = xmean, xcov
        self.flights, self.xland, self.dx0 = flights, xland, dx0
        for name, i in _lib.MC_INDEX.items():
            setattr(self, name, self.raw[:, i])

    def _with_q(self, mq):
        self.probs, self.ranks, self.q, self.pathq, self.pathv = mq.probs, mq.ranks, mq.flightq, mq.pathq, mq.pathv
        return self

    def _with_veh(self, vh):
        """`theta` [B][S][6]: the vehicle errors every flight flew (a call with vehicle= and the dense name "theta"), else None"""
        self.theta = vh.theta
        return self

    def _qi(self, p):
        if self.probs is None:
            raise ValueError("the call was made without quantiles=")
        hit = np.flatnonzero(self.probs == float(p))
        if hit.size == 0:
            raise ValueError("quantile %r was not asked for (probs = %s)" % (p, self.probs.tolist()))
        return int(hit[0])

    def quantile(self, column, p):
        """[B]: the order statistic of probability p (one of `probs`) of flight column `column` (_lib.FLIGHT_COLUMNS) over the samples."""
        return self.q[:, _lib.FLIGHT_INDEX[column], self._qi(p)]

    def path_quantile(self, column, p):
        """[B][K+1]: the order statistic of probability p of path function `column` (_lib.PSIG_COLUMNS) at every node (per_node=True)."""
        if self.pathq is None:
            raise ValueError("the call was made without per_node=True")
        return self.pathq[:, :, _lib.PSIG_INDEX[column], self._qi(p)]

    def __len__(self):
        return self.raw.shape[0]

    def flight(self, b):
        """The S flights of plan b as a FlightReport of S rows (needs dense "flights")."""
        if self.flights is None:
            raise ValueError("McReport.flight: the call was made without dense 'flights'")
        return FlightReport(self.flights[b], None, "track")


class _McQ:
    """What the _q forms of the sampled calls add: quantiles (an iterable of probabilities, or None), per_node, and "pathv" among the
    dense names -> the five trailing C arguments (nq, ranks, flightq, pathq, pathv) and their host arrays.  `on` False: the call is
    the old entry point, with exactly its arguments.  dense=True stays "all the dense outputs the call had": pathv is by name only."""

    def __init__(self, quantiles, per_node, dense):
        want_pv, self.rest = _calls.split_dense(dense, ("pathv",))
        self.pq = None if quantiles is None else np.atleast_1d(np.asarray(list(np.atleast_1d(quantiles)), np.float64))
        if self.pq is not None and not 1 <= self.pq.size <= 16:
            raise ValueError("quantiles: between 1 and 16 probabilities")
        if per_node and self.pq is None:
            raise ValueError("per_node=True needs quantiles=")
        self.per_node, self.want_pv = bool(per_node), bool(want_pv)
        self.on = self.pq is not None or self.want_pv
        self.probs = self.ranks = self.flightq = self.pathq = self.pathv = None

    def fields(self, B, K, S):
        """the five trailing fields of a call with `S` samples, allocated here"""
        from .montecarlo import quantile_ranks
        names = set()
        if self.pq is not None:
            self.probs, self.ranks = self.pq, np.ascontiguousarray(quantile_ranks(self.pq, S), np.int32)
            names = {"flightq", "pathq"} if self.per_node else {"flightq"}
        if self.want_pv:
            names.add("pathv")
        nq = 0 if self.ranks is None else int(self.ranks.size)
        out = _calls.mc_outputs(B, K, S, names, nq)
        self.flightq, self.pathq, self.pathv = out["flightq"], out["pathq"], out["pathv"]
        return dict(nq=nq, ranks=self.ranks, flightq=self.flightq, pathq=self.pathq, pathv=self.pathv)


class _McVeh:
    """What the _veh forms of the sampled calls add: vehicle = None, (mu, sp) as montecarlo.vehicle_errors returns them, or (mu, sp,
    zeta [S][6]) with draws of the caller's own, and "theta" among the dense names -> the five trailing C arguments (rng, noise, veh,
    zeta, theta).  `on` False: the call is the one it was, with exactly its arguments."""

    def __init__(self, vehicle, dense):
        want, self.rest = _calls.split_dense(dense, ("theta",))
        self.on = vehicle is not None
        if want and not self.on:
            raise ValueError('dense "theta" needs vehicle=')
        self.want, self.theta, self.zeta, self.veh = bool(want), None, None, None
        if self.on:
            if len(vehicle) not in (2, 3):
                raise ValueError("vehicle = (mu [6], sp [6]) or (mu, sp, zeta [S][6]): montecarlo.vehicle_errors")
            mu, sp = (np.ascontiguousarray(v, np.float64) for v in vehicle[:2])
            if mu.shape != (6,) or sp.shape != (6,):
                raise ValueError("vehicle = (mu [6], sp [6]) or (mu, sp, zeta [S][6]): montecarlo.vehicle_errors")
            self.veh = _lib.ScvxMcVehicle((C.c_double * 6)(*mu), (C.c_double * 6)(*sp), (C.c_int32 * 2)(0, 0))
            self.sp = sp
            self.zeta = None if len(vehicle) == 2 or vehicle[2] is None else np.ascontiguousarray(vehicle[2], np.float64)

    def fields(self, B, S, rg, seed, lo):
        """the fields veh, zeta and theta of a call with `S` samples; rg: the scvx_mc_rng of rng="device" or None"""
        from .montecarlo import mc_vehicle_draws
        if not self.on:
            return dict(veh=None, zeta=None, theta=None)
        if rg is not None:
            if self.zeta is not None:
                raise ValueError('vehicle: zeta cannot be combined with rng="device": the device makes its own '
                                 "(montecarlo.mc_vehicle_draws_device is its twin)")
        elif self.zeta is None:
            self.zeta = mc_vehicle_draws(S, seed, lo)
        elif self.zeta.shape != (S, 6):
            raise ValueError("shape mismatch: zeta [S][6]")
        if self.want:
            self.theta = np.empty((B, S, 6))
        return dict(veh=self.veh, zeta=self.zeta, theta=self.theta)


def _mc_rng(rng, draws, independent, seed, sample_lo, plan_lo):
    """rng = "host" (the draws are made here and uploaded: None) or "device" (the lanes make them: the scvx_mc_rng of the _rng forms)"""
    if rng not in ("host", "device"):
        raise ValueError('rng: "host" or "device", not %r' % (rng,))
    if rng == "host":
        if independent:
            raise ValueError('independent=True needs rng="device": uploaded draws are shared by all plans')
        return None
    if draws is not None:
        raise ValueError('draws= cannot be combined with rng="device": the device makes its own (dynamics.mc_draws_device_batch)')
    if int(sample_lo) < 0 or int(plan_lo) < 0:
        raise ValueError("sample_lo and plan_lo must be >= 0")
    return _lib.ScvxMcRng(int(seed) & (2 ** 64 - 1), int(sample_lo), int(plan_lo), 1 if independent else 0, 0)


def mc_draws_device_batch(cache: IntegratorCache, samples, K=None, seed=0, sample_lo=0, plan_lo=0, plans=None):
    """The draws the device makes with rng="device", dumped (scvx_mc_draws_f64_host; the stream is spelled out in include/scvx.h): a dict
    of xi0, xin [samples][14] and eta, nud [samples][K][14] (all 14 draws of every node's group: a call with m measurement rows reads
    nud[..., :m]) with shared draws (plans None); plans = P: [P][samples][..], the independent draws of plans plan_lo..plan_lo+P-1.
    The same bits the flying kernels consume: track_mc_batch(..., draws=) fed them is bitwise the rng="device" call.
    montecarlo.mc_draws_device / mc_nav_draws_device are the numpy twin, a few ulp away."""
    K = int(cache.problem.K if K is None else K)
    S, P = int(samples), 1 if plans is None else int(plans)
    rg = _mc_rng("device", None, plans is not None, seed, sample_lo, plan_lo)
    out = {n: np.empty((P, S, 14) if n in ("xi0", "xin") else (P, S, K, 14)) for n in ("xi0", "eta", "xin", "nud")}
    _lib.check(cache.handle, cache._L.scvx_mc_draws_f64_host(cache.handle, C.byref(rg), P, S, K, *[_p(a) for a in out.values()]),
               "scvx_mc_draws_f64_host")
    return {n: (a[0] if plans is None else a) for n, a in out.items()}


def _mc_inputs(S0, B, K, samples, seed, w, draws, lo=0, device=False):
    """(C0 [B][14][14], xi0 [S][14], eta [S][K][14] or None, sw [14] or None) of a sampled dispersion: the factor of every plan's
    handover covariance (montecarlo.handover_factor), the draws of montecarlo.mc_draws -- or `draws` = (xi0, eta); both None with
    `device`, the lanes make them -- and sqrt(w)"""
    from .montecarlo import handover_factor, mc_draws
    s0 = _cov_s0(S0, B)
    wv = _cov_noise(w)
    c0 = np.ascontiguousarray(np.stack([handover_factor(s0[b]) for b in range(B)]))
    if device:
        if int(samples) < 1:
            raise ValueError("samples must be >= 1")
        xi0 = eta = None
    elif draws is None:
        if int(samples) < 1:
            raise ValueError("samples must be >= 1")
        xi0, eta = mc_draws(int(samples), K, seed, noise=wv is not None, lo=lo)
    else:
        xi0 = np.ascontiguousarray(draws[0], np.float64)
        eta = None if draws[1] is None else np.ascontiguousarray(draws[1], np.float64)
        if xi0.ndim != 2 or xi0.shape[1] != 14 or xi0.shape[0] < 1 or (eta is not None and eta.shape != (xi0.shape[0], K, 14)):
            raise ValueError("shape mismatch: draws = (xi0 [S][14], eta [S][K][14] or None)")
    if wv is not None and np.all(wv >= 0.0):
        sw = np.sqrt(wv)
    else:
        sw = wv   # None, or a bad w as it is: the library refuses it with its own message
    return c0, xi0, eta, sw


def _mc_keywords(rng, draws, independent, seed, sample_lo, plan_lo, vehicle, dense, quantiles, per_node):
    """the keywords every sampled call starts with -> (the scvx_mc_rng or None, the _McVeh, the _McQ); mq.rest is what is left of dense"""
    rg = _mc_rng(rng, draws, independent, seed, sample_lo, plan_lo)
    vh = _McVeh(vehicle, dense)
    return rg, vh, _McQ(quantiles, per_node, vh.rest)


def _mc_call(L, err_handle, f, B, K, samples, rg, vh, mq, seed, lo):
    """the shared end of the four sampled callers: the record f holds the head and the inputs; allocate the outputs, add the _q and _veh
    tails, choose the entry point from the record, call, build the report (a McNavReport where the record has CN)"""
    nav = "CN" in f
    S = int(samples) if rg is not None else f["xi0"].shape[0]
    reduced, dense = (_calls.MC_NAV_REDUCED, _calls.MC_NAV_DENSE) if nav else (_calls.MC_REDUCED, _calls.MC_DENSE)
    f.update(_calls.mc_outputs(B, K, S, _calls.dense_names(mq.rest, dense) | set(reduced)))
    f.update(mq.fields(B, K, S))
    f.update(vh.fields(B, S, rg, seed, lo), S=S, rng=rg, noise=1 if rg is not None and f["w14" if nav else "sw14"] is not None else 0)
    _calls.call(L, err_handle, _calls.mc_entry(f), f)
    rep = (McNavReport if nav else McReport)(*[f[k] for k in reduced + dense])
    return rep._with_q(mq)._with_veh(vh)


def track_mc_batch(cache: IntegratorCache, x, u, sigma, gain, S0, samples, seed=0, w=None, nsub=10, clamp=False, tol=0.0, dense=(),
                   draws=None, nav=None, quantiles=None, per_node=False, rng="host", independent=False, sample_lo=0,
                   plan_lo=0, vehicle=None) -> McReport:
    """Sampled closed-loop dispersion of the plans x [B][K+1][14], u [B][K+1][nu], sigma [B] tracked under the gains gain
    [B][K][nu][14+nu]: `samples` flights PER PLAN on the device, reduced there to one McReport row per plan (scvx_track_mc_f64_host;
    the model, the impulse convention and the limits are in include/scvx.h).  S0: the handover covariance, [B][14][14], one [14][14]
    for all, or a [14] vector of standard deviations; flight (b, s) starts at x[b, 0] + handover_factor(S0[b]) @ xi0[s].  The draws
    are montecarlo.mc_draws(samples, K, seed), shared by all plans.  w: process-noise variance per segment, a scalar or [14] (None =
    no noise), applied as an impulse sqrt(w) * eta at every node -- the + diag(w) of cov_propagate_batch.  clamp as track_fly_batch;
    tol: the threshold of the P_* and OUT_* columns.  dense: True, or names out of "flights", "xland", "dx0".  draws = (xi0 [S][14],
    eta [S][K][14] or None): use these instead of mc_draws (`samples` and `seed` are then ignored).  nav = (N0, H, rm): the flights
    are flown on a navigation estimate (track_mc_nav_batch on the plans' own linearisation, a McNavReport; draws then has four
    entries); None: the law is fed the truth.
    quantiles: an iterable of probabilities (at most 16): the report carries `q` [B][16][nq], the order statistics of the sixteen flight
    columns over the samples, reduced on the device (scvx_track_mc_q_f64_host; probability -> rank by montecarlo.quantile_ranks, a
    selection); per_node=True adds `pathq` [B][K+1][5][nq], those of the five path functions at every node, and dense may name "pathv"
    for the samples themselves [B][K+1][5][S].  With the clamp the THRUST function is still the unclamped command.  With these keywords
    at their defaults the call is the one it was.
    rng="device": every lane makes its own draws from a counter-based generator (scvx_track_mc_rng_f64_host; the stream is spelled out
    in include/scvx.h): nothing is generated or uploaded here, and the flights are bitwise those of the call fed
    mc_draws_device_batch's dump.  independent=True (device only): every plan flies draws of its own, plan b the stream plan_lo + b, so
    the rows of one call are independent experiments; sample_lo: the first sample, so that shards of one sample set can be flown by
    separate calls.  rng="host" (the default) makes exactly the C calls it always made; draws= cannot be combined with "device".
    vehicle = (mu, sp) (montecarlo.vehicle_errors): every flight flies a vehicle of its own, theta = mu + sp * zeta constant over the
    flight -- thrust scale, thrust misalignment, specific impulse, aerodynamic scale, fin scale (scvx_track_mc_veh_f64_host; the model
    and its limits are in include/scvx.h).  The error lies behind the command: the law, the clamp, OUT_LO / OUT_HI and the thrust
    columns see the command, the state columns and the landing statistics the vehicle that flew.  zeta [S][6] is
    montecarlo.mc_vehicle_draws of `seed` with rng="host" (or the third entry of vehicle), the device's stream 8 with "device"
    (montecarlo.mc_vehicle_draws_device is its twin); dense may name "theta" for the errors flown, `theta` [B][S][6].  None (the
    default): exactly the C calls made without it."""
    if nav is not None:
        _mc_rng(rng, draws, independent, seed, sample_lo, plan_lo)   # refused before the plan is linearised
        n0, _, Hm, rv = _nav_arg(nav, np.shape(x)[0])
        _, deriv = linearize_batch(cache, x, u, sigma, 1.0 / np.shape(x)[1])
        return track_mc_nav_batch(cache, x, u, sigma, deriv, gain, S0, n0, Hm, rv, samples, seed=seed, w=w, nsub=nsub, clamp=clamp,
                                  tol=tol, dense=dense, draws=draws, quantiles=quantiles, per_node=per_node, rng=rng,
                                  independent=independent, sample_lo=sample_lo, plan_lo=plan_lo, vehicle=vehicle)
    rg, vh, mq = _mc_keywords(rng, draws, independent, seed, sample_lo, plan_lo, vehicle, dense, quantiles, per_node)
    f = _calls.plan_shapes(cache.nu, x, u, gain, sigma=sigma)
    c0, xi0, eta, sw = _mc_inputs(S0, f["B"], f["K"], samples, seed, w, draws, sample_lo, rg is not None)
    f.update(handle=cache.handle, C0=c0, xi0=xi0, eta=eta, sw14=sw, reserved=None, nsub=cache.npts if nsub is None else nsub,
             flags=_lib.TRACK_CLAMP if clamp else 0, tol=tol)
    return _mc_call(cache._L, cache.handle, f, f["B"], f["K"], samples, rg, vh, mq, seed, sample_lo)


def vehicle_sensitivity_batch(cache: IntegratorCache, x, u, sigma, gain, h=2.0 ** -10, nsub=10, clamp=False):
    """J [B][14][6] = d x_K / d theta of the closed loop about the nominal vehicle and the planned start: central differences of step h
    from ONE sampled launch (track_mc_batch with vehicle=) -- C0 = 0, no noise, twelve flights with zeta = +-e_i, sp = h, the dense
    landings.  The column of a component the model does not have (AERO without aerodynamics, FIN without fins) is zero.  The error
    of a central difference is h^2 / 6 times the third derivative plus the flights' rounding over 2 h; montecarlo.vehicle_budget turns
    J into each component's share of the landing variance."""
    B = np.shape(x)[0]
    sp = np.full(6, float(h))
    if not isinstance(cache.problem.aero, AtmosphericData):
        sp[_lib.VEH_INDEX["AERO"]] = 0.0
    if cache.nu != 5:
        sp[_lib.VEH_INDEX["FIN"]] = 0.0
    zeta = np.zeros((12, 6))
    zeta[0::2] = np.eye(6)
    zeta[1::2] = -np.eye(6)
    rep = track_mc_batch(cache, x, u, sigma, gain, np.zeros(14), 12, nsub=nsub, clamp=clamp, dense=("xland",),
                         draws=(np.zeros((12, 14)), None), vehicle=(np.zeros(6), sp, zeta))
    J = (rep.xland[:, 0::2] - rep.xland[:, 1::2]) / (2.0 * float(h))   # [B][6][14]
    J[:, sp == 0.0] = 0.0
    return np.ascontiguousarray(np.swapaxes(J, 1, 2))


class NavReport(CovReport):
    """The two reports of a navigation-error covariance analysis (scvx_nav_cov_f64, include/scvx.h): everything a CovReport has (the
    sixteen columns read off the truth-dispersion block; `covK` and `cov` are None -- ask for `joint`), plus `navraw` [B][8] with one
    named numpy view per column (report.NAV_R, report.EST_R, ... -- _lib.NAV_COLUMNS) and the optional dense outputs `navsig`
    [B][K+1][14] (the 1 sigma of the navigation error before the update at each node), `kf` [B][K][14][m] (the filter gains) and
    `joint` [B][K+1][N][N], N = 14 + nu + 14 (the covariance of [z; eps] before the update at each node), or None."""

    def __init__(self, raw, navraw, sig=None, navsig=None, kf=None, joint=None, sens=None):
        super().__init__(raw, sig, sens=sens)
        self.navraw = np.asarray(navraw, np.float64).reshape(-1, _lib.NAV_NREP)
        self.navsig = navsig
        self.kf = kf
        self.joint = joint
        for name, i in _lib.NAV_INDEX.items():
            setattr(self, name, self.navraw[:, i])


def _nav_model(H, rm):
    """the measurement model: H [m][14] (None or no rows: no measurement) and rm, a scalar or [m] variances -> (m, H, rm), contiguous"""
    if H is None or np.size(H) == 0:
        return 0, None, None
    Hm = np.ascontiguousarray(H, np.float64)
    if Hm.ndim != 2 or Hm.shape[1] != 14:
        raise ValueError("H must be [m][14]")
    m = Hm.shape[0]
    if rm is None:
        raise ValueError("rm (the measurement variances, a scalar or [m]) is needed with H")
    r = np.asarray(rm, np.float64)
    if r.ndim > 1 or (r.ndim == 1 and r.shape[0] != m):
        raise ValueError("rm must be a scalar or have %d components" % m)
    return m, Hm, np.ascontiguousarray(np.broadcast_to(r, (m,)), np.float64)


def _nav_record(cache, x, u, deriv, gain, S0, N0, H, rm, w):
    """the checked plan and the inputs of the two navigation analyses as a record"""
    f = _calls.plan_shapes(cache.nu, x, u, gain, deriv)
    f.update(S0=_cov_s0(S0, f["B"]), N0=_cov_s0(N0, f["B"]))
    f["m"], f["H"], f["rm"] = _nav_model(H, rm)
    f["w14"] = _cov_noise(w)
    return f


def nav_cov_batch(cache: IntegratorCache, x, u, deriv, gain, S0, N0, H, rm, w=None, dense=False, vehicle=None, vtile=None) -> NavReport:
    """Covariance of the closed loop flown on a navigation ESTIMATE: the joint of the truth dispersion z and the navigation error eps
    of the plans x, u tracked under `gain` from the tiles `deriv` (all as cov_propagate_batch), on the device (scvx_nav_cov_f64_host;
    the recursion and its limits are in include/scvx.h).  S0: the handover covariance of the truth, N0: that of the navigation error
    (each [B][14][14], one [14][14], or a [14] vector of standard deviations).  H [m][14] (montecarlo.measurement_rows) and rm (variances, a
    scalar or [m]): the measurement taken at every node but the last; H None: inertial propagation only.  w: process-noise variance per
    segment, which moves the truth and is missed by the estimate alike.  dense: True for sig, navsig, kf and joint, or a subset.
    vehicle, vtile: as cov_propagate_batch (scvx_nav_cov_vehicle_f64_host): J_k diag(sp^2) J_k' is added to the truth block wherever
    the report, sig and joint read it; the eps blocks, navsig, kf and NAV_* are untouched -- the filter does not know theta -- and
    EST_R / EST_V receive it in their truth term.  dense may then name "sens"."""
    f = _nav_record(cache, x, u, deriv, gain, S0, N0, H, rm, w)
    f["sp6"], f["vtile"], f["sens"], dense = _cov_vehicle(cache, vehicle, vtile, dense, f["B"], f["K"])
    _analysis(cache, f, _calls.dense_names(dense, _calls.NAV_DENSE) | {"report", "navrep"})
    return NavReport(f["report"], f["navrep"], f["sig"], f["navsig"], f["kf"], f["joint"], f["sens"])


def _nav_arg(nav, B):
    """nav = (N0, H, rm), the navigation model of the calls that take back-offs from the navigation analysis: N0 as S0 (_cov_s0), H and
    rm as nav_cov_batch (_nav_model), with rm finite and > 0 -> (N0 [B][14][14], m, H, rm).  ValueError before any library call."""
    if not isinstance(nav, (tuple, list)) or len(nav) != 3:
        raise ValueError("nav must be (N0, H, rm)")
    N0, H, rm = nav
    if N0 is None:
        raise ValueError("nav: N0 (the handover covariance of the navigation error) is required")
    n0 = _cov_s0(N0, B)
    m, Hm, rv = _nav_model(H, rm)
    if m > 14:
        raise ValueError("H must have at most 14 rows")
    if m and not (np.all(np.isfinite(rv)) and np.all(rv > 0.0)):
        raise ValueError("rm (the measurement variances) must be finite and > 0")
    if m and not np.all(np.isfinite(Hm)):
        raise ValueError("H must be finite")
    return n0, m, Hm, rv


class McNavReport(McReport):
    """The report of a sampled dispersion flown on a navigation estimate (scvx_track_mc_nav_f64, include/scvx.h): everything a McReport
    has, plus `jmean` [B][28] and `jcov` [B][28][28], the mean and the sample covariance of [e; eps_K] (e = x_fly[K] - xbar_K the landing
    deviation, eps_K the error of the estimate there; xcov is jcov[:, :14, :14]), `navraw` [B][8] with one named numpy view per column
    (report.NAV_R, report.MAX_FED, report.EST_R, ... -- _lib.MCNAV_COLUMNS) and the optional dense outputs `navfed` [B][S][K][14] (the
    error eps+_k of the estimate the law was fed) and `navK` [B][S][14], or None."""

    def __init__(self, raw, xmean, xcov, jmean, jcov, navraw, flights=None, xland=None, dx0=None, navfed=None, navK=None):
        super().__init__(raw, xmean, xcov, flights, xland, dx0)
        self.jmean, self.jcov = jmean, jcov
        self.navraw = np.asarray(navraw, np.float64).reshape(-1, _lib.NAV_NREP)
        self.navfed, self.navK = navfed, navK
        for name, i in _lib.MCNAV_INDEX.items():
            setattr(self, name, self.navraw[:, i])


def _mc_nav_inputs(S0, N0, B, K, m, samples, seed, w, draws, lo=0, device=False):
    """(C0, CN [B][14][14], xi0, eta or None, xin, nud or None, w [14] or None) of a sampled dispersion flown on an estimate: the factors
    of every plan's two handover covariances (montecarlo.handover_factor), the draws of montecarlo.mc_draws and mc_nav_draws -- or
    `draws` = (xi0, eta, xin, nud) -- and the process-noise VARIANCE, which the library roots"""
    from .montecarlo import handover_factor, mc_draws, mc_nav_draws
    s0, n0 = _cov_s0(S0, B), _cov_s0(N0, B)
    wv = _cov_noise(w)
    c0 = np.ascontiguousarray(np.stack([handover_factor(s0[b]) for b in range(B)]))
    cn = np.ascontiguousarray(np.stack([handover_factor(n0[b]) for b in range(B)]))
    if device:   # the lanes make the four
        if int(samples) < 1:
            raise ValueError("samples must be >= 1")
        xi0 = eta = xin = nud = None
    elif draws is None:
        if int(samples) < 1:
            raise ValueError("samples must be >= 1")
        xi0, eta = mc_draws(int(samples), K, seed, noise=wv is not None, lo=lo)
        xin, nud = mc_nav_draws(int(samples), K, m, seed, lo=lo)
    else:
        if len(draws) != 4:
            raise ValueError("draws = (xi0 [S][14], eta [S][K][14] or None, xin [S][14], nud [S][K][m] or None)")
        xi0, xin = (np.ascontiguousarray(draws[i], np.float64) for i in (0, 2))
        eta, nud = (None if draws[i] is None else np.ascontiguousarray(draws[i], np.float64) for i in (1, 3))
        S = xi0.shape[0] if xi0.ndim == 2 else 0
        if (S < 1 or xi0.shape != (S, 14) or xin.shape != (S, 14) or (eta is not None and eta.shape != (S, K, 14))
                or (m > 0 and (nud is None or nud.shape != (S, K, m)))):
            raise ValueError("shape mismatch: draws = (xi0 [S][14], eta [S][K][14] or None, xin [S][14], nud [S][K][m] or None)")
    return c0, cn, n0, xi0, eta, xin, (nud if m else None), wv


def track_mc_nav_batch(cache: IntegratorCache, x, u, sigma, deriv, gain, S0, N0, H, rm, samples, seed=0, w=None, kf=None, nsub=10,
                       clamp=False, tol=0.0, dense=(), draws=None, quantiles=None, per_node=False, rng="host", independent=False,
                       sample_lo=0, plan_lo=0, vehicle=None) -> McNavReport:
    """track_mc_batch with the law fed a navigation ESTIMATE whose error is generated per flight on the device (scvx_track_mc_nav_f64_host;
    the model and its limits are in include/scvx.h): the sampled, nonlinear counterpart of nav_cov_batch, whose arguments deriv, N0, H,
    rm and w mean here what they mean there.  The error starts at handover_factor(N0[b]) @ xin[s], is corrected at every node but the
    last by the filter gains kf [B][K][14][m] with the measurement noise sqrt(rm) * nud, and receives the impulse sqrt(w) * eta that
    the truth receives.  kf None: the gains of nav_cov_batch for the same model.  The draws are montecarlo.mc_draws and
    montecarlo.mc_nav_draws of `seed`, or draws = (xi0, eta, xin, nud).  dense: True, or names out of "flights", "xland", "dx0",
    "navfed", "navK".  quantiles, per_node and the dense name "pathv" as track_mc_batch (scvx_track_mc_nav_q_f64_host): the state
    path functions are those of the TRUTH, the thrust norm that of the command formed from the estimate.  rng, independent, sample_lo
    and plan_lo as track_mc_batch (scvx_track_mc_nav_rng_f64_host): with "device" the lanes make all four draws.  vehicle and the
    dense name "theta" as track_mc_batch (scvx_track_mc_nav_veh_f64_host): the truth is flown with the vehicle errors, the recursion
    of the estimate's error is the analysis's, unchanged."""
    rg, vh, mq = _mc_keywords(rng, draws, independent, seed, sample_lo, plan_lo, vehicle, dense, quantiles, per_node)
    f = _calls.plan_shapes(cache.nu, x, u, gain, deriv, sigma)
    B, K = f["B"], f["K"]
    m, Hm, rv = _nav_model(H, rm)
    c0, cn, n0, xi0, eta, xin, nud, wv = _mc_nav_inputs(S0, N0, B, K, m, samples, seed, w, draws, sample_lo, rg is not None)
    if m and kf is None:
        kf = nav_cov_batch(cache, f["x"], f["u"], f["deriv"], f["gain"], np.zeros((B, 14, 14)), n0, Hm, rv, wv, dense=("kf",)).kf
    if m:
        kf = np.ascontiguousarray(kf, np.float64)
        if kf.shape != (B, K, 14, m):
            raise ValueError("shape mismatch: kf [B][K][14][%d]" % m)
    f.update(handle=cache.handle, C0=c0, xi0=xi0, eta=eta, w14=wv, kf=kf if m else None, CN=cn, xin=xin, nud=nud, m=m, H=Hm, rm=rv,
             nsub=cache.npts if nsub is None else nsub, flags=_lib.TRACK_CLAMP if clamp else 0, tol=tol)
    return _mc_call(cache._L, cache.handle, f, B, K, samples, rg, vh, mq, seed, sample_lo)


def nav_path_sigma_batch(cache: IntegratorCache, x, u, deriv, gain, S0, N0, H, rm, w=None, vehicle=None, vtile=None, dense=()):
    """What the margins of nav_cov_batch are made of (scvx_nav_path_sigma_f64_host; same arguments without dense): (NavReport, psig) with
    psig [B][K+1][5] as cov_path_sigma_batch, read off the TRUTH block of the joint covariance before the update at each node -- the
    constraints bind the vehicle, not its estimate.  Node 0 and a node its margin skips are 0; a non-finite tile, gain, S0 or N0 entry
    makes the rows of its own trajectory NaN.  With N0 = 0 this is cov_path_sigma_batch's psig to rounding.
    vehicle, vtile: as nav_cov_batch (psig and the report are then read off the truth block + J_k diag(sp^2) J_k'); dense: () or ("sens",)."""
    f = _nav_record(cache, x, u, deriv, gain, S0, N0, H, rm, w)
    f["sp6"], f["vtile"], f["sens"], dense = _cov_vehicle(cache, vehicle, vtile, dense, f["B"], f["K"])
    if dense:
        raise ValueError('dense: () or ("sens",), not %r' % (dense,))
    _analysis(cache, f, {"report", "navrep", "psig"})
    return NavReport(f["report"], f["navrep"], sens=f["sens"]), f["psig"]


def _pf(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def linearize_batch_f32(cache: IntegratorCache, x, u, sigma, dt):
    """fp32 form (scvx_linearize_f32_host): float arrays in and out, float arithmetic on the device."""
    x = np.ascontiguousarray(x, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    sigma = np.ascontiguousarray(sigma, np.float32)
    B, K1, nx = x.shape
    K = K1 - 1
    if nx != 14 or u.shape != (B, K1, cache.nu) or sigma.shape != (B,):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    e = np.empty((B, K, 14), np.float32)
    d = np.empty((B, K, cache.np, 14), np.float32)
    _lib.check(cache.handle, cache._L.scvx_linearize_f32_host(cache.handle, B, K, _pf(x), _pf(u), _pf(sigma), float(dt),
                                                              _pf(e), _pf(d)), "scvx_linearize_f32_host")
    return e, d


def propagate_batch_f32(cache: IntegratorCache, x, u, sigma, dt):
    x = np.ascontiguousarray(x, np.float32)
    u = np.ascontiguousarray(u, np.float32)
    sigma = np.ascontiguousarray(sigma, np.float32)
    B, K1, nx = x.shape
    K = K1 - 1
    if nx != 14 or u.shape != (B, K1, cache.nu) or sigma.shape != (B,):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d], sigma [B]" % cache.nu)
    e = np.empty((B, K, 14), np.float32)
    _lib.check(cache.handle, cache._L.scvx_propagate_f32_host(cache.handle, B, K, _pf(x), _pf(u), _pf(sigma), float(dt),
                                                              _pf(e)), "scvx_propagate_f32_host")
    return e


def make_state(a: LinPoint, b: LinPoint, sig: float):
    """dynamics.jl:318-320"""
    return np.concatenate([a.state, a.control, b.control, [sig]])


def linearize_dynamics(states, tf_guess: float, base_dt: float, cache: IntegratorCache):
    """dynamics.jl:321-334: K+1 LinPoints -> K LinRes."""
    x = np.stack([s.state for s in states])[None]
    u = np.stack([s.control for s in states])[None]
    e, d = linearize_batch(cache, x, u, np.array([tf_guess]), base_dt)
    return [LinRes(e[0, k].copy(), d[0, k].T.copy()) for k in range(len(states) - 1)]


def predict_state(initial_state, uk, up, sigma, dt, pinfo, cache: IntegratorCache):
    """dynamics.jl:315-317: state at the end of one segment."""
    x = np.zeros((1, 2, 14))
    u = np.zeros((1, 2, cache.nu))
    x[0, 0] = initial_state
    u[0, 0] = uk
    u[0, 1] = up
    return propagate_batch(cache, x, u, np.array([float(sigma)]), dt)[0, 0]


def next_step(dynam, ab, abn, state, control_k, control_kp, sigma, sigHat, relax):
    """autodiff_dynamics.jl:104-107 / old_dynamics.jl:150-153: the affine prediction of the next node from a LinRes,
    derivative * [dx; du_k; du_{k+1}; dsigma] + endpoint + relax (host-side helper, a 14x21 product)."""
    ctrl = np.concatenate([np.asarray(state) - ab.state, np.asarray(control_k) - ab.control,
                           np.asarray(control_kp) - abn.control, [sigma - sigHat]])
    return dynam.derivative @ ctrl + dynam.endpoint + relax
