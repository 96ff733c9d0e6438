"""One table and one dispatcher for the Python binding of the two wide call families of include/scvx.h: the first-order analyses
(covariance, navigation, their vehicle-error, clamp-aware and path-sigma forms, the back-offs taken from them) and the sampled
closed-loop dispersion (nav? x plain / _q / _rng / _veh), each in its context (_f64_host) and its batch (scvx_batch_) form.

A caller fills a record -- a dict keyed by the header's own parameter names -- and `call` lays it out in the order of TABLE, so no
argument list is assembled by hand and none can be passed at the wrong position: tests/test_py_call_table_cpu.py holds every tuple of
TABLE against the parameter list parsed from include/scvx.h and against _lib.SIGNATURES.
"""
import ctypes as C

import numpy as np

from . import _lib

# ---- the runs the argument lists are made of, named once -------------------------------------------------------------------------
_PLAN = ("B", "K", "x", "u", "deriv", "gain")                   # the context head of the analyses
_WEIGHTS = ("q14", "rNU", "qf14")                               # the batch head: the LQR weights of the batch's own gains
_COV_IN, _NAV_IN = ("S0", "w14"), ("S0", "N0", "m", "H", "rm", "w14")
_COV_OUT, _NAV_OUT = ("sig", "covK", "cov"), ("sig", "navsig", "kf", "joint")
_CLAMP = ("S0", "w14", "band2", "report", "satrep", "mean") + _COV_OUT + ("satk",)
_VEH_TILES = ("vtile", "sp6", "sens")
_MARGINS = ("nsigma", "cap", "which", "psig")
_MC_CTX, _MC_BATCH = ("B", "K", "S", "x", "u", "sigma", "gain", "C0"), _WEIGHTS + ("S", "C0")
_MC_MID = ("sw14", "reserved", "nsub", "flags", "tol", "mcrep", "xmean", "xcov", "flights", "xland", "dx0")
_MC_NAV_TAIL = ("m", "H", "rm", "nsub", "flags", "tol", "mcrep", "xmean", "xcov", "jmean", "jcov", "mcnav", "flights", "xland", "dx0", "navfed",
                "navK")
_MC_Q = ("nq", "ranks", "flightq", "pathq", "pathv")
_MC_VEH = ("rng", "noise", "veh", "zeta", "theta")

TABLE = {
    "scvx_cov_propagate_f64_host": _PLAN + _COV_IN + ("report",) + _COV_OUT,
    "scvx_cov_path_sigma_f64_host": _PLAN + _COV_IN + ("report", "psig"),
    "scvx_cov_vehicle_f64_host": _PLAN + _COV_IN + ("report", "psig") + _COV_OUT + _VEH_TILES,
    "scvx_cov_clamp_f64_host": _PLAN + _CLAMP,
    "scvx_nav_cov_f64_host": _PLAN + _NAV_IN + ("report", "navrep") + _NAV_OUT,
    "scvx_nav_path_sigma_f64_host": _PLAN + _NAV_IN + ("report", "navrep", "psig"),
    "scvx_nav_cov_vehicle_f64_host": _PLAN + _NAV_IN + ("report", "navrep", "psig") + _NAV_OUT + _VEH_TILES,
    "scvx_batch_cov": _WEIGHTS + _COV_IN + ("report",) + _COV_OUT,
    "scvx_batch_cov_veh": _WEIGHTS + _COV_IN + ("report",) + _COV_OUT + ("sp6",),
    "scvx_batch_cov_clamp": _WEIGHTS + _CLAMP,
    "scvx_batch_nav_cov": _WEIGHTS + _NAV_IN + ("report", "navrep") + _NAV_OUT,
    "scvx_batch_nav_cov_veh": _WEIGHTS + _NAV_IN + ("report", "navrep") + _NAV_OUT + ("sp6",),
    "scvx_batch_thrust_margins_from_cov": _WEIGHTS + _COV_IN + ("nsigma", "cap", "psig"),
    "scvx_batch_margins_from_cov": _WEIGHTS + _COV_IN + _MARGINS,
    "scvx_batch_margins_from_cov_veh": _WEIGHTS + _COV_IN + _MARGINS + ("sp6",),
    "scvx_batch_margins_from_nav": _WEIGHTS + _NAV_IN + _MARGINS,
    "scvx_batch_margins_from_nav_veh": _WEIGHTS + _NAV_IN + _MARGINS + ("sp6",),
}
for _batch, _head in ((False, _MC_CTX), (True, _MC_BATCH)):
    for _nav in (False, True):
        for _form in ("", "_q", "_rng", "_veh"):
            _draws = ("rng", "noise") if _form == "_rng" else ("xi0", "eta")
            _own = () if _form == "_rng" else ("xin", "nud")          # the _rng forms make the estimate's draws too
            _mid = (("w14", "N0" if _batch else "deriv") + (() if _batch else ("kf",)) + ("CN",) + _own + _MC_NAV_TAIL) if _nav else _MC_MID
            _name = ("scvx_batch_track_mc%s%s" if _batch else "scvx_track_mc%s%s_f64_host") % ("_nav" if _nav else "", _form)
            TABLE[_name] = _head + _draws + _mid + (_MC_Q if _form else ()) + (_MC_VEH if _form == "_veh" else ())


def _converter(kind):
    """field -> C argument for a position of the kind _lib.SIGNATURES declares: an array becomes a pointer and None stays None, a struct
    goes by reference, a scalar is coerced to int or float; the reserved void pointer passes what it is given"""
    if kind in (C.c_int, C.c_uint):
        return int
    if kind is C.c_double:
        return float
    if kind is C.c_void_p:
        return lambda v: v
    if issubclass(kind._type_, C.Structure):
        return lambda v: None if v is None else C.byref(v)
    return lambda v: None if v is None else v.ctypes.data_as(kind)


# The segment audit and the back-offs taken from it go through the same dispatcher.  They are a family of their own, so they stand beside
# TABLE, which holds exactly the two wide families.
AUDIT_TABLE = {
    "scvx_segment_audit_f64_host": ("B", "K", "x", "u", "sigma", "nsub", "seg", "report"),
    "scvx_batch_segment_audit": ("nsub", "seg", "report"),
    "scvx_batch_audit_margins": ("nsub", "which", "gain", "tol", "cap", "seg"),
}

_LAYOUT = {name: tuple(zip(fields, [_converter(k) for k in _lib.SIGNATURES[name][1][1:]]))
           for name, fields in {**TABLE, **AUDIT_TABLE}.items()}


def call(L, err_handle, name, fields):
    """Make the call `name` of TABLE on the library L: fields["handle"] (the context or the batch) first, then every field TABLE names,
    each turned into its C argument by the kind _lib.SIGNATURES gives its position.  A field the table names but the record lacks is a
    KeyError.  A non-zero return raises through _lib.check with the entry point's name and the message of the context `err_handle`."""
    args = [convert(fields[key]) for key, convert in _LAYOUT[name]]
    _lib.check(err_handle, getattr(L, name)(fields["handle"], *args), name)


def mc_entry(f):
    """the sampled entry point a record asks for: nav? (it has CN) x veh / rng / q / plain, x context / batch (it has q14)"""
    form = ("_veh" if f["veh"] is not None else "_rng" if f["rng"] is not None else "_q" if f["nq"] or f["pathv"] is not None else "")
    return ("scvx_batch_track_mc%s%s" if "q14" in f else "scvx_track_mc%s%s_f64_host") % ("_nav" if "CN" in f else "", form)


def analysis_entry(f):
    """the analysis entry point a record asks for: nav? (it has N0) x vehicle (sp6) / clamp (satrep) / path-sigma (psig) / plain, x
    context / batch (it has q14); a batch record with nsigma asks for the back-offs, `which` None for the thrust band alone"""
    nav, veh, clamp = "N0" in f, f.get("sp6") is not None, f.get("satrep") is not None
    if "q14" not in f:
        if veh:
            return "scvx_nav_cov_vehicle_f64_host" if nav else "scvx_cov_vehicle_f64_host"
        if clamp:
            return "scvx_cov_clamp_f64_host"
        if f["psig"] is not None:
            return "scvx_nav_path_sigma_f64_host" if nav else "scvx_cov_path_sigma_f64_host"
        return "scvx_nav_cov_f64_host" if nav else "scvx_cov_propagate_f64_host"
    if "nsigma" in f:
        if f["which"] is None and not nav and not veh:
            return "scvx_batch_thrust_margins_from_cov"
        return "scvx_batch_margins_from_%s%s" % ("nav" if nav else "cov", "_veh" if veh else "")
    return "scvx_batch_%s%s" % ("nav_cov" if nav else "cov", "_veh" if veh else "_clamp" if clamp else "")


COV_DENSE, CLAMP_DENSE, NAV_DENSE = ("sig", "covK", "cov"), ("mean", "sig", "covK", "cov", "satk"), ("sig", "navsig", "kf", "joint")
MC_REDUCED, MC_DENSE = ("mcrep", "xmean", "xcov"), ("flights", "xland", "dx0")
MC_NAV_REDUCED, MC_NAV_DENSE = MC_REDUCED + ("jmean", "jcov", "mcnav"), MC_DENSE + ("navfed", "navK")


def split_dense(dense, aside):
    """The set-aside step of `dense` = True / False / () / a name / an iterable of names -> (the names of `aside` it asks for, what is
    left of it for dense_names).  True stays True and asks for none of `aside`: those outputs are by name only."""
    if dense is True or not dense:
        return set(), dense
    names = {dense} if isinstance(dense, str) else set(dense)
    return names & set(aside), tuple(n for n in names if n not in aside)


def dense_names(dense, allowed):
    """The one `dense` normaliser: True = all of `allowed`, False / () = none, a name or an iterable of names = those -> the set of
    wanted outputs; a name outside `allowed` is refused."""
    if dense is True:
        return set(allowed)
    if not dense:
        return set()
    want = {dense} if isinstance(dense, str) else set(dense)
    if not want <= set(allowed):
        raise ValueError("dense: True, False or names out of %s, not %r" % (", ".join(repr(n) for n in allowed), dense))
    return want


def plan_shapes(nu, x, u, gain, deriv=None, sigma=None):
    """The one shape check of the plans of both families: x [B][K+1][14], u [B][K+1][nu], gain [B][K][nu][14+nu], and with them deriv
    [B][K][14+2nu+1][14] (the analyses, the estimate-fed flights) and sigma [B] (the flights) -> the record's head: B, K and the
    contiguous arrays."""
    f = dict(x=x, u=u, sigma=sigma, gain=gain, deriv=deriv)
    f = {k: np.ascontiguousarray(v, np.float64) for k, v in f.items() if v is not None}
    x = f["x"]
    if (x.ndim != 3 or x.shape[2] != 14 or f["u"].shape != (x.shape[0], x.shape[1], nu)
            or (sigma is not None and f["sigma"].shape != (x.shape[0],))):
        raise ValueError("shape mismatch: x [B][K+1][14], u [B][K+1][%d]%s" % (nu, ", sigma [B]" if sigma is not None else ""))
    B, K = x.shape[0], x.shape[1] - 1
    if f["gain"].shape != (B, K, nu, 14 + nu):
        raise ValueError("shape mismatch: gain [B][K][%d][%d]" % (nu, 14 + nu))
    if deriv is not None and (f["deriv"].size != B * K * 14 * (15 + 2 * nu) or f["deriv"].shape[-2:] != (15 + 2 * nu, 14)):
        raise ValueError("shape mismatch: deriv [B][K][%d][14]" % (15 + 2 * nu))
    return dict(f, B=B, K=K)


def analysis_outputs(B, K, nu, names, m=0):
    """{name: a fresh array, or None where `names` lacks it} over every output of the analyses but sens (_cov_vehicle's)"""
    n = 14 + nu
    shapes = {"report": (B, _lib.COV_NREP), "navrep": (B, _lib.NAV_NREP), "satrep": (B, _lib.SAT_NREP), "psig": (B, K + 1, _lib.PSIG_N),
              "mean": (B, K + 1, n), "sig": (B, K + 1, n), "covK": (B, n, n), "cov": (B, K + 1, n, n), "satk": (B, K, 4),
              "navsig": (B, K + 1, 14), "kf": (B, K, 14, m), "joint": (B, K + 1, n + 14, n + 14)}
    return {k: np.empty(s) if k in names else None for k, s in shapes.items()}


def mc_outputs(B, K, S, names, nq=0):
    """{name: a fresh array, or None where `names` lacks it} over every output of the sampled calls"""
    shapes = {"mcrep": (B, _lib.MC_NREP), "xmean": (B, 14), "xcov": (B, 14, 14), "jmean": (B, 28), "jcov": (B, 28, 28),
              "mcnav": (B, _lib.NAV_NREP), "flights": (B, S, _lib.FLIGHT_NREP), "xland": (B, S, 14), "dx0": (B, S, 14),
              "navfed": (B, S, K, 14), "navK": (B, S, 14), "flightq": (B, _lib.FLIGHT_NREP, nq), "pathq": (B, K + 1, _lib.PSIG_N, nq),
              "pathv": (B, K + 1, _lib.PSIG_N, S), "theta": (B, S, _lib.VEH_N)}
    return {k: np.empty(s) if k in names else None for k, s in shapes.items()}
