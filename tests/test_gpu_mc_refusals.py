"""What the eight batch-level forms of the sampled closed-loop dispersion (scvx_batch_track_mc[_nav][_q|_rng|_veh]) refuse, in which
words, and which fault wins when two are present: the case table of tests/host_staging_asan.cpp (its context-level forms cannot link
scvx_batch.hip), restricted to what a batch form takes from the caller -- the plan, the gains, the tiles, kf and the shape are the
batch's own -- plus N0, the tracking weights and a batch that was never initialised.  One exo batch, B = 2, K = 3, S = 2, through ctypes.

Every form starts from one valid call; one argument (or two) is made bad; (rc, scvx_last_error) of every case is required to equal
tests/golden/mc_batch_refusals.txt, recorded on the MI355X with the library as it stood before check_mc_call replaced the checks of the
six hand-written bodies.  A refused call enqueues nothing: the outputs keep their fill, and the file runs in about a second."""
import ctypes as C
import os
from dataclasses import replace

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

B, K, S = 2, 3, 2
F_NAV, F_Q, F_UP, F_RNG, F_VEH, F_TRUTH, F_M = 1, 2, 4, 8, 16, 32, 64
# (entry point, traits); the _veh forms twice: on uploaded draws and with rng
FORMS = (("scvx_batch_track_mc", F_TRUTH | F_UP), ("scvx_batch_track_mc_q", F_TRUTH | F_UP | F_Q),
         ("scvx_batch_track_mc_rng", F_TRUTH | F_RNG | F_Q), ("scvx_batch_track_mc_veh", F_TRUTH | F_UP | F_Q | F_VEH),
         ("scvx_batch_track_mc_veh", F_TRUTH | F_RNG | F_Q | F_VEH), ("scvx_batch_track_mc_nav", F_NAV | F_UP),
         ("scvx_batch_track_mc_nav_q", F_NAV | F_UP | F_Q), ("scvx_batch_track_mc_nav_rng", F_NAV | F_RNG | F_Q),
         ("scvx_batch_track_mc_nav_veh", F_NAV | F_UP | F_Q | F_VEH), ("scvx_batch_track_mc_nav_veh", F_NAV | F_RNG | F_Q | F_VEH))
NAN = float("nan")
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)


def _args(traits, m):
    """every argument of a valid call of a form with these traits; the outputs are filled with 7"""
    from successiveconvexification_amd import _lib
    up, eye = bool(traits & F_UP), np.ascontiguousarray(np.stack([np.eye(14) * 1e-6] * B))
    a = dict(q=np.ones(14), r=np.ones(3), qf=np.full(14, 100.0), S=S, C0=eye, xi0=np.zeros((S, 14)) if up else None,
             eta=np.zeros((S, K, 14)) if up else None, w=np.full(14, 1e-6), reserved=None, nsub=10, flags=0, tol=0.0, N0=eye.copy(),
             CN=eye.copy(), xin=np.zeros((S, 14)) if up else None, nud=np.zeros((S, K, m)) if up and m else None, m=m,
             H=np.ascontiguousarray(np.eye(14)[1:1 + m]) if m else None, rm=np.full(m, 1e-6) if m else None, nq=1,
             ranks=np.array([1], np.int32), rng=None, noise=0, veh=None, zeta=None, theta=None)
    for name, shape in (("mcrep", (B, 48)), ("xmean", (B, 14)), ("xcov", (B, 14, 14)), ("jmean", (B, 28)), ("jcov", (B, 28, 28)),
                        ("mcnav", (B, 8)), ("flightq", (B, 16, 1)), ("pathq", (B, K + 1, 5, 1))):
        a[name] = np.full(shape, 7.0)
    if traits & F_RNG:
        a["rng"], a["noise"] = _lib.ScvxMcRng(20261020, 0, 0, 0, 0), 1
    if traits & F_VEH:
        a["veh"] = _lib.ScvxMcVehicle((C.c_double * 6)(1e-3, 0, 0, 0, 0, 0), (C.c_double * 6)(1e-3, 0, 0, 0, 0, 0), (C.c_int32 * 2)(0, 0))
        a["zeta"], a["theta"] = np.zeros((S, 6)) if up else None, np.full((B, S, 6), 7.0)
    return a


def _call(L, handle, name, traits, a):
    p = lambda k: None if a[k] is None else a[k].ctypes.data_as(_dp)   # noqa: E731
    ref = lambda k: None if a[k] is None else C.byref(a[k])            # noqa: E731
    own_rng = bool(traits & F_RNG) and not traits & F_VEH               # the _rng forms: (rng, noise) where the others have (xi0, eta)
    head = [handle, p("q"), p("r"), p("qf"), a["S"], p("C0")] + ([ref("rng"), a["noise"]] if own_rng else [p("xi0"), p("eta")])
    out, dense = [p("mcrep"), p("xmean"), p("xcov")], [None, None, None]
    if traits & F_NAV:
        mid = [p("w"), p("N0"), p("CN")] + ([] if own_rng else [p("xin"), p("nud")]) + [a["m"], p("H"), p("rm"), a["nsub"], a["flags"], a["tol"]]
        mid += out + [p("jmean"), p("jcov"), p("mcnav")] + dense + [None, None]
    else:
        mid = [p("w"), a["reserved"], a["nsub"], a["flags"], a["tol"]] + out + dense
    qt = [a["nq"], None if a["ranks"] is None else a["ranks"].ctypes.data_as(_ip), p("flightq"), p("pathq"), None] if traits & F_Q else []
    vt = [ref("rng"), a["noise"], ref("veh"), p("zeta"), p("theta")] if traits & F_VEH else []
    return getattr(L, name)(*head, *mid, *qt, *vt)


def _w(i, v):
    w = np.full(14, 1e-6)
    w[i] = v
    return w


def _veh(a, field, i, v):
    getattr(a["veh"], field)[i] = v


# (case, traits a form needs for it, what makes the argument bad)
FAULTS = (
    ("q=NULL", 0, lambda a: a.update(q=None)), ("r=NULL", 0, lambda a: a.update(r=None)), ("qf=NULL", 0, lambda a: a.update(qf=None)),
    ("q<0", 0, lambda a: a.update(q=_w(2, -1.0))), ("r=0", 0, lambda a: a.update(r=np.array([1.0, 0.0, 1.0]))),
    ("qf=NaN", 0, lambda a: a.update(qf=_w(13, NAN))),
    ("C0=NULL", 0, lambda a: a.update(C0=None)), ("xi0=NULL", F_UP, lambda a: a.update(xi0=None)),
    ("N0=NULL", F_NAV, lambda a: a.update(N0=None)), ("CN=NULL", F_NAV, lambda a: a.update(CN=None)),
    ("xin=NULL", F_NAV | F_UP, lambda a: a.update(xin=None)),
    ("S=0", 0, lambda a: a.update(S=0)), ("nsub=-1", 0, lambda a: a.update(nsub=-1)), ("nsub=1001", 0, lambda a: a.update(nsub=1001)),
    ("flags=2", 0, lambda a: a.update(flags=2)), ("tol=-1", 0, lambda a: a.update(tol=-1.0)), ("tol=NaN", 0, lambda a: a.update(tol=NAN)),
    ("w<0", 0, lambda a: a.update(w=_w(2, -1e-6))), ("w=NaN", 0, lambda a: a.update(w=_w(1, NAN))),
    ("eta-without-w", 0, lambda a: a.update(w=None)), ("reserved", F_TRUTH, lambda a: a.update(reserved=C.c_void_p(1))),
    ("rng=NULL", F_RNG, lambda a: a.update(rng=None)),   # at a _veh form this is the call on uploaded draws with noise: refused as such
    ("rng.reserved=1", F_RNG, lambda a: setattr(a["rng"], "reserved", 1)),
    ("rng.independent=2", F_RNG, lambda a: setattr(a["rng"], "independent", 2)),
    ("nq=0", F_Q, lambda a: a.update(nq=0)), ("nq=17", F_Q, lambda a: a.update(nq=17)), ("ranks=NULL", F_Q, lambda a: a.update(ranks=None)),
    ("rank=-1", F_Q, lambda a: a.update(ranks=np.array([-1], np.int32))), ("rank=S", F_Q, lambda a: a.update(ranks=np.array([S], np.int32))),
    ("zeta-without-veh", F_VEH | F_UP, lambda a: a.update(veh=None, theta=None)),
    ("theta-without-veh", F_VEH, lambda a: a.update(veh=None, zeta=None)),
    ("veh.reserved=1", F_VEH, lambda a: _veh(a, "reserved", 1, 1)), ("veh.mu=NaN", F_VEH, lambda a: _veh(a, "mu", 3, NAN)),
    ("veh.sp<0", F_VEH, lambda a: _veh(a, "sp", 3, -1.0)), ("veh.sp=NaN", F_VEH, lambda a: _veh(a, "sp", 3, NAN)),
    ("veh.aero", F_VEH, lambda a: _veh(a, "mu", 4, 1e-3)), ("veh.fin", F_VEH, lambda a: _veh(a, "sp", 5, 1e-3)),
    ("veh.sp-without-zeta", F_VEH | F_UP, lambda a: a.update(zeta=None)),
    ("rng+xi0", F_VEH | F_RNG, lambda a: a.update(xi0=np.zeros((S, 14)))), ("rng+zeta", F_VEH | F_RNG, lambda a: a.update(zeta=np.zeros((S, 6)))),
    ("noise-without-rng", F_VEH | F_UP, lambda a: a.update(noise=1)),
    ("m=-1", F_NAV, lambda a: a.update(m=-1)), ("m=15", F_NAV, lambda a: a.update(m=15)),
    ("H=NULL", F_NAV | F_M, lambda a: a.update(H=None)), ("rm=NULL", F_NAV | F_M, lambda a: a.update(rm=None)),
    ("rm=0", F_NAV | F_M, lambda a: a.update(rm=np.zeros(a["m"]))), ("nud=NULL", F_NAV | F_M | F_UP, lambda a: a.update(nud=None)),
)
# two faults at once: the first named belongs to the earlier check
PAIRS = (("q=NULL", "S=0"), ("r=0", "C0=NULL"), ("noise-without-rng", "q=NULL"), ("rng+zeta", "qf=NaN"), ("S=0", "rng.reserved=1"),
         ("C0=NULL", "rng.independent=2"), ("S=0", "nq=17"), ("xi0=NULL", "rank=S"), ("S=0", "veh.reserved=1"),
         ("C0=NULL", "theta-without-veh"), ("C0=NULL", "w<0"), ("w<0", "reserved"), ("S=0", "m=15"), ("w=NaN", "m=15"), ("m=-1", "CN=NULL"),
         ("CN=NULL", "nud=NULL"), ("nud=NULL", "N0=NULL"), ("N0=NULL", "rng.reserved=1"), ("N0=NULL", "nq=0"),
         ("rng.reserved=1", "nq=0"), ("rank=-1", "veh.mu=NaN"), ("rng.independent=2", "veh.fin"), ("tol=NaN", "xin=NULL"))


def refusal_lines(L, ctx, batch, fresh):
    """the lines of every case: `batch` initialised, `fresh` never; ends with the valid calls, the only ones that enqueue anything"""
    faults = {name: (need, make) for name, need, make in FAULTS}
    lines, valid = [], []
    for entry, base in FORMS:
        for m in (0, 2) if base & F_NAV else (0,):
            traits = base | (F_M if m else 0)
            label = entry + ("+rng" if base & F_VEH and base & F_RNG else "")
            applies = lambda name: faults[name][0] & traits == faults[name][0]   # noqa: E731
            cases = [(n,) for n, _, _ in FAULTS if applies(n)] + [p for p in PAIRS if applies(p[0]) and applies(p[1])]
            for case in cases + [("uninitialised",)]:
                a = _args(traits, m)
                for name in case:
                    if name in faults:
                        faults[name][1](a)
                rc = _call(L, fresh if case == ("uninitialised",) else batch, entry, traits, a)
                lines.append("refusal %s m=%d/%s %d %s" % (label, m, "+".join(case), rc, L.scvx_last_error(ctx).decode()))
                assert all(np.all(a[k] == 7.0) for k in ("mcrep", "xmean", "xcov", "jmean", "jcov", "mcnav", "flightq", "pathq")), lines[-1]
            valid.append("refusal %s m=%d/valid %d -" % (label, m, _call(L, batch, entry, traits, _args(traits, m))))
    return lines + valid


def run_cases():
    """(lines) on a fresh exo problem at K = 3"""
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    c = IntegratorCache(replace(sp.base_prob_scaled, K=K), npts=10)
    b, fresh = ScvxBatch(c, B).init(None), ScvxBatch(c, B)
    try:
        return refusal_lines(c._L, c.handle, b.handle, fresh.handle)
    finally:
        b.close(), fresh.close(), c.close()


def test_batch_refusals_equal_the_recorded_ones():
    got = run_cases()
    with open(os.path.join(GOLDEN, "mc_batch_refusals.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 500 and all(line.startswith("refusal scvx_batch_track_mc") for line in want)
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    assert all(line.endswith(" 0 -") for line in got if "/valid " in line) and sum("/valid " in line for line in got) == 15
