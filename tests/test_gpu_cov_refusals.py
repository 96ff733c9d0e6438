"""What the nine batch-level forms of the covariance and navigation analyses (scvx_batch_cov[_veh], scvx_batch_nav_cov[_veh],
scvx_batch_margins_from_{cov,nav}[_veh], scvx_batch_thrust_margins_from_cov) refuse, in which words, and which fault wins when two
are present: the case table of cov_refusals() in tests/host_staging_asan.cpp (its context-level forms cannot link scvx_batch.hip),
restricted to what a batch form takes from the caller -- the plan, the gains, the tiles, the vehicle tiles and the shape are the
batch's own -- plus the tracking weights, nsigma, cap, which and a batch that was never initialised.  One exo batch, B = 2, K = 3,
through ctypes.

Every form starts from one valid call; one argument (or two) is made bad; (rc, scvx_last_error) of every case is required to equal
tests/golden/cov_batch_refusals.txt, recorded on the MI355X with the library as it stood before check_cov_call replaced the checks of
the hand-written bodies.  Among what only line order defined there: scvx_batch_[nav_]cov_veh refuse a bad vehicle before bad tracking
weights, the margins calls the other way round.  A refused call enqueues nothing: the outputs keep their fill, and the file runs in
about a second."""
import ctypes as C
import os
from dataclasses import replace

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

B, K = 2, 3
F_NAV, F_VEH, F_MARG, F_WHICH, F_M = 1, 2, 4, 8, 16
FORMS = (("scvx_batch_cov", 0), ("scvx_batch_cov_veh", F_VEH), ("scvx_batch_nav_cov", F_NAV), ("scvx_batch_nav_cov_veh", F_NAV | F_VEH),
         ("scvx_batch_margins_from_cov", F_MARG | F_WHICH), ("scvx_batch_margins_from_nav", F_MARG | F_WHICH | F_NAV),
         ("scvx_batch_margins_from_cov_veh", F_MARG | F_WHICH | F_VEH), ("scvx_batch_margins_from_nav_veh", F_MARG | F_WHICH | F_NAV | F_VEH),
         ("scvx_batch_thrust_margins_from_cov", F_MARG))
OUTPUTS = ("report", "navrep", "sig", "navsig", "covK", "cov", "kf", "joint", "psig")
NAN = float("nan")
_dp = C.POINTER(C.c_double)


def _args(m):
    """every argument of a valid call; the outputs are filled with 7"""
    eye = np.ascontiguousarray(np.stack([np.eye(14) * 1e-6] * B))
    a = dict(q=np.ones(14), r=np.ones(3), qf=np.full(14, 100.0), S0=eye, N0=eye.copy(), m=m,
             H=np.ascontiguousarray(np.eye(14)[1:1 + m]) if m else None, rm=np.full(m, 1e-6) if m else None, w=np.full(14, 1e-6),
             sp=np.array([1e-3, 0.0, 0.0, 1e-3, 0.0, 0.0]), nsigma=3.0, cap=0.25, which=31)
    for name, shape in (("report", (B, 16)), ("navrep", (B, 8)), ("sig", (B, K + 1, 17)), ("navsig", (B, K + 1, 14)), ("covK", (B, 17, 17)),
                        ("cov", (B, K + 1, 17, 17)), ("kf", (B, K, 14, max(m, 1))), ("joint", (B, K + 1, 31, 31)), ("psig", (B, K + 1, 5))):
        a[name] = np.full(shape, 7.0)
    return a


def _call(L, handle, name, traits, a):
    p = lambda k: None if a[k] is None else a[k].ctypes.data_as(_dp)   # noqa: E731
    head = [handle, p("q"), p("r"), p("qf"), p("S0")] + ([p("N0"), a["m"], p("H"), p("rm")] if traits & F_NAV else []) + [p("w")]
    if traits & F_MARG:
        tail = [a["nsigma"], a["cap"]] + ([a["which"]] if traits & F_WHICH else []) + [p("psig")]
    elif traits & F_NAV:
        tail = [p("report"), p("navrep"), p("sig"), p("navsig"), p("kf") if a["m"] > 0 else None, p("joint")]
    else:
        tail = [p("report"), p("sig"), p("covK"), p("cov")]
    return getattr(L, name)(*head, *tail, *([p("sp")] if traits & F_VEH else []))


def _v(n, fill, i, v):
    w = np.full(n, fill)
    w[i] = v
    return w


def _sp(i, v):
    sp = np.array([1e-3, 0.0, 0.0, 1e-3, 0.0, 0.0])
    sp[i] = v
    return sp


def _h(a, v):
    h = a["H"].copy()
    h[1, 1] = v
    return h


# (case, traits a form needs for it, what makes the argument bad)
FAULTS = (
    ("q=NULL", 0, lambda a: a.update(q=None)), ("r=NULL", 0, lambda a: a.update(r=None)), ("qf=NULL", 0, lambda a: a.update(qf=None)),
    ("q<0", 0, lambda a: a.update(q=_v(14, 1.0, 2, -1.0))), ("r=0", 0, lambda a: a.update(r=np.array([1.0, 0.0, 1.0]))),
    ("qf=NaN", 0, lambda a: a.update(qf=_v(14, 100.0, 13, NAN))),
    ("S0=NULL", 0, lambda a: a.update(S0=None)), ("N0=NULL", F_NAV, lambda a: a.update(N0=None)),
    ("w<0", 0, lambda a: a.update(w=_v(14, 1e-6, 2, -1e-6))), ("w=NaN", 0, lambda a: a.update(w=_v(14, 1e-6, 1, NAN))),
    ("m=-1", F_NAV, lambda a: a.update(m=-1)), ("m=15", F_NAV, lambda a: a.update(m=15)),
    ("H=NULL", F_NAV | F_M, lambda a: a.update(H=None)), ("rm=NULL", F_NAV | F_M, lambda a: a.update(rm=None)),
    ("rm=0", F_NAV | F_M, lambda a: a.update(rm=_v(2, 1e-6, 1, 0.0))), ("rm=NaN", F_NAV | F_M, lambda a: a.update(rm=_v(2, 1e-6, 0, NAN))),
    ("H=NaN", F_NAV | F_M, lambda a: a.update(H=_h(a, NAN))),
    ("sp6=NULL", F_VEH, lambda a: a.update(sp=None)), ("sp<0", F_VEH, lambda a: a.update(sp=_sp(1, -1e-3))),
    ("sp=NaN", F_VEH, lambda a: a.update(sp=_sp(2, NAN))), ("sp.aero", F_VEH, lambda a: a.update(sp=_sp(4, 1e-3))),
    ("sp.fin", F_VEH, lambda a: a.update(sp=_sp(5, 1e-3))),
    ("nsigma=-1", F_MARG, lambda a: a.update(nsigma=-1.0)), ("nsigma=NaN", F_MARG, lambda a: a.update(nsigma=NAN)),
    ("cap=0", F_MARG, lambda a: a.update(cap=0.0)), ("cap=0.5", F_MARG, lambda a: a.update(cap=0.5)), ("cap=NaN", F_MARG, lambda a: a.update(cap=NAN)),
    ("which=0", F_WHICH, lambda a: a.update(which=0)), ("which=64", F_WHICH, lambda a: a.update(which=64)),
)
# two faults at once, one from each of two groups of checks (null buffers, nsigma / cap / which, w, the navigation model, the vehicle, the
# tracking weights) and a few within a group; whichever check comes first in a form decides the line
PAIRS = (("S0=NULL", "N0=NULL"), ("S0=NULL", "w<0"), ("N0=NULL", "m=15"), ("S0=NULL", "sp6=NULL"), ("N0=NULL", "q=NULL"), ("S0=NULL", "nsigma=-1"),
         ("N0=NULL", "cap=0"), ("w<0", "m=15"), ("w=NaN", "sp=NaN"), ("w=NaN", "q=NULL"), ("w<0", "which=0"), ("cap=NaN", "w=NaN"),
         ("m=15", "H=NULL"), ("rm=NULL", "H=NaN"), ("rm=0", "sp<0"), ("m=-1", "r=0"), ("H=NaN", "which=64"), ("nsigma=NaN", "m=15"),
         ("sp<0", "q=NULL"), ("sp.fin", "qf=NaN"), ("sp6=NULL", "r=NULL"), ("sp.aero", "sp.fin"), ("cap=0.5", "sp=NaN"), ("which=0", "sp6=NULL"),
         ("nsigma=-1", "cap=0"), ("cap=0", "which=0"), ("nsigma=NaN", "q<0"), ("which=64", "r=0"), ("q=NULL", "r=0"))


def refusal_lines(L, ctx, batch, fresh):
    """the lines of every case: `batch` initialised, `fresh` never; ends with the valid calls, the only ones that enqueue anything"""
    faults = {name: (need, make) for name, need, make in FAULTS}
    lines, valid = [], []
    for entry, base in FORMS:
        for m in (0, 2) if base & F_NAV else (0,):
            traits = base | (F_M if m else 0)
            applies = lambda name: faults[name][0] & traits == faults[name][0]   # noqa: E731
            cases = [(n,) for n, _, _ in FAULTS if applies(n)] + [p for p in PAIRS if applies(p[0]) and applies(p[1])]
            for case in cases + [("uninitialised",)]:
                a = _args(m)
                for name in case:
                    if name in faults:
                        faults[name][1](a)
                rc = _call(L, fresh if case == ("uninitialised",) else batch, entry, traits, a)
                lines.append("cov-refusal %s m=%d/%s %d %s" % (entry, m, "+".join(case), rc, L.scvx_last_error(ctx).decode()))
                assert all(np.all(a[k] == 7.0) for k in OUTPUTS), lines[-1]
            valid.append("cov-refusal %s m=%d/valid %d -" % (entry, m, _call(L, batch, entry, traits, _args(m))))
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
    with open(os.path.join(GOLDEN, "cov_batch_refusals.txt")) as f:
        want = f.read().splitlines()
    assert len(want) > 400 and all(line.startswith("cov-refusal scvx_batch_") for line in want)
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
    assert all(line.endswith(" 0 -") for line in got if "/valid " in line) and sum("/valid " in line for line in got) == 13
    assert all(int(line.split()[3]) != 0 for line in got if "/valid " not in line)
