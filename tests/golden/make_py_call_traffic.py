"""Writes tests/golden/py_call_traffic.txt: the C traffic of the Python binding of the analysis and dispersion calls, and its refusals.

    python tests/golden/make_py_call_traffic.py

`traffic_lines()` drives dynamics.py and batch.py over tests/py_call_recorder.py's stand-in library -- no shared library, no device --
at B = 2, K = 3, S = 5 -- every case at NU = 3 without an aerodynamic model, every entry point again at NU = 5 with one, and the calls with
vehicle=, whose refusals depend on the model, at the two mixed configurations -- and returns the recorded lines;
tests/test_py_call_traffic_cpu.py regenerates them and compares byte for byte.  Every input is a dyadic arithmetic pattern and the host
draws (montecarlo.mc_draws, mc_nav_draws, mc_vehicle_draws) are replaced by such patterns for the run, so nothing depends on the numpy
or LAPACK build: S0 is diagonal with dyadic standard deviations, w a power of four, the gains and tiles dyadic.

The refusal section pins every ValueError of these functions: one line per single fault and, for every pair of faults that one call can
hold, which of the two wins (one line per fault, _refusals) -- all with a stand-in that fails if the library is reached.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [p for p in (os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))) if p not in sys.path]

from py_call_recorder import Recorder, Unreachable, make_cache, pattern  # noqa: E402

B, K, S = 2, 3, 5
OUT = os.path.join(HERE, "py_call_traffic.txt")


def _draws(n, *shape):
    return lambda samples, seed, lo: pattern((samples,) + shape, 2 * n + 1) + (seed + 3 * lo) / 8.0


def _patch_draws():
    """the three host generators as arithmetic patterns that still depend on (samples, K, m, seed, noise, lo); returns the originals"""
    from successiveconvexification_amd import montecarlo as mc
    saved = mc.mc_draws, mc.mc_nav_draws, mc.mc_vehicle_draws
    mc.mc_draws = lambda samples, K, seed, noise=False, lo=0: (
        _draws(1, 14)(samples, seed, lo), _draws(2, K, 14)(samples, seed, lo) if noise else None)
    mc.mc_nav_draws = lambda samples, K, m, seed, lo=0: (
        _draws(3, 14)(samples, seed, lo), _draws(4, K, m)(samples, seed, lo) if m else None)
    mc.mc_vehicle_draws = lambda samples, seed, lo=0: _draws(5, 6)(samples, seed, lo)
    return saved


def _inputs(nu, aero):
    """the named inputs of one configuration"""
    n = 14 + nu
    sd = 2.0 ** -(np.arange(14) % 4 + 1.0)
    nd = 2.0 ** -(np.arange(14) % 3 + 2.0)
    v = dict(x=pattern((B, K + 1, 14), 3), u=pattern((B, K + 1, nu), 5), sigma=pattern((B,), 7), gain=pattern((B, K, nu, n), 9) - 0.5,
             deriv=pattern((B, K, 15 + 2 * nu, 14), 11) - 0.5,
             S0=(sd, np.diag(sd * sd), np.stack([np.diag(sd * sd), 4.0 * np.diag(sd * sd)])),
             N0=(nd, np.diag(nd * nd), np.stack([np.diag(nd * nd), 0.25 * np.diag(nd * nd)])),
             w=(None, 0.25, 4.0 ** -(np.arange(14) % 3 + 1.0)), H=np.eye(14)[1:4], rm=(0.25, np.array([0.25, 0.0625, 1.0])),
             vtile=pattern((B, K, 2, 14), 13), kf=pattern((B, K, 14, 3), 15) - 0.25,
             draws=(pattern((S, 14), 17), pattern((S, K, 14), 19)), ndraws=(pattern((S, 14), 21), pattern((S, K, 3), 23)),
             zeta=pattern((S, 6), 25) - 0.5)
    sp = np.array([2.0 ** -6, 2.0 ** -7, 0.0, 0.0, 0.0, 2.0 ** -8 if nu == 5 else 0.0])
    spt = sp.copy()
    spt[3] = 2.0 ** -9
    if aero:
        spt[4] = 2.0 ** -5
    v["veh"] = (np.zeros(6), sp)                    # needs no tiles
    v["veht"] = (np.zeros(6), spt)                  # ISP (and AERO with an aerodynamic model): needs vtile
    v["vehm"] = (pattern((6,), 27) - 0.5, spt)      # a mean shift: the sampled calls only
    return v


def _context_calls(c, v, level):
    """level "full": every case; "lean": the analyses, and of the sampled matrix one call per entry point and the calls with vehicle=;
    "vehicle": only the analyses with vehicle=, where the model (fins, aerodynamics) decides what is refused"""
    from successiveconvexification_amd import dynamics as dy
    x, u, sg, gain, deriv = v["x"], v["u"], v["sigma"], v["gain"], v["deriv"]
    S0, N0, w, H, rm = v["S0"], v["N0"], v["w"], v["H"], v["rm"]
    for i, dense in enumerate((False, True, "sig", ("covK",), ["cov"], ("sig", "cov")) if level != "vehicle" else ()):
        dy.cov_propagate_batch(c, x, u, deriv, gain, S0[i % 3], w[i % 3], dense=dense)
    dy.cov_propagate_batch(c, x, u, deriv, gain, S0[0], w[1], dense=("sens", "sig"), vehicle=v["veh"])
    dy.cov_propagate_batch(c, x, u, deriv, gain, S0[1], dense=True, vehicle=v["veht"], vtile=v["vtile"])
    dy.cov_propagate_batch(c, x, u, deriv, gain, S0[2], w[2], dense="sens", vehicle=v["veh"], vtile=v["vtile"])
    for i, dense in enumerate((False, True, "mean", "sig", "covK", "cov", "satk") if level != "vehicle" else ()):
        dy.cov_propagate_batch(c, x, u, deriv, gain, S0[i % 3], w[i % 3], dense=dense, clamp=True, band=(0.5, np.inf) if i % 2 else None)
    if level != "vehicle":
        dy.cov_propagate_batch(c, x, u, deriv, gain, S0[1], w[1], clamp=True, band=(0.25, 1.5))
        dy.cov_path_sigma_batch(c, x, u, deriv, gain, S0[0])
    dy.cov_path_sigma_batch(c, x, u, deriv, gain, S0[1], w[2], vehicle=v["veh"])
    dy.cov_path_sigma_batch(c, x, u, deriv, gain, S0[2], w[1], vehicle=v["veht"], vtile=v["vtile"], dense=("sens",))
    for i, dense in enumerate((False, True, "sig", "navsig", "kf", "joint") if level != "vehicle" else ()):
        dy.nav_cov_batch(c, x, u, deriv, gain, S0[i % 3], N0[(i + 1) % 3], H if i else None, rm[i % 2] if i else None, w[i % 3], dense=dense)
    dy.nav_cov_batch(c, x, u, deriv, gain, S0[0], N0[0], H, rm[1], dense=("sens", "kf"), vehicle=v["veh"])
    dy.nav_cov_batch(c, x, u, deriv, gain, S0[1], N0[2], None, None, w[1], dense=True, vehicle=v["veht"], vtile=v["vtile"])
    if level != "vehicle":
        dy.nav_path_sigma_batch(c, x, u, deriv, gain, S0[0], N0[1], None, None)
        dy.nav_path_sigma_batch(c, x, u, deriv, gain, S0[2], N0[0], H, rm[0], w[2])
    dy.nav_path_sigma_batch(c, x, u, deriv, gain, S0[1], N0[1], H, rm[1], w[1], vehicle=v["veh"], dense="sens")
    dy.nav_path_sigma_batch(c, x, u, deriv, gain, S0[1], N0[1], H, rm[1], vehicle=v["veht"], vtile=v["vtile"])
    dy.vehicle_sensitivity_batch(c, x, u, sg, gain, h=2.0 ** -8, nsub=3, clamp=True)
    if level == "vehicle":
        return
    dy.mc_draws_device_batch(c, S, seed=11, sample_lo=2, plan_lo=1, plans=B)
    full = level == "full"

    def fly(nav, direct, *a, **kw):
        if nav is not None and kw.get("draws") is not None:
            kw["draws"] = kw["draws"] + (v["ndraws"] if nav[1] is not None else (v["ndraws"][0], None))
        if direct:   # with the filter gains passed in: kf=None is what the calls through track_mc_batch(nav=) make
            return dy.track_mc_nav_batch(c, x, u, sg, deriv, gain, a[0], nav[0], nav[1], nav[2], *a[1:], kf=v["kf"], **kw)
        return dy.track_mc_batch(c, x, u, sg, gain, *a, nav=nav, **kw)
    _sampled(lambda *a, **kw: fly(None, False, *a, **kw), v, False, 2 * full)
    # through track_mc_batch(nav=): the plan is linearised and, with a measurement, the filter gains are computed first
    if full:
        _sampled(lambda *a, **kw: fly((N0[1], None, None), False, *a, **kw), v, True, 0)
    _sampled(lambda *a, **kw: fly((N0[0], H, rm[0]), False, *a, **kw), v, True, 0)
    _sampled(lambda *a, **kw: fly((N0[2], H, rm[1]), True, *a, **kw), v, True, 1 if full else 0)
    dy.track_mc_nav_batch(c, x, u, sg, deriv, gain, S0[0], N0[0], H, rm[0], S, kf=v["kf"], dense="navK")
    dy.track_mc_nav_batch(c, x, u, sg, deriv, gain, S0[1], N0[1], H, rm[1], S, seed=4, w=w[2], kf=v["kf"], quantiles=(0.5,), vehicle=v["vehm"])
    dy.track_mc_nav_batch(c, x, u, sg, deriv, gain, S0[2], N0[2], None, None, S, rng="device")


def _sampled(fly, v, nav, depth):
    """the matrix of one sampled call: fly(S0, samples, **keywords).  depth 0: one call per entry point; 1: and the forms of vehicle=;
    2: every case"""
    S0, w = v["S0"], v["w"]
    names = ("flights", "xland", "dx0") + (("navfed", "navK") if nav else ())
    fly(S0[0], S)
    fly(S0[1], S, w=w[1], quantiles=(0.5, 0.9))
    fly(S0[0], S, seed=7, rng="device")
    fly(S0[1], S, seed=9, w=w[1], vehicle=v["vehm"], dense=("theta", "xland"), sample_lo=3)
    if depth == 0:
        return
    fly(S0[2], S, vehicle=v["vehm"] + (v["zeta"],), dense="theta", quantiles=(0.5,))
    fly(S0[0], S, seed=13, w=w[2], vehicle=v["vehm"], rng="device", independent=True, plan_lo=2, dense=("theta", "pathv"))
    if depth == 1:
        return
    fly(S0[0], S, seed=9, vehicle=v["veh"])
    fly(S0[2], S, vehicle=v["veh"] + (None,), draws=v["draws"], dense=True)
    fly(S0[0], S, seed=13, vehicle=v["veh"], rng="device", quantiles=(0.5,), per_node=True)
    _sampled_plain(fly, v, names)


def _sampled_plain(fly, v, names):
    S0, w = v["S0"], v["w"]
    fly(S0[1], S, seed=3, w=w[1], nsub=2, clamp=True, tol=0.125, dense=True)
    fly(S0[2], S, seed=5, w=w[2], nsub=None, dense=names[:2], sample_lo=2)
    for i, name in enumerate(names):
        fly(S0[i % 3], S, dense=name if i % 2 else (name,))
    fly(S0[0], 99, seed=99, draws=v["draws"], dense=("dx0",))
    fly(S0[0], S, draws=(v["draws"][0], None))
    fly(S0[1], S, quantiles=0.75, per_node=True, dense=True)
    fly(S0[2], S, dense="pathv")
    fly(S0[2], S, w=w[2], quantiles=[0.0, 1.0], per_node=True, dense=("pathv", "xland"), draws=v["draws"])
    fly(S0[0], S, seed=-7, w=w[1], rng="device", independent=True, sample_lo=4, plan_lo=6, dense=("flights",))
    fly(S0[1], S, seed=2 ** 64 + 5, w=w[2], rng="device", quantiles=(0.25,), per_node=True, dense=("pathv",))


def _batch_calls(c, v, level):
    from successiveconvexification_amd.batch import ScvxBatch
    S0, N0, w, H, rm = v["S0"], v["N0"], v["w"], v["H"], v["rm"]
    b = ScvxBatch(c, B)
    nu = c.nu
    wt = (dict(), dict(q=0.5, r=2.0, qf=8.0), dict(q=pattern((14,), 3), r=pattern((nu,), 5), qf=pattern((14,), 7)))
    plain, full = level != "vehicle", level == "full"
    for i, dense in enumerate((False, True, "sig", ("covK",), ["cov"]) if plain else ()):
        b.covariance(S0[i % 3], w[i % 3], dense=dense, **wt[i % 3])
    b.covariance(S0[0], w[1], dense=True, vehicle=v["veh"])
    b.covariance(S0[1], vehicle=v["veht"], **wt[1])
    for i, dense in enumerate((False, True, "mean", "sig", "covK", "cov", "satk") if plain else ()):
        b.covariance(S0[i % 3], w[i % 3], dense=dense, clamp=True, band=(0.5, np.inf) if i % 2 else None, **wt[i % 3])
    for i, dense in enumerate((False, True, "sig", "navsig", "kf", "joint") if plain else ()):
        b.navigation(S0[i % 3], N0[(i + 1) % 3], H if i else None, rm[i % 2] if i else None, w[i % 3], dense=dense, **wt[i % 3])
    b.navigation(S0[0], N0[0], H, rm[1], dense=("kf",), vehicle=v["veh"])
    b.navigation(S0[1], N0[2], None, None, w[1], dense=True, vehicle=v["veht"], **wt[2])
    b.margins_from_cov(S0[1], ("mass", "tilt"), 2.0, 0.125, w[1], vehicle=v["veh"], **wt[1])
    b.margins_from_cov(S0[2], ("thrust",), w=w[2], vehicle=v["veht"])
    b.margins_from_nav(S0[2], N0[2], H, rm[0], w=w[2], vehicle=v["veht"])
    if not plain:
        return
    for nav in (None, (N0[1], None, None), (N0[0], H, rm[0])):
        if not full and nav is not None and nav[1] is None:
            continue

        def fly(*a, **kw):
            if nav is not None and kw.get("draws") is not None:
                kw["draws"] = kw["draws"] + (v["ndraws"] if nav[1] is not None else (v["ndraws"][0], None))
            return b.track_mc(a[0], samples=a[1], nav=nav, **kw)
        _sampled(fly, v, nav is not None, (0, 1, 2)[(nav is None) + 2 * (nav is not None and nav[1] is not None)] if full else 0)
        b.track_mc(S0[0], nav=nav, samples=S, **wt[2])
        b.margins_from_mc(S0[1], p=0.75, samples=S, constraints=("thrust", "mass", "rate"), seed=3, w=w[1], clamp=True, nav=nav)
        b.path_sigma(S0[0], nav=nav, vehicle=v["veht"], **wt[1])
        if full:
            b.margins_from_mc(S0[0], samples=S, constraints=("rate",), nav=nav, vehicle=v["vehm"], rng="device", independent=True, **wt[1])
            b.path_sigma(S0[2], w[2], nav=nav)
    b.margins_from_cov(S0[0])
    b.margins_from_nav(S0[0], N0[0], None, None)
    b.margins_from_nav(S0[1], N0[1], H, rm[1], ("glide", "rate"), 2.0, 0.125, w[1], **wt[2])
    b.robustify(S0[0])
    b.robustify(S0[1], 2.0, 1, 0.125, w[1], vehicle=v["veh"], **wt[1])
    b.robustify(S0[2], constraints="all", w=w[2])
    b.robustify(S0[0], nav=(N0[0], H, rm[0]))
    if full:
        b.robustify(S0[0], constraints=("thrust", "mass"), vehicle=v["veht"])
        b.robustify(S0[1], nav=(N0[1], None, None), constraints=("tilt",), w=w[1], vehicle=v["veh"])
        b.robustify(S0[0], mc=dict(p=0.75, samples=S, seed=2))
    b.robustify(S0[1], mc=dict(samples=S, rng="device", independent=True, sample_lo=1, plan_lo=2, vehicle=v["vehm"], clamp=True),
                nav=(N0[0], H, rm[1]), constraints=("thrust", "mass", "rate"), w=w[2], **wt[1])


PAIRS = True


def _refusals(tag, fn, base, faults):
    """One line per fault with what it raises.  With PAIRS also one line per fault a with, for every later fault b that fits into one
    call with it (no keyword given two different values), which of the two refusals the call raises: `>b` a's, `<b` b's, `=b` the two
    are one message, `!b{c}` the refusal of a third fault c (one the pair brings about), `!b{...}` anything else, spelled out.  Without
    PAIRS only the faults of vehicle=, whose refusals depend on the model, are run."""
    def outcome(combo):
        kw, given = dict(base), {}
        for n in combo:
            for k, val in faults[n].items():
                given.setdefault(k, []).append(val)
                kw[k] = val
        if any(a is not vals[0] for vals in given.values() for a in vals):
            return None
        try:
            fn(**kw)
            return "no refusal"
        except ValueError as e:
            return "ValueError: %s" % e
        except AssertionError as e:
            return "AssertionError: %s" % e
    names = [n for n in faults if PAIRS or n.startswith(("veh", "sens", "vtile"))]
    single = {n: outcome((n,)) for n in names}
    third = {msg: n for n, msg in reversed(list(single.items()))}
    lines = ["refusal %s [%s] -> %s" % (tag, n, single[n]) for n in names]
    for i, a in enumerate(names if PAIRS else ()):
        row = []
        for b in names[i + 1:]:
            got = outcome((a, b))
            if got is not None:
                row.append(("=" if got == single[a] == single[b] else ">" if got == single[a] else "<" if got == single[b] else "!") + b
                           + ("{%s}" % third.get(got, got) if got not in (single[a], single[b]) else ""))
        if row:
            lines.append("pairs %s [%s] %s" % (tag, a, " ".join(row)))
    return lines


def _refusal_lines(nu, aero):
    from successiveconvexification_amd import dynamics as dy
    from successiveconvexification_amd.batch import ScvxBatch
    c = make_cache(Unreachable(), nu, aero)
    v = _inputs(nu, aero)
    b = ScvxBatch.__new__(ScvxBatch)
    b.cache, b.B, b.K, b.nu, b._L, b.handle = c, B, K, nu, c._L, None
    T, bad14 = True, np.zeros(13)
    mu1 = np.zeros(6)
    mu1[0] = 1.0
    sp = v["veh"][1]
    spn, spf, spa = sp.copy(), sp.copy(), sp.copy()
    spn[1], spf[5], spa[4] = -1.0, 0.5, 0.5
    plan = dict(x=dict(x=v["x"][:, :, :13]), x2=dict(x=v["x"][0]), u=dict(u=v["u"][:, :-1]), gain=dict(gain=v["gain"][:, :-1]),
                deriv=dict(deriv=v["deriv"][..., :13]))
    plans = dict(plan, sigma=dict(sigma=v["sigma"][:1]))
    del plans["deriv"]
    cov_in = dict(S0=dict(S0=bad14), w=dict(w=bad14), w2=dict(w=np.zeros((14, 1))))
    weights = dict(q=dict(q=bad14), r=dict(r=np.zeros(nu + 1)), qf=dict(qf=np.zeros((14, 14))))
    fveh = dict(veh_len=dict(vehicle=(mu1,)), veh_shape=dict(vehicle=(np.zeros(5), sp)), veh_mu=dict(vehicle=(mu1, sp)),
                veh_neg=dict(vehicle=(np.zeros(6), spn)), veh_fin=dict(vehicle=(np.zeros(6), spf)), veh_aero=dict(vehicle=(np.zeros(6), spa)),
                veh_tile=dict(vehicle=v["veht"]))
    fvt = dict(fveh, sens=dict(dense=("sens",)), vtile=dict(vtile=v["vtile"]), vtile_shape=dict(vehicle=v["veht"], vtile=v["vtile"][:, :, :1]))
    model = dict(H=dict(H=np.eye(13)), rm_none=dict(rm=None), rm_shape=dict(rm=np.ones(2)))
    N0b = dict(N0=dict(N0=bad14))
    navs = dict(nav_len=dict(nav=(v["N0"][0], v["H"])), nav_none=dict(nav=(None, v["H"], 0.25)), nav_n0=dict(nav=(bad14, v["H"], 0.25)),
                nav_h=dict(nav=(v["N0"][0], np.eye(13), 0.25)), nav_rows=dict(nav=(v["N0"][0], np.ones((15, 14)), 0.25)),
                nav_rm=dict(nav=(v["N0"][0], v["H"], 0.0)), nav_inf=dict(nav=(v["N0"][0], np.where(v["H"] != 0.0, np.inf, 0.0), 0.25)))
    smp = dict(rng=dict(rng="gpu"), indep=dict(independent=T), dev_draws=dict(rng="device", draws=v["draws"]),
               lo=dict(rng="device", sample_lo=-1), theta=dict(dense=("theta",)), sv_len=dict(vehicle=(mu1,)),
               sv_shape=dict(vehicle=(mu1, np.zeros(5))), nq=dict(quantiles=np.linspace(0.0, 1.0, 17)), per_node=dict(per_node=T),
               prob=dict(quantiles=(1.5,)), samples=dict(samples=0), dev_samples=dict(rng="device", samples=0),
               dense=dict(dense=("bogus",)), zeta_dev=dict(rng="device", vehicle=v["vehm"] + (v["zeta"],)),
               zeta_shape=dict(vehicle=v["vehm"] + (v["zeta"][:4],)), **cov_in)
    out = []
    base = dict(cache=c, x=v["x"], u=v["u"], deriv=v["deriv"], gain=v["gain"], S0=v["S0"][0])
    out += _refusals("cov_propagate_batch", dy.cov_propagate_batch, base, dict(
        plan, **cov_in, **fvt, clamp_veh=dict(clamp=T, vehicle=v["veh"]), clamp_vtile=dict(clamp=T, vtile=v["vtile"]), band=dict(band=(0.5, 1.0)),
        band_bad=dict(clamp=T, band=(2.0, 1.0)), clamp_dense=dict(clamp=T, dense="sens"), dense=dict(dense="bogus")))
    out += _refusals("cov_path_sigma_batch", dy.cov_path_sigma_batch, base, dict(plan, **cov_in, **fvt, dense=dict(dense=("sig",))))
    nbase = dict(base, N0=v["N0"][0], H=v["H"], rm=0.25)
    out += _refusals("nav_cov_batch", dy.nav_cov_batch, nbase, dict(plan, **cov_in, **N0b, **model, **fvt, dense=dict(dense="cov")))
    out += _refusals("nav_path_sigma_batch", dy.nav_path_sigma_batch, nbase, dict(plan, **cov_in, **N0b, **model, **fvt, dense=dict(dense=("sig",))))
    sbase = dict(cache=c, x=v["x"], u=v["u"], sigma=v["sigma"], gain=v["gain"], S0=v["S0"][0], samples=S)
    out += _refusals("track_mc_batch", dy.track_mc_batch, sbase, dict(plans, **smp, **navs, draws=dict(draws=(v["draws"][0][:, :13], None)),
                                                                    draws_eta=dict(draws=(v["draws"][0], v["draws"][1][:, :2]))))
    snbase = dict(sbase, deriv=v["deriv"], N0=v["N0"][0], H=v["H"], rm=0.25, kf=v["kf"])
    out += _refusals("track_mc_nav_batch", dy.track_mc_nav_batch, snbase, dict(
        plans, deriv=plan["deriv"], **smp, **N0b, **model, kf=dict(kf=v["kf"][:, :, :13]), draws_len=dict(draws=v["draws"]),
        draws_nud=dict(draws=v["draws"] + (v["ndraws"][0], None))))
    out += _refusals("ScvxBatch.covariance", b.covariance, dict(S0=v["S0"][0]), dict(
        weights, **cov_in, **fveh, clamp_veh=dict(clamp=T, vehicle=v["veh"]), band=dict(band=(0.5, 1.0)), band_bad=dict(clamp=T, band=(2.0, 1.0)),
        clamp_dense=dict(clamp=T, dense="sens"), dense=dict(dense="bogus")))
    out += _refusals("ScvxBatch.navigation", b.navigation, dict(S0=v["S0"][0], N0=v["N0"][0], H=v["H"], rm=0.25), dict(
        weights, **cov_in, **N0b, **model, **fveh, clamp=dict(clamp=T), dense=dict(dense="cov")))
    out += _refusals("ScvxBatch.track_mc", b.track_mc, dict(S0=v["S0"][0], samples=S), dict(
        weights, **smp, **navs, draws=dict(draws=(v["draws"][0][:, :13], None)), draws_len=dict(nav=(v["N0"][0], v["H"], 0.25), draws=v["draws"])))
    con = dict(con_empty=dict(constraints=()), con_name=dict(constraints=("thrust", "gimbal")), con_str=dict(constraints="thrust"))
    out += _refusals("ScvxBatch.margins_from_cov", b.margins_from_cov, dict(S0=v["S0"][0]), dict(weights, **cov_in, **fveh, **con))
    out += _refusals("ScvxBatch.margins_from_nav", b.margins_from_nav, dict(S0=v["S0"][0], N0=v["N0"][0], H=v["H"], rm=0.25), dict(
        weights, **cov_in, **fveh, **con, N0_none=dict(N0=None), **N0b, **model, rm_zero=dict(rm=0.0), rows=dict(H=np.ones((15, 14)))))
    out += _refusals("ScvxBatch.margins_from_mc", b.margins_from_mc, dict(S0=v["S0"][0], samples=S), dict(
        con, rng=smp["rng"], indep=smp["indep"], nav_len=navs["nav_len"], samples=smp["samples"], S0=cov_in["S0"], q=weights["q"]))
    out += _refusals("ScvxBatch.path_sigma", b.path_sigma, dict(S0=v["S0"][0]), dict(nav_len=navs["nav_len"], nav_rm=navs["nav_rm"]))
    out += _refusals("ScvxBatch.robustify", b.robustify, dict(S0=v["S0"][0]), dict(
        con, rounds=dict(rounds=0), veh_mc=dict(vehicle=v["veh"], mc=dict(samples=S)), **fveh, mc_type=dict(mc=(S,)), mc_key=dict(mc=dict(nsigma=3.0)),
        nav_len=navs["nav_len"], nav_rm=navs["nav_rm"], mc_nav=dict(mc=dict(samples=S), nav=(None, None, None))))
    return out


def traffic_lines():
    global PAIRS
    from successiveconvexification_amd import montecarlo as mc
    saved = _patch_draws()
    lines = []
    try:
        for nu, aero, level in ((3, False, "full"), (5, True, "lean"), (3, True, "vehicle"), (5, False, "vehicle")):
            rec = Recorder()
            c = make_cache(rec, nu, aero)
            v = _inputs(nu, aero)
            _context_calls(c, v, level)
            _batch_calls(c, v, level)
            lines.append("# NU = %d, %s: %d calls" % (nu, "aerodynamic" if aero else "exo-atmospheric", len(rec.lines)))
            lines += rec.lines
        for nu, aero in ((3, False), (5, True)):
            lines.append("# refusals, NU = %d, %s" % (nu, "aerodynamic" if aero else "exo-atmospheric"))
            lines += _refusal_lines(nu, aero)
            PAIRS = False
    finally:
        PAIRS = True
        mc.mc_draws, mc.mc_nav_draws, mc.mc_vehicle_draws = saved
    return lines


if __name__ == "__main__":
    lines = traffic_lines()
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%s: %d lines" % (OUT, len(lines)))
