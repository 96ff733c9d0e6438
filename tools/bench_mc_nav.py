"""Cost of the sampled closed-loop dispersion flown on a navigation estimate (scvx_track_mc_nav_f64) next to the call it extends and
next to the sampled check it replaces.

    python tools/bench_mc_nav.py [--nsub 10] [--launches 20] [--repeats 5] [--json out.json]
    python tools/bench_mc_nav.py [--from-json out.json] [--parent-log LOG --log LOG] --md profiles/mc_nav.md     (no device needed)

For the flyable problem (mdry = 0.55, tf_guess = 8) on the exo and the aero + fins model, K = 50: 128 dispersed plans are stepped
`--plan-steps` times to get physical plans, their tiles and their gains, and the navigation analysis gives the filter gains (position
and velocity measured, m = 6).  Then, in the same process, B S = 8192 flights at B = 128, S = 64 and at B = 8, S = 1024, at m = 0 and
m = 6, with process noise:
  * scvx_track_mc_nav_f64 and scvx_track_mc_f64 (device pointers, no dense output) in alternating windows: the ratio of the two;
  * scvx_track_fly_nav_f64 at B = 8192 on the REPLICATED plans with a host-made nav [8192][K][14] (the errors the new call formed),
    again in alternating windows with the new call (without noise: that flyer has none).
HIP events, `--repeats` windows of `--launches` launches after a warm-up, median (min .. max) of the windows.  --parent-log / --log:
the outputs of `python -m successiveconvexification_amd.build --force -v` on the parent commit and on this one, for the resource
tables; without --from-json and without a device only those tables are written."""
import argparse
import ctypes as C
import json
import os
import re
import sys
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_mc import FIELDS, FLYABLE, SHAPES, resources   # noqa: E402


def demangled(name):
    """fly_kernel<true, false, ...> from the mangled name of one of the flight kernels"""
    m = re.match(r"_ZN4scvx\d+(fly_kernel|mc_fly_kernel|mc_nav_fly_kernel)I((?:Lb[01]E)+)([df])?(J(?:PKd)?E)?", name)
    if not m:
        return "mc_nav_finish_kernel" if "mc_nav_finish" in name else "mc_finish_kernel" if "mc_finish" in name else name
    args = ["true" if b == "1" else "false" for b in re.findall(r"Lb([01])E", m.group(2))]
    if m.group(3):
        args.append("double" if m.group(3) == "d" else "float")
    if m.group(4) and "PKd" in m.group(4):
        args.append("double const*")
    return "%s<%s>" % (m.group(1), ", ".join(args))


def resource_section(parent_log, log):
    par, new = resources(parent_log), resources(log)
    same = [n for n in par if par[n] == new.get(n)]
    lines = ["## Resources: parent against this change\n",
             "`python -m successiveconvexification_amd.build --force -v` (`-Rpass-analysis=kernel-resource-usage`, gfx950) on the parent "
             "commit and on this one.  The parent reports %d kernels; %d of them report the same figures here (every field below), %d "
             "differ, %d are new.  The new kernels are in a translation unit of their own (`csrc/scvx_mc_nav.hip`); `csrc/scvx_mc.hip` "
             "lost only the declarations it now shares through `csrc/scvx_mc.hpp`, `csrc/scvx_flight.hip` is unchanged.  Below: every "
             "kernel of those three files.  mc_nav_fly_kernel (the last template argument is the tiles' storage type) keeps eps, A_k, Kf_k "
             "and H in 12 KB of LDS per block; it spills more SGPRs (into VGPR lanes) than mc_fly_kernel and, in some aerodynamic "
             "instantiations, 4 to 6 VGPRs (into AGPRs: the scratch size stays 0); of the two models that run at 2 waves / SIMD in "
             "mc_fly_kernel the exo one still does, the exo + fins one runs at 1.\n"
             % (len(par), len(same), len(par) - len(same), len([n for n in new if n not in par])),
             "| kernel | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR spills | waves/SIMD | LDS B/block | parent |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    rows = [n for n in new if "fly_kernel" in n or "mc_finish" in n or "mc_nav_finish" in n]
    for n in sorted(rows, key=lambda n: ("mc_nav" in n, "mc_" in n, n)):
        tag = "new" if n not in par else ("the same" if par[n] == new[n] else "WAS " + " ".join(par[n].get(f, "?") for f in FIELDS))
        lines.append("| %s | %s | %s |" % (demangled(n), " | ".join(new[n].get(f, "?") for f in FIELDS), tag))
    return "\n".join(lines) + "\n"


def measure(a):
    import torch
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.defns import AtmosphericData
    from successiveconvexification_amd.dynamics import IntegratorCache
    z = np.load(os.path.join(ROOT, "tests", "golden", "lift_drag_tables.npz"))
    aero = AtmosphericData(z["drag"], z["lift"], z["torque"])
    models = {"exo": lambda: replace(sp.base_prob_scaled, **FLYABLE), "aero+fins": lambda: replace(sp.base_prob_fin_scaled(aero), **FLYABLE)}
    ts = torch.cuda.Stream()   # torch's events see kernels on a torch stream: the context runs on one for this tool
    res = {"nsub": a.nsub, "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "models": {}}

    def timed_ab(call_a, call_b):
        """[median, min, max] ms per launch of two calls in alternating windows: what a ratio of the two is taken from"""
        for call in (call_a, call_b):
            for _ in range(a.warmup):
                assert call() == 0
        w = ([], [])
        for _ in range(a.repeats):
            for i, call in enumerate((call_a, call_b)):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(ts)
                for _ in range(a.launches):
                    call()
                t1.record(ts)
                torch.cuda.synchronize()
                w[i].append(t0.elapsed_time(t1) / a.launches)
        return [[float(np.median(v)), float(min(v)), float(max(v))] for v in w]

    vp = lambda t: None if t is None else C.c_void_p(t.data_ptr())   # noqa: E731
    dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    dev = lambda v: torch.tensor(np.ascontiguousarray(v), device="cuda")   # noqa: E731
    f64 = dict(dtype=torch.float64, device="cuda")
    for name in a.models.split(","):
        p = models[name]()
        K = p.K
        c = IntegratorCache(p, npts=10)
        c.set_stream(ts.cuda_stream)
        PB = SHAPES[0][0]
        b = ScvxBatch(c, PB).init(mc.disperse_ics(p, 0, PB, a.seed))
        for _ in range(a.plan_steps):
            b.solve_step_async()
        x, u, s = b.trajectory()
        gain = b.track_gains()
        deriv = b.linearization()[1]
        L, h, nu = c._L, c.handle, c.nu
        n = 14 + nu
        sd = np.zeros(14)
        sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
        sd[7:] = 1e-3
        w = np.full(14, 1e-10)
        H6 = mc.measurement_rows("rv")
        rm6 = np.repeat([(3e-5 * np.abs(x[0, 0, 1:4]).max()) ** 2, (3e-5 * np.abs(x[0, 0, 4:7]).max()) ** 2], 3)
        kf6 = b.navigation(sd, 0.5 * sd, H6, rm6, w=w, dense=("kf",)).kf
        b.close()
        C0 = np.stack([mc.handover_factor(sd)] * PB)
        CN = 0.5 * C0
        sw = np.sqrt(w)
        out = {"shapes": {}}
        plan_doubles = (K + 1) * (14 + nu) + 1 + K * nu * n            # x, u, sigma and the gains of one plan
        nav_doubles = K * 196 + K * 14 * 6                              # the state blocks of its tiles and its filter gains (m = 6)
        for B, S in SHAPES:
            xi0, eta = mc.mc_draws(S, K, a.seed, noise=True)
            xin, nud6 = mc.mc_nav_draws(S, K, 6, a.seed)
            xd, ud, sg, gd, cd, xid, etd, dd, cnd, xnd = (dev(v) for v in (x[:B], u[:B], s[:B], gain[:B], C0[:B], xi0, eta, deriv[:B], CN[:B], xin))
            rep, xm, xc = torch.empty((B, _lib.MC_NREP), **f64), torch.empty((B, 14), **f64), torch.empty((B, 14, 14), **f64)
            jm, jc, nv = torch.empty((B, 28), **f64), torch.empty((B, 28, 28), **f64), torch.empty((B, 8), **f64)
            d0, fed = torch.empty((B, S, 14), **f64), torch.empty((B, S, K, 14), **f64)
            old = lambda e: L.scvx_track_mc_f64(h, B, K, S, vp(xd), vp(ud), vp(sg), vp(gd), vp(cd), vp(xid), e, dp(sw), None, a.nsub, 0,   # noqa: E731
                                                0.0, vp(rep), vp(xm), vp(xc), None, None, None)
            N = B * S
            rp = lambda t: t.repeat_interleave(S, dim=0).contiguous()   # noqa: E731
            xr, ur, sr, gr = rp(xd), rp(ud), rp(sg), rp(gd)
            frep = torch.empty((N, _lib.FLIGHT_NREP), **f64)
            o = {"plan_bytes": B * plan_doubles * 8, "nav_bytes": B * nav_doubles * 8, "replicated_bytes": N * plan_doubles * 8,
                 "replicated_nav_bytes": N * K * 14 * 8}
            for m, Hm, rmm, kfh, nudh in ((0, None, None, None, None), (6, H6, rm6, kf6[:B], nud6)):
                kfd = None if kfh is None else dev(kfh)
                ndd = None if nudh is None else dev(nudh)
                new = lambda e, d, f: L.scvx_track_mc_nav_f64(h, B, K, S, vp(xd), vp(ud), vp(sg), vp(gd), vp(cd), vp(xid), e, dp(w), vp(dd),   # noqa: E731
                                                              vp(kfd), vp(cnd), vp(xnd), vp(ndd), m, dp(Hm), dp(rmm), a.nsub, 0, 0.0, vp(rep),
                                                              vp(xm), vp(xc), vp(jm), vp(jc), vp(nv), None, None, d, f, None)
                q = {}
                q["nav_ms"], q["mc_ms"] = timed_ab(lambda: new(vp(etd), None, None), lambda: old(vp(etd)))
                q["ratio_mc"] = q["nav_ms"][0] / q["mc_ms"][0]
                assert new(None, vp(d0), vp(fed)) == 0          # without noise: the dx0 and the errors the flyer is fed
                torch.cuda.synchronize()
                q["finite_flights"] = int(B * S - rep[:, 44].sum().item())
                d0f, fedf = d0.reshape(N, 14), fed.reshape(N, K, 14)
                fly = lambda: L.scvx_track_fly_nav_f64(h, N, K, vp(xr), vp(ur), vp(sr), vp(gr), vp(d0f), vp(fedf), a.nsub, 0, vp(frep),   # noqa: E731
                                                       None, None)
                q["nav_quiet_ms"], q["fly_nav_ms"] = timed_ab(lambda: new(None, None, None), fly)
                q["ratio_fly"] = q["nav_quiet_ms"][0] / q["fly_nav_ms"][0]
                o["m%d" % m] = q
            out["shapes"]["%dx%d" % (B, S)] = o
            del xr, ur, sr, gr, frep, d0, fed
            torch.cuda.empty_cache()
        res["models"][name] = out
        c.set_stream(None)
        c.close()
    return res


def write_md(res, a):
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    with open(a.md, "w") as f:
        f.write("# Sampled closed-loop dispersion flown on a navigation estimate\n\n")
        if res is None:
            f.write("**No device time has been measured yet** (`python tools/bench_mc_nav.py --json out.json` on an MI355X, then "
                    "`--from-json out.json --md profiles/mc_nav.md`): this file holds only what the compiler reports.\n\n")
        else:
            f.write("Device time at B S = 8192 flights, K = 50, nsub = %d.  `python tools/bench_mc_nav.py`; %s; HIP events; per entry %d "
                    "windows of %d launches after %d warm-up launches, median (min .. max) of the windows in ms; fp64; flyable problem "
                    "(mdry = 0.55, tf_guess = 8), plans after 3 solve_steps, weights q = 1, r = 1, qf = 100, handover 1e-3, navigation "
                    "handover half of it, w = 1e-10; m = 6: position and velocity measured at every node.  `mc_nav`: "
                    "scvx_track_mc_nav_f64 without dense outputs; `mc`: scvx_track_mc_f64 on the same shape, both with process noise, in "
                    "alternating windows; `fly_nav`: scvx_track_fly_nav_f64 at B = 8192 on the replicated plans with the host-made nav "
                    "the new call formed, beside `mc_nav` without noise, in alternating windows.\n\n"
                    % (res["nsub"], res["device"], res["repeats"], res["launches"], res["warmup"]))
            f.write("| model | B x S | m | mc_nav | mc | mc_nav / mc | mc_nav, no noise | fly_nav, replicated | mc_nav / fly_nav |\n"
                    "|---|---|---|---|---|---|---|---|---|\n")
            for name, mdl in res["models"].items():
                for shp, o in mdl["shapes"].items():
                    for m in (0, 6):
                        q = o["m%d" % m]
                        f.write("| %s | %s | %d | %s | %s | %.3f | %s | %s | %.3f |\n"
                                % (name, shp.replace("x", " x "), m, fmt(q["nav_ms"]), fmt(q["mc_ms"]), q["ratio_mc"], fmt(q["nav_quiet_ms"]),
                                   fmt(q["fly_nav_ms"]), q["ratio_fly"]))
            f.write("\nThe device memory that holds the plans, their gains and what the estimate needs, in each form:\n\n"
                    "| model | B x S | plans + gains, shared | tiles' state blocks + filter gains (m = 6), shared | plans + gains, replicated | "
                    "nav [8192][K][14], host-made |\n|---|---|---|---|---|---|\n")
            for name, mdl in res["models"].items():
                for shp, o in mdl["shapes"].items():
                    f.write("| %s | %s | %.3f MB | %.3f MB | %.1f MB | %.1f MB |\n"
                            % (name, shp.replace("x", " x "), o["plan_bytes"] / 1e6, o["nav_bytes"] / 1e6, o["replicated_bytes"] / 1e6,
                               o["replicated_nav_bytes"] / 1e6))
            rs = [o["m%d" % m]["ratio_mc"] for mdl in res["models"].values() for o in mdl["shapes"].values() for m in (0, 6)]
            f.write("\nThe extra work per node is about 196 + 28 m fused multiply-adds beside roughly forty right-hand-side evaluations; "
                    "the expectation stated with the feature (not a bar) was a ratio to scvx_track_mc_f64 close to 1.  Measured: %.3f .. "
                    "%.3f.  Every flight of every run is finite (%s).\n\n"
                    % (min(rs), max(rs), all(o["m%d" % m]["finite_flights"] == 8192 for mdl in res["models"].values()
                                               for o in mdl["shapes"].values() for m in (0, 6))))
            ov = lambda m, key: [1e3 * (o["m%d" % m]["nav_ms"][0] - o["m%d" % m]["mc_ms"][0]) for o in res["models"][key]["shapes"].values()]   # noqa: E731
            keys = list(res["models"])
            f.write("The ratios are NOT close to 1, and the surprise is in the shape of the overhead: in microseconds per launch it is "
                    + "; ".join("%s %s at m = 0 and %s at m = 6" % (k, " / ".join("%.0f" % v for v in ov(0, k)), " / ".join("%.0f" % v for v in ov(6, k)))
                                for k in keys)
                    + " -- about the same on both models, so it weighs three times as much on the exo flight, which is three times "
                    "shorter.  It is not the fused multiply-adds (196 of them are under a microsecond per node for a wavefront).  A first "
                    "form of the kernel read A_k, Kf_k and H element by element through scalar loads (H from the kernel argument) and "
                    "measured 1.31 / 1.49 (exo, m = 0 / 6) and 1.16 / 1.22 (aero + fins) in this tool; fetching the matrices with "
                    "coalesced loads a node ahead and reading them from LDS gave the figures above, and moving eps out of the registers "
                    "of the RK4 loop changed the compiler's report (the exo kernel back at 2 waves / SIMD) but not the time: with 128 "
                    "wavefronts on 256 compute units the launch is bound by the latency of one wavefront, not by occupancy.  What is "
                    "left has NOT been attributed by a measurement.  Candidates, in the order of what the code adds outside the RK4 loop: "
                    "the end of the flight reduces 468 statistics over the wavefront where mc_fly_kernel reduces 153, each a chain of six "
                    "dependent cross-lane steps on doubles; per node one more pass of per-lane loads (eta is read a second time, nud at "
                    "m > 0) and two barriers; one more small launch per call.\n\n")
        if a.parent_log and a.log:
            f.write(resource_section(a.parent_log, a.log))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsub", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--models", default="exo,aero+fins")
    ap.add_argument("--json", default=None)
    ap.add_argument("--from-json", default=None)
    ap.add_argument("--resources-only", action="store_true")
    ap.add_argument("--parent-log", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if a.resources_only:
        res = None
    elif a.from_json:
        res = json.load(open(a.from_json))
    else:
        res = measure(a)
        print(json.dumps(res))
        if a.json:
            with open(a.json, "w") as f:
                json.dump(res, f)
    if a.md:
        write_md(res, a)


if __name__ == "__main__":
    main()
