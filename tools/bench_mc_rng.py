"""Cost of making the sampled dispersion's draws on the device (scvx_track_mc_rng_f64, scvx_track_mc_nav_rng_f64) next to the calls on
uploaded draws, measured in the same run, kernel time and end to end from Python.

    python tools/bench_mc_rng.py [--nsub 10] [--launches 20] [--repeats 5] [--json out.json]
    python tools/bench_mc_rng.py --from-json out.json [--parent-log LOG --log LOG] --md profiles/mc_rng.md   (no device needed)

For the flyable problem (mdry = 0.55, tf_guess = 8) on the exo and the aero + fins model, K = 50, nsub = 10: 128 dispersed plans are
stepped `--plan-steps` times to get physical plans, their tiles and their gains.  Then B S = 8192 flights as 128 x 64 and as 8 x 1024,
WITH process noise, truth-fed and flown on an estimate with m = 6 (position and velocity measured):
  * `plain`: scvx_track_mc_f64 / scvx_track_mc_nav_f64 on uploaded draws already on the device (kernel time only), in windows
    alternating with
  * `shared` and `independent`: scvx_track_mc_rng_f64 / scvx_track_mc_nav_rng_f64 with independent = 0 and 1;
  * end to end from Python, wall clock: dynamics.track_mc_batch(rng="host"), which makes the draws with montecarlo.mc_draws (and
    mc_nav_draws) and uploads them, beside rng="device"; and the host generator alone.
HIP events for the kernel times, `--repeats` windows of `--launches` launches after a warm-up, median (min .. max) of the windows; the
end-to-end figures are the median (min .. max) of `--e2e` calls.  Estimate stated with the feature, not a bar: a Philox block costs 20
64 x 64 -> 128 bit multiplies on quarter-rate integer multiplies, so with noise the fused call should cost 10 - 30 % more kernel time
than the plain one on the exo model and far less on aero + fins.  --parent-log / --log: the compiler's resource remarks
(-Rpass-analysis=kernel-resource-usage, the flags of successiveconvexification_amd.build -v) of the parent commit and of this one."""
import argparse
import ctypes as C
import json
import os
import re
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_mc import FIELDS, FLYABLE, SHAPES, resources   # noqa: E402  the verbose build log's parser and the flyable problem


def _key(name):
    """(kernel<template arguments without RNG>, RNG) of a flying kernel of the sampled calls from its mangled name; the parent's names
    lack the trailing RNG argument.  None for every other kernel"""
    m = re.match(r"_ZN4scvx\d+(mc_fly_kernel|mc_nav_fly_kernel)I((?:Lb[01]E)+)([df]?)((?:Lb[01]E)*)E", name)
    if not m:
        return None
    b = ["true" if v == "1" else "false" for v in re.findall(r"Lb([01])E", m.group(2))]
    t = {"d": ["double"], "f": ["float"], "": []}[m.group(3)]
    tail = ["true" if v == "1" else "false" for v in re.findall(r"Lb([01])E", m.group(4))]
    args = b + t + tail
    full = 5 if m.group(1) == "mc_fly_kernel" else 6
    rng = len(args) == full and args[-1] == "true"
    if len(args) == full:
        args = args[:-1]
    return "%s<%s>" % (m.group(1), ", ".join(args)), rng


def resource_section(parent_log, log):
    par, new = resources(parent_log), resources(log)
    pk = {_key(n): r for n, r in par.items() if _key(n)}
    rows, same, differ = [], 0, 0
    for n, r in new.items():
        k = _key(n)
        if k is None:
            if "mc_draws_kernel" in n:
                rows.append(("mc_draws_kernel", r, "new"))
            continue
        if k[1]:
            rows.append((k[0][:-1] + ", RNG>", r, "new"))
            continue
        old = pk.get(k)
        tag = "the same" if old == r else ("WAS " + " ".join(old.get(f, "?") for f in FIELDS) if old else "new")
        same += tag == "the same"
        differ += tag.startswith("WAS")
        rows.append((k[0], r, tag))
    lines = ["## Resources: parent against this change\n",
             "The compiler's report (`-Rpass-analysis=kernel-resource-usage`, `--offload-arch=gfx950 -O3`, the flags of "
             "`python -m successiveconvexification_amd.build --force -v`) of the two translation units that hold the flying kernels, "
             "`csrc/scvx_mc.hip` and `csrc/scvx_mc_nav.hip`, on the parent commit and on this one; no other kernel of the library is "
             "touched.  The two flying kernels gained one compile-time parameter, RNG, and one trailing kernel argument (the stream): their "
             "instantiations with RNG off are matched to the parent's by their other template arguments.  Of the parent's %d "
             "instantiations %d report the same figures here (every field below), %d differ.  New: the instantiations with RNG on and "
             "mc_draws_kernel.  With RNG the navigation kernel keeps eta_k in LDS between the error's time step and the truth's impulse "
             "(7,168 bytes more per block).\n" % (len(pk), same, differ),
             "| kernel | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR spills | waves/SIMD | LDS B/block | parent |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r, tag in sorted(rows, key=lambda t: ("draws" in t[0], "nav" in t[0], "RNG" in t[0], t[0])):
        lines.append("| %s | %s | %s |" % (name, " | ".join(r.get(f, "?") for f in FIELDS), tag))
    return "\n".join(lines) + "\n"


def measure(a):
    import torch
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.defns import AtmosphericData
    from successiveconvexification_amd.dynamics import IntegratorCache, track_mc_batch
    z = np.load(os.path.join(ROOT, "tests", "golden", "lift_drag_tables.npz"))
    aero = AtmosphericData(z["drag"], z["lift"], z["torque"])
    models = {"exo": lambda: replace(sp.base_prob_scaled, **FLYABLE), "aero+fins": lambda: replace(sp.base_prob_fin_scaled(aero), **FLYABLE)}
    ts = torch.cuda.Stream()   # torch's events see kernels on a torch stream: the context runs on one for this tool
    res = {"nsub": a.nsub, "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup, "e2e": a.e2e,
           "device": torch.cuda.get_device_name(0), "models": {}}

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(a.launches):
            call()
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def timed(*calls):
        """[median, min, max] ms per launch over the windows, per call, in alternating windows"""
        for call in calls:
            for _ in range(a.warmup):
                assert call() == 0
        w = [[] for _ in calls]
        for _ in range(a.repeats):
            for i, call in enumerate(calls):
                w[i].append(window(call))
        return [[float(np.median(v)), float(min(v)), float(max(v))] for v in w]

    def wall(fn):
        fn()
        v = []
        for _ in range(a.e2e):
            t = time.perf_counter()
            fn()
            v.append(1e3 * (time.perf_counter() - t))
        return [float(np.median(v)), float(min(v)), float(max(v))]

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
        L, h = c._L, c.handle
        sd = np.zeros(14)
        sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
        sd[7:] = 1e-3
        w = np.full(14, 1e-10)
        sw = np.sqrt(w)
        H6 = mc.measurement_rows("rv")
        rm6 = np.repeat([(3e-5 * np.abs(x[0, 0, 1:4]).max()) ** 2, (3e-5 * np.abs(x[0, 0, 4:7]).max()) ** 2], 3)
        kf6 = b.navigation(sd, 0.5 * sd, H6, rm6, w=w, dense=("kf",)).kf
        b.close()
        C0 = np.stack([mc.handover_factor(sd)] * PB)
        CN = 0.5 * C0
        out = {"shapes": {}}
        for B, S in SHAPES:
            xi0, eta = mc.mc_draws(S, K, a.seed, noise=True)
            xin, nud = mc.mc_nav_draws(S, K, 6, a.seed)
            xd, ud, sg, gd, cd, xid, etd, dd, cnd, xnd, ndd, kfd = (dev(v) for v in (x[:B], u[:B], s[:B], gain[:B], C0[:B], xi0, eta, deriv[:B],
                                                                                     CN[:B], xin, nud, kf6[:B]))
            rep, xm, xc = torch.empty((B, _lib.MC_NREP), **f64), torch.empty((B, 14), **f64), torch.empty((B, 14, 14), **f64)
            jm, jc, nv = torch.empty((B, 28), **f64), torch.empty((B, 28, 28), **f64), torch.empty((B, 8), **f64)
            plan = (h, B, K, S, vp(xd), vp(ud), vp(sg), vp(gd), vp(cd))
            red = (a.nsub, 0, 0.0, vp(rep), vp(xm), vp(xc))
            noq = (0, None, None, None, None)
            rgs = {"shared": _lib.ScvxMcRng(a.seed, 0, 0, 0, 0), "independent": _lib.ScvxMcRng(a.seed, 0, 0, 1, 0)}
            o = {}
            plain = lambda: L.scvx_track_mc_f64(*plan, vp(xid), vp(etd), dp(sw), None, *red, None, None, None)   # noqa: E731
            fused = lambda g: (lambda: L.scvx_track_mc_rng_f64(*plan, C.byref(g), 1, dp(sw), None, *red, None, None, None, *noq))   # noqa: E731
            o["mc"] = dict(zip(("plain", "shared", "independent"), timed(plain, fused(rgs["shared"]), fused(rgs["independent"]))))
            torch.cuda.synchronize()
            o["mc"]["finite_flights"] = int(B * S - rep[:, 44].sum().item())
            nplain = lambda: L.scvx_track_mc_nav_f64(*plan, vp(xid), vp(etd), dp(w), vp(dd), vp(kfd), vp(cnd), vp(xnd), vp(ndd), 6, dp(H6),   # noqa: E731
                                                     dp(rm6), *red, vp(jm), vp(jc), vp(nv), None, None, None, None, None)
            nfused = lambda g: (lambda: L.scvx_track_mc_nav_rng_f64(*plan, C.byref(g), 1, dp(w), vp(dd), vp(kfd), vp(cnd), 6, dp(H6), dp(rm6),   # noqa: E731
                                                                    *red, vp(jm), vp(jc), vp(nv), None, None, None, None, None, *noq))
            o["nav"] = dict(zip(("plain", "shared", "independent"), timed(nplain, nfused(rgs["shared"]), nfused(rgs["independent"]))))
            torch.cuda.synchronize()
            o["nav"]["finite_flights"] = int(B * S - rep[:, 44].sum().item())
            # end to end from Python: the host generator, the upload and the call
            a0 = (c, x[:B], u[:B], s[:B], gain[:B], sd, S)
            nav6 = (0.5 * sd, H6, rm6)
            for key, nv_ in (("mc", None), ("nav", nav6)):
                o[key]["e2e_host"] = wall(lambda: track_mc_batch(*a0, seed=a.seed, w=w, nsub=a.nsub, nav=nv_))
                o[key]["e2e_device"] = wall(lambda: track_mc_batch(*a0, seed=a.seed, w=w, nsub=a.nsub, nav=nv_, rng="device"))
                o[key]["e2e_independent"] = wall(lambda: track_mc_batch(*a0, seed=a.seed, w=w, nsub=a.nsub, nav=nv_, rng="device", independent=True))
            o["mc"]["draws_host"] = wall(lambda: mc.mc_draws(S, K, a.seed, noise=True))
            o["nav"]["draws_host"] = wall(lambda: (mc.mc_draws(S, K, a.seed, noise=True), mc.mc_nav_draws(S, K, 6, a.seed)))
            o["draw_bytes_shared"] = (xi0.size + eta.size + xin.size + nud.size) * 8
            o["draw_bytes_independent"] = B * S * (1 + K) * 28 * 8
            out["shapes"]["%dx%d" % (B, S)] = o
        res["models"][name] = out
        c.set_stream(None)
        c.close()
    return res


def write_md(res, a):
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    with open(a.md, "w") as f:
        f.write("# The sampled dispersion's draws made on the device\n\n")
        f.write("Device time at B S = 8192 flights, K = 50, nsub = %d, WITH process noise.  `python tools/bench_mc_rng.py`; %s; HIP events; per "
                "entry %d windows of %d launches after %d warm-up launches, median (min .. max) of the windows in ms; fp64; flyable problem "
                "(mdry = 0.55, tf_guess = 8), plans after 3 solve_steps, weights q = 1, r = 1, qf = 100, handover 1e-3, navigation handover "
                "half of it, w = 1e-10; `nav`: flown on an estimate, m = 6 (position and velocity measured at every node).  `plain`: "
                "scvx_track_mc_f64 / scvx_track_mc_nav_f64 on draws that are already on the device, no dense output; `shared`, "
                "`independent`: scvx_track_mc_rng_f64 / scvx_track_mc_nav_rng_f64 with independent = 0 / 1, every lane making its own "
                "draws (Philox4x64-10, Box-Muller); the three in alternating windows of one run.\n\n"
                % (res["nsub"], res["device"], res["repeats"], res["launches"], res["warmup"]))
        f.write("| model | call | B x S | plain | shared | shared / plain - 1 | independent | independent / plain - 1 |\n|---|---|---|---|---|---|---|---|\n")
        ratios = {}
        for name, m in res["models"].items():
            for shp, o in m["shapes"].items():
                for key in ("mc", "nav"):
                    q = o[key]
                    r1, r2 = q["shared"][0] / q["plain"][0] - 1.0, q["independent"][0] / q["plain"][0] - 1.0
                    ratios.setdefault((name, key), []).extend([r1, r2])
                    f.write("| %s | %s | %s | %s | %s | %+.1f %% | %s | %+.1f %% |\n"
                            % (name, key, shp.replace("x", " x "), fmt(q["plain"]), fmt(q["shared"]), 100 * r1, fmt(q["independent"]), 100 * r2))
        every = [o[k] for m in res["models"].values() for o in m["shapes"].values() for k in ("mc", "nav")]
        f.write("\nEvery flight of every timed call is finite: %s.\n" % all(q["finite_flights"] == 8192 for q in every))
        f.write("\nEstimate stated with the feature (an estimate, not a bar): with process noise the fused call should cost 10 - 30 %% more "
                "kernel time than the plain call on the exo model, and far less on aero + fins.  Measured, fused / plain - 1: %s.\n\n"
                % "; ".join("%s %s %+.1f %% .. %+.1f %%" % (n, k, 100 * min(v), 100 * max(v)) for (n, k), v in ratios.items()))
        f.write("## End to end from Python\n\n")
        f.write("Wall clock of one `dynamics.track_mc_batch` call (host arrays in, the reduced report out; median (min .. max) of %d calls "
                "after one warm-up, ms): `rng=\"host\"` makes the draws with montecarlo.mc_draws (and mc_nav_draws), one numpy generator per "
                "sample, and uploads them; `rng=\"device\"` uploads the plans alone.  `host generator`: the draws' share of the host call, "
                "timed alone.  The uploaded draws are shared by all plans; independent draws as uploaded arrays would be B S (K + 1) 28 "
                "doubles.\n\n" % res["e2e"])
        f.write("| model | call | B x S | rng=\"host\" | host generator alone | rng=\"device\" | device, independent | host / device | uploaded draws | "
                "the same, independent |\n|---|---|---|---|---|---|---|---|---|---|\n")
        for name, m in res["models"].items():
            for shp, o in m["shapes"].items():
                for key in ("mc", "nav"):
                    q = o[key]
                    f.write("| %s | %s | %s | %s | %s | %s | %s | %.1f x | %.1f MB | %.1f MB |\n"
                            % (name, key, shp.replace("x", " x "), fmt(q["e2e_host"]), fmt(q["draws_host"]), fmt(q["e2e_device"]),
                               fmt(q["e2e_independent"]), q["e2e_host"][0] / q["e2e_device"][0], o["draw_bytes_shared"] / 1e6,
                               o["draw_bytes_independent"] / 1e6))
        f.write("\n")
        if a.note:
            f.write(open(a.note).read().rstrip("\n") + "\n\n")
        if a.parent_log and a.log:
            f.write(resource_section(a.parent_log, a.log))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsub", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--e2e", type=int, default=5)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--models", default="exo,aero+fins")
    ap.add_argument("--json", default=None)
    ap.add_argument("--from-json", default=None)
    ap.add_argument("--parent-log", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--note", default=None, help="a text file placed between the measurements and the resource tables")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if a.from_json:
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
