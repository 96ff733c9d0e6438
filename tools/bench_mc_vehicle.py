"""Cost of per-flight vehicle errors in the sampled dispersion (scvx_track_mc_veh_f64, scvx_track_mc_nav_veh_f64) next to the calls
without them, measured in the same run, and what the feature shows on the golden plans.

    python tools/bench_mc_vehicle.py [--nsub 10] [--launches 20] [--repeats 5] [--json out.json]
    python tools/bench_mc_vehicle.py --from-json out.json [--parent-log LOG --log LOG] --md profiles/mc_vehicle.md   (no device needed)

Timing: the set-up of tools/bench_mc_rng.py -- the flyable problem on the exo and the aero + fins model, K = 50, nsub = 10, 128 plans
after `--plan-steps` solve_steps, B S = 8192 flights as 128 x 64 and 8 x 1024, WITH process noise and device draws, truth-fed and flown
on an estimate with m = 6.  `plain`: scvx_track_mc_rng_f64 / scvx_track_mc_nav_rng_f64; `veh`: the _veh form with the same rng and every
component the model has dispersed (the ACT instantiations); `null`: the _veh form with veh = NULL (the plain kernels through the new
entry point).  HIP events, alternating windows, median (min .. max).  Expectation stated with the feature, not a bar: a few multiply-adds
per control component per RK stage and three per-lane constants should be small against the right-hand side.

Show (`show` in the JSON): on the two golden plans of tests/golden/oracle_flight_runs.npz under the device's gains, handover 1e-3 of the
start's position and velocity components and 1e-3 on attitude and rate, 1 sigma = 1e-3 on THRUST, MIS_Y, MIS_Z and ISP: the first-order
budget of the landing position (montecarlo.vehicle_budget on dynamics.vehicle_sensitivity_batch), P_ANY, OUT_LO, OUT_HI and the 99.87 %
miss of 8,192 flights with and without vehicle errors on the same draws, and one round of robustify(mc=dict(vehicle=...)) beside one
without, with the final masses.

--parent-log / --log: the compiler's resource remarks (python -m successiveconvexification_amd.build --force -v) of the parent commit
and of this one; --build-times "parent_mc,parent_nav,mc,nav,veh,nav_veh": seconds of one hipcc per translation unit, measured apart."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_mc import FIELDS, FLYABLE, SHAPES   # noqa: E402

SP = 1e-3   # the 1 sigma of the show


def fly_resources(log):
    """{template arguments: {field: value}} of every mc_fly_kernel instantiation in a verbose build log"""
    out, cur = {}, None
    pat = re.compile(r"remark:\s+(Function Name|%s): (\S+)" % "|".join(re.escape(f) for f in FIELDS))
    for line in open(log, errors="replace"):
        m = pat.search(line)
        if not m:
            continue
        if m.group(1) == "Function Name":
            cur = out.setdefault(m.group(2), {}) if "mc_fly_kernel" in m.group(2) else None
        elif cur is not None:
            cur[m.group(1)] = m.group(2)
    names = subprocess.run(["c++filt"] + list(out), capture_output=True, text=True).stdout.split("\n")
    res = {}
    for mangled, dem in zip(out, names):
        args = re.search(r"mc_fly_kernel<(.*?)>\(", dem).group(1)
        assert len(out[mangled]) == len(FIELDS), (dem, out[mangled])
        res[args] = out[mangled]
    return res


def resource_section(parent_log, log, times):
    par, new = fly_resources(parent_log), fly_resources(log)
    rows, same = [], 0
    for k, r in sorted(new.items()):
        act = "scvx::McVehK" in k
        base = k[:-len(", false")] if k.endswith(", false") else k   # the parent's names end before ACT
        old = None if act else par.get(base)
        tag = "new (ACT)" if act else ("the same" if old == r else "WAS " + " ".join((old or {}).get(f, "?") for f in FIELDS))
        same += tag == "the same"
        rows.append((k.replace(", scvx::McVehK", ""), r, tag))
    lines = ["## Resources: parent against this change\n",
             "The compiler's report (`-Rpass-analysis=kernel-resource-usage`, `--offload-arch=gfx950 -O3`) of every `mc_fly_kernel` "
             "instantiation on the parent commit and on this one.  Template arguments: AERO, FIN, TRQ, PV, RNG, NAV, the tiles' type, "
             "then ACT.  Of the parent's %d instantiations %d report the same figures here in every field below, %d differ; the %d "
             "instantiations with ACT are new.  No instantiation uses scratch: the per-lane copy of the parameter block leaves only "
             "alpha, force_scalar and trq_scalar in vector registers.\n" % (len(par), same, len(par) - same, len(new) - len(par)),
             "| mc_fly_kernel< > | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR spills | waves/SIMD | LDS B/block | parent |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r, tag in rows:
        lines.append("| %s | %s | %s |" % (name, " | ".join(r.get(f, "?") for f in FIELDS), tag))
    if times:
        t = [float(v) for v in times.split(",")]
        lines.append("\n## Build time\n\nOne hipcc per translation unit on one CPU core, seconds, measured once each on the build machine: "
                     "parent `scvx_mc.hip` %.0f, `scvx_mc_nav.hip` %.0f; this change `scvx_mc.hip` %.0f, `scvx_mc_nav.hip` %.0f, and the "
                     "two new units `scvx_mc_veh.hip` %.0f, `scvx_mc_nav_veh.hip` %.0f, which the build compiles beside the others.\n" % tuple(t))
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
    ts = torch.cuda.Stream()
    res = {"nsub": a.nsub, "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "models": {}}

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(a.launches):
            call()
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def timed(*calls):
        for call in calls:
            for _ in range(a.warmup):
                assert call() == 0
        w = [[] for _ in calls]
        for _ in range(a.repeats):
            for i, call in enumerate(calls):
                w[i].append(window(call))
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
        spv = [SP, SP, SP, SP, SP if name != "exo" else 0.0, SP if name != "exo" else 0.0]
        veh = _lib.ScvxMcVehicle((C.c_double * 6)(*[0.0] * 6), (C.c_double * 6)(*spv), (C.c_int32 * 2)(0, 0))
        out = {"shapes": {}}
        for B, S in SHAPES:
            xd, ud, sg, gd, cd, dd, cnd, kfd = (dev(v) for v in (x[:B], u[:B], s[:B], gain[:B], C0[:B], deriv[:B], CN[:B], kf6[:B]))
            rep, xm, xc = torch.empty((B, _lib.MC_NREP), **f64), torch.empty((B, 14), **f64), torch.empty((B, 14, 14), **f64)
            jm, jc, nv = torch.empty((B, 28), **f64), torch.empty((B, 28, 28), **f64), torch.empty((B, 8), **f64)
            plan = (h, B, K, S, vp(xd), vp(ud), vp(sg), vp(gd), vp(cd))
            red = (a.nsub, 0, 0.0, vp(rep), vp(xm), vp(xc))
            noq = (0, None, None, None, None)
            rg = _lib.ScvxMcRng(a.seed, 0, 0, 1, 0)
            o = {}
            plain = lambda: L.scvx_track_mc_rng_f64(*plan, C.byref(rg), 1, dp(sw), None, *red, None, None, None, *noq)   # noqa: E731
            withv = lambda v: (lambda: L.scvx_track_mc_veh_f64(*plan, None, None, dp(sw), None, *red, None, None, None, *noq, C.byref(rg), 1,   # noqa: E731
                                                               v, None, None))
            o["mc"] = dict(zip(("plain", "veh", "null"), timed(plain, withv(C.byref(veh)), withv(None))))
            torch.cuda.synchronize()
            o["mc"]["finite_flights"] = int(B * S - rep[:, 44].sum().item())
            nargs = (dp(w), vp(dd), vp(kfd), vp(cnd))
            ntail = (6, dp(H6), dp(rm6), *red, vp(jm), vp(jc), vp(nv), None, None, None, None, None, *noq)
            nplain = lambda: L.scvx_track_mc_nav_rng_f64(*plan, C.byref(rg), 1, *nargs, *ntail)   # noqa: E731
            nwithv = lambda v: (lambda: L.scvx_track_mc_nav_veh_f64(*plan, None, None, *nargs, None, None, *ntail, C.byref(rg), 1, v, None, None))   # noqa: E731
            o["nav"] = dict(zip(("plain", "veh", "null"), timed(nplain, nwithv(C.byref(veh)), nwithv(None))))
            torch.cuda.synchronize()
            o["nav"]["finite_flights"] = int(B * S - rep[:, 44].sum().item())
            out["shapes"]["%dx%d" % (B, S)] = o
        res["models"][name] = out
        c.set_stream(None)
        c.close()
    res["show"] = show(a)
    return res


def show(a):
    """the budget, the sampled figures with and without vehicle errors, and one round of replanning, on the golden plans"""
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, track_gains_batch,
                                                          track_mc_batch, vehicle_sensitivity_batch)
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_flight_runs.npz"))
    p = replace(sp.base_prob_scaled, **FLYABLE)
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(p, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (p.K + 1))
    L = track_gains_batch(c, d)
    sd = np.zeros(14)
    sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
    sd[7:] = 1e-3
    veh = mc.vehicle_errors(thrust=SP, misalign=SP, isp=SP)
    J = vehicle_sensitivity_batch(c, x, u, s, L)
    covK = cov_propagate_batch(c, x, u, d, L, sd, None, dense=("covK",)).covK
    out = {"sp": SP, "plans": []}
    kw = dict(seed=0, nsub=10, rng="device", quantiles=(0.99865,), tol=0.0)
    r0 = track_mc_batch(c, x, u, s, L, sd, 8192, **kw)
    r1 = track_mc_batch(c, x, u, s, L, sd, 8192, vehicle=veh, **kw)
    for b in range(2):
        bud = mc.vehicle_budget(J[b], veh[1], covK[b][:14, :14])
        row = {"sigma_r": bud["sigma_r"].tolist(), "sigma_v": bud["sigma_v"].tolist(), "share": bud["share"].tolist(),
               "J_norm": np.linalg.norm(J[b], axis=0).tolist()}
        for tag, r in (("without", r0), ("with", r1)):
            row[tag] = {"P_ANY": float(r.P_ANY[b]), "OUT_LO": float(r.OUT_LO[b]), "OUT_HI": float(r.OUT_HI[b]),
                        "MISS_R_q": float(r.quantile("MISS_R", 0.99865)[b]), "MISS_V_q": float(r.quantile("MISS_V", 0.99865)[b]),
                        "sample_sigma_r": float(np.sqrt(np.trace(r.xcov[b][1:4, 1:4])))}
        out["plans"].append(row)
    # one round of replanning on the sampled closed loop, with and without vehicle errors
    ic = np.concatenate([x[:, 0, 1:4], x[:, 0, 4:7]], axis=1)
    rob = {}
    for tag, v in (("without", None), ("with", veh)):
        bt = ScvxBatch(c, 2).init(ic)
        st0 = bt.solve()[0]
        m0 = bt.trajectory()[0][:, -1, 0].copy()
        st, it, _, _, lo, hi = bt.robustify(sd, mc=dict(p=0.99865, samples=1024, rng="device", vehicle=v))
        rob[tag] = {"status0": st0.tolist(), "status": st.tolist(), "iters": np.asarray(it).tolist(), "mass0": m0.tolist(),
                    "mass": bt.trajectory()[0][:, -1, 0].tolist(), "lo_max": lo.max(axis=1).tolist(), "hi_max": hi.max(axis=1).tolist()}
        bt.close()
    out["robustify"] = rob
    c.close()
    return out


def write_md(res, a):
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    with open(a.md, "w") as f:
        f.write("# Vehicle errors in the sampled dispersion\n\n")
        f.write("Device time at B S = 8192 flights, K = 50, nsub = %d, WITH process noise and device draws (independent = 1).  "
                "`python tools/bench_mc_vehicle.py`; %s; HIP events; per entry %d windows of %d launches after %d warm-up launches, median "
                "(min .. max) of the windows in ms; fp64; the set-up of profiles/mc_rng.md.  `plain`: scvx_track_mc_rng_f64 / "
                "scvx_track_mc_nav_rng_f64; `veh`: scvx_track_mc_veh_f64 / scvx_track_mc_nav_veh_f64 with 1 sigma = 1e-3 on every component "
                "the model has (the ACT instantiations); `null`: the same entry points with veh = NULL (the plain kernels); the three in "
                "alternating windows of one run.\n\n" % (res["nsub"], res["device"], res["repeats"], res["launches"], res["warmup"]))
        f.write("| model | call | B x S | plain | veh | veh / plain - 1 | null | null / plain - 1 |\n|---|---|---|---|---|---|---|---|\n")
        ratios = []
        for name, m in res["models"].items():
            for shp, o in m["shapes"].items():
                for key in ("mc", "nav"):
                    q = o[key]
                    r1, r2 = q["veh"][0] / q["plain"][0] - 1.0, q["null"][0] / q["plain"][0] - 1.0
                    ratios.append(r1)
                    f.write("| %s | %s | %s | %s | %s | %+.1f %% | %s | %+.1f %% |\n"
                            % (name, key, shp.replace("x", " x "), fmt(q["plain"]), fmt(q["veh"]), 100 * r1, fmt(q["null"]), 100 * r2))
        every = [o[k] for m in res["models"].values() for o in m["shapes"].values() for k in ("mc", "nav")]
        f.write("\nEvery flight of every timed call is finite: %s.\n" % all(q["finite_flights"] == 8192 for q in every))
        f.write("\nExpectation stated with the feature (not a bar): small against the right-hand side.  Measured, veh / plain - 1: "
                "%+.1f %% .. %+.1f %%.\n\n" % (100 * min(ratios), 100 * max(ratios)))
        sh = res.get("show")
        if sh:
            names = ("THRUST", "MIS_Y", "MIS_Z", "ISP", "AERO", "FIN", "handover")
            f.write("## What it shows (device figures)\n\nThe two golden plans under the device's gains, handover 1 sigma 1e-3 of the start's "
                    "position and velocity components and 1e-3 on attitude and rate, vehicle errors 1 sigma = %g on THRUST, MIS_Y, MIS_Z "
                    "(radians) and ISP.  First-order budget of the landing position, 1 sigma by component (normalised units), "
                    "montecarlo.vehicle_budget on dynamics.vehicle_sensitivity_batch and scvx_cov_propagate_f64:\n\n" % sh["sp"])
            f.write("| plan | " + " | ".join(names) + " | share of the trace by vehicle errors |\n|---|" + "---|" * 8 + "\n")
            for b, row in enumerate(sh["plans"]):
                f.write("| %d | %s | %.1f %% |\n" % (b, " | ".join("%.2e" % v for v in row["sigma_r"]), 100 * sum(row["share"][:6])))
            f.write("\n8,192 sampled flights per plan (device draws, seed 0, no process noise, no clamp), without and with the vehicle errors "
                    "on the same draws:\n\n| plan | vehicle errors | P_ANY | OUT_LO | OUT_HI | 99.87 % MISS_R | 99.87 % MISS_V | sample 1 sigma of "
                    "the landing position |\n|---|---|---|---|---|---|---|---|\n")
            for b, row in enumerate(sh["plans"]):
                for tag in ("without", "with"):
                    q = row[tag]
                    f.write("| %d | %s | %.4f | %.5f | %.5f | %.3e | %.3e | %.3e |\n" % (b, tag, q["P_ANY"], q["OUT_LO"], q["OUT_HI"],
                                                                                        q["MISS_R_q"], q["MISS_V_q"], q["sample_sigma_r"]))
            f.write("\nOne round of `robustify(mc=dict(p=0.99865, samples=1024, rng=\"device\", vehicle=...))` from the converged plans of "
                    "the golden starts, beside the same round without vehicle errors:\n\n| vehicle errors | status before -> after | steps | "
                    "final mass before | final mass after | largest back-off lo | hi |\n|---|---|---|---|---|---|---|\n")
            for tag in ("without", "with"):
                q = sh["robustify"][tag]
                js = lambda v, spec: ", ".join(spec % e for e in v)   # noqa: E731
                f.write("| %s | %s -> %s | %s | %s | %s | %s | %s |\n" % (tag, js(q["status0"], "%d"), js(q["status"], "%d"), js(q["iters"], "%d"),
                        js(q["mass0"], "%.5f"), js(q["mass"], "%.5f"), js(q["lo_max"], "%.4f"), js(q["hi_max"], "%.4f")))
            f.write("\n")
        if a.note:
            f.write(open(a.note).read().rstrip("\n") + "\n\n")
        if a.parent_log and a.log:
            f.write(resource_section(a.parent_log, a.log, a.build_times))


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
    ap.add_argument("--parent-log", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--build-times", default=None)
    ap.add_argument("--note", default=None, help="a text file placed between the measurements and the resource tables")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    if a.from_json:
        res = json.load(open(a.from_json))
    else:
        res = measure(a)
        print(json.dumps(res))
        if a.json:
            os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
            with open(a.json, "w") as f:
                json.dump(res, f)
    if a.md:
        write_md(res, a)


if __name__ == "__main__":
    main()
