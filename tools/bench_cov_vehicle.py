"""Cost of the vehicle errors in the first-order analyses (scvx_vehicle_tiles_f64, scvx_cov_vehicle_f64, scvx_nav_cov_vehicle_f64 and
the batch forms) next to the calls they extend, measured in the same run, and what the analysis shows on the golden plans.

    python tools/bench_cov_vehicle.py [--plans 8192] [--launches 10] [--repeats 5] [--json out.json] [--md out.md]

Timing: the flyable problem on the exo and the aero + fins model, K = 50, nsub = 10, `--plans` plans after `--plan-steps` solve_steps.
Kernel times by HIP events in alternating windows of one run, median (min .. max) per launch:
  * the covariance launch with VEH beside the plain PS launch (scvx_cov_path_sigma_f64), the navigation launch likewise (m = 3),
  * the vehicle-tile launch beside K2 (scvx_propagate_f64) and beside the K1 launch (scvx_linearize_f64),
and wall times of the batch calls, median of `--repeats`: margins_from_cov(vehicle=) beside margins_from_cov, and one round of
robustify(vehicle=) beside robustify(mc=dict(vehicle=..., samples=1024, rng="device")) on `--rob-plans` plans.
Expectation stated with the feature, not a bar: the J step is n 6 n multiply-adds and the rank-6 update n n 6, beside 2 n^3 for the two
products -- about a third more arithmetic in a kernel bound by its LDS traffic and barriers, so well under +50 %; the tile launch should
cost about what K2 costs times a small factor for the Jacobian.

Show: on the two golden plans of tests/golden/oracle_flight_runs.npz under the device's gains, handover 1e-3 of the start's position
and velocity components and 1e-3 on attitude and rate, 1 sigma = 1e-3 on THRUST, MIS_Y, MIS_Z and ISP: SIG_R, N_TMIN, N_TMAX and the
landing-variance share with and without vehicle errors, covariance and navigation form."""
import argparse
import ctypes as C
import json
import os
import sys
import time
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_mc import FLYABLE   # noqa: E402

SP = 1e-3


def measure(a):
    import torch
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.defns import AtmosphericData
    from successiveconvexification_amd.dynamics import IntegratorCache
    z = np.load(os.path.join(ROOT, "tests", "golden", "lift_drag_tables.npz"))
    aero = AtmosphericData(z["drag"], z["lift"], z["torque"])
    models = {"exo": lambda: replace(sp.base_prob_scaled, **FLYABLE), "aero+fins": lambda: replace(sp.base_prob_fin_scaled(aero), **FLYABLE)}
    ts = torch.cuda.Stream()
    res = {"plans": a.plans, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "models": {}}

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(a.launches):
            call()
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def timed(calls):
        for call in calls.values():
            for _ in range(a.warmup):
                assert call() == 0
        w = {k: [] for k in calls}
        for _ in range(a.repeats):
            for k, call in calls.items():
                w[k].append(window(call))
        return {k: [float(np.median(v)), float(min(v)), float(max(v))] for k, v in w.items()}

    def wall(call):
        v = []
        for _ in range(a.repeats):
            t = time.perf_counter()
            call()
            v.append(1e3 * (time.perf_counter() - t))
        return [float(np.median(v)), float(min(v)), float(max(v))]

    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    dev = lambda v: torch.tensor(np.ascontiguousarray(v), device="cuda")   # noqa: E731
    f64 = dict(dtype=torch.float64, device="cuda")
    for name in a.models.split(","):
        p = models[name]()
        K, B = p.K, a.plans
        c = IntegratorCache(p, npts=10)
        c.set_stream(ts.cuda_stream)
        b = ScvxBatch(c, B).init(mc.disperse_ics(p, 0, B, a.seed))
        for _ in range(a.plan_steps):
            b.solve_step_async()
        x, u, s = b.trajectory()
        gain, deriv = b.track_gains(), b.linearization()[1]
        L, h, nu = c._L, c.handle, c.nu
        n = 14 + nu
        sd = np.zeros(14)
        sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
        sd[7:] = 1e-3
        S0 = np.broadcast_to(np.diag(sd * sd), (B, 14, 14))
        H = mc.measurement_rows("r")
        rm = np.full(3, (3e-5 * np.abs(x[0, 0, 1:4]).max()) ** 2)
        spv = np.array([SP, SP, SP, SP, SP if name != "exo" else 0.0, SP if nu == 5 else 0.0])
        dx, du, dsg, dd, dg, d0 = (dev(v) for v in (x, u, s, deriv, gain, S0))
        rep, nrep = torch.empty(B, 16, **f64), torch.empty(B, 8, **f64)
        psig, vt = torch.empty(B, K + 1, 5, **f64), torch.empty(B, K, 2, 14, **f64)
        xn, de = torch.empty(B, K, 14, **f64), torch.empty(B, K, 14 + 2 * nu + 1, 14, **f64)
        dt = 1.0 / (K + 1)
        assert L.scvx_vehicle_tiles_f64(h, B, K, vp(dx), vp(du), vp(dsg), vp(vt)) == 0
        cov = (h, B, K, vp(dx), vp(du), vp(dd), vp(dg), vp(d0), None, vp(rep))
        nav = (h, B, K, vp(dx), vp(du), vp(dd), vp(dg), vp(d0), vp(d0), 3, dp(H), dp(rm), None, vp(rep), vp(nrep))
        m = {"kernels": timed({
            "cov_ps": lambda: L.scvx_cov_path_sigma_f64(*cov, vp(psig)),
            "cov_veh": lambda: L.scvx_cov_vehicle_f64(*cov, vp(psig), None, None, None, vp(vt), dp(spv), None),
            "nav_ps": lambda: L.scvx_nav_path_sigma_f64(*nav, vp(psig)),
            "nav_veh": lambda: L.scvx_nav_cov_vehicle_f64(*nav, vp(psig), None, None, None, None, vp(vt), dp(spv), None),
            "vtile": lambda: L.scvx_vehicle_tiles_f64(h, B, K, vp(dx), vp(du), vp(dsg), vp(vt)),
            "k2": lambda: L.scvx_propagate_f64(h, B, K, vp(dx), vp(du), vp(dsg), dt, vp(xn)),
            "k1": lambda: L.scvx_linearize_f64(h, B, K, vp(dx), vp(du), vp(dsg), dt, vp(xn), vp(de))})}
        veh = (np.zeros(6), spv)
        b.margins_from_cov(S0), b.margins_from_cov(S0, vehicle=veh)
        m["margins_from_cov_ms"] = wall(lambda: b._margins_from_cov(S0, None, None, None, None, 3.0, 0.25, False, 31))
        m["margins_from_cov_veh_ms"] = wall(lambda: b._margins_from_cov(S0, None, None, None, None, 3.0, 0.25, False, 31, veh))
        b.close()
        # one round of robustify on converged plans: the first-order path with vehicle errors beside the sampled one
        R = a.rob_plans
        rob = {}
        for tag, kw in (("vehicle", dict(vehicle=veh)), ("mc", dict(mc=dict(vehicle=veh, samples=1024, rng="device")))):
            bb = ScvxBatch(c, R).init(mc.disperse_ics(p, 0, R, a.seed))
            st = bb.solve()[0]
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = bb.robustify(S0[:R], nsigma=3.0, rounds=1, **kw)
            rob[tag] = {"ms": 1e3 * (time.perf_counter() - t), "converged_before": int((st == 0).sum()), "converged": int((out[0] == 0).sum()),
                        "steps": [int(v) for v in out[1][:8]]}
            bb.close()
        m["robustify"] = rob
        res["models"][name] = m
        c.close()
    res["show"] = show()
    return res


def show():
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, nav_cov_batch, track_gains_batch,
                                                          vehicle_tiles_batch)
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_flight_runs.npz"))
    p = replace(sp.base_prob_scaled, **FLYABLE)
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(p, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (p.K + 1))
    L = track_gains_batch(c, d)
    sd = np.zeros((2, 14))
    sd[:, 1:7] = 1e-3 * np.abs(x[:, 0, 1:7])
    sd[:, 7:] = 1e-3
    S0 = np.stack([np.diag(v * v) for v in sd])
    veh = mc.vehicle_errors(thrust=SP, misalign=SP, isp=SP)
    vt = vehicle_tiles_batch(c, x, u, s)
    H = mc.measurement_rows("r")
    rm = np.full(3, (3e-5 * np.abs(x[0, 0, 1:4]).max()) ** 2)
    out = {}
    for tag, call in (("cov", lambda **kw: cov_propagate_batch(c, x, u, d, L, S0, dense=("covK",), **kw)),
                      ("nav", lambda **kw: nav_cov_batch(c, x, u, d, L, S0, S0, H, rm, dense=("joint",), **kw))):
        r0, r1 = call(), call(vehicle=veh, vtile=vt)
        lk = (lambda r: r.covK[:, :14, :14]) if tag == "cov" else (lambda r: r.joint[:, -1, :14, :14])
        t0, t1 = np.trace(lk(r0), axis1=1, axis2=2), np.trace(lk(r1), axis1=1, axis2=2)
        out[tag] = {k: [getattr(r0, k).tolist(), getattr(r1, k).tolist()] for k in ("SIG_R", "SIG_V", "SIG_M", "S_THRUST", "N_TMIN", "N_TMAX")}
        out[tag]["share"] = ((t1 - t0) / t1).tolist()
    c.close()
    return out


def markdown(r):
    f = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    lines = ["## Timings\n", "%s, %d plans, K = 50, nsub = 10; kernel times in ms per launch by HIP events, %d launches per window, %d alternating "
             "windows, median (min .. max).\n" % (r["device"], r["plans"], r["launches"], r["repeats"]),
             "| model | cov PS | cov VEH | ratio | nav PS | nav VEH | ratio | vehicle tiles | K2 | tiles / K2 | K1 | tiles / K1 |", "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for name, m in r["models"].items():
        k = m["kernels"]
        lines.append("| %s | %s | %s | %.2f | %s | %s | %.2f | %s | %s | %.2f | %s | %.2f |" % (
            name, f(k["cov_ps"]), f(k["cov_veh"]), k["cov_veh"][0] / k["cov_ps"][0], f(k["nav_ps"]), f(k["nav_veh"]),
            k["nav_veh"][0] / k["nav_ps"][0], f(k["vtile"]), f(k["k2"]), k["vtile"][0] / k["k2"][0], f(k["k1"]), k["vtile"][0] / k["k1"][0]))
    lines += ["\nBatch calls, wall ms (gains, analysis and back-off kernel; with vehicle errors the tile launch in front):\n",
              "| model | margins_from_cov | margins_from_cov(vehicle=) | robustify(vehicle=), one round | robustify(mc=dict(vehicle=, samples=1024, rng=\"device\")), one round |",
              "|---|---|---|---|---|"]
    for name, m in r["models"].items():
        rb = m["robustify"]
        lines.append("| %s | %s | %s | %.1f (%d converged, %d before the round; steps %s) | %.1f (%d converged, steps %s) |" % (
            name, f(m["margins_from_cov_ms"]), f(m["margins_from_cov_veh_ms"]), rb["vehicle"]["ms"], rb["vehicle"]["converged"],
            rb["vehicle"]["converged_before"], rb["vehicle"]["steps"], rb["mc"]["ms"], rb["mc"]["converged"], rb["mc"]["steps"]))
    lines += ["\n## What the analysis shows on the two golden plans (the device's)\n",
              "1 sigma = 1e-3 on THRUST, MIS_Y, MIS_Z and ISP; [without, with] vehicle errors, per plan.\n", "```", json.dumps(r["show"], indent=1), "```"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=8192)
    ap.add_argument("--rob-plans", type=int, default=64)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--models", default="exo,aero+fins")
    ap.add_argument("--json")
    ap.add_argument("--md")
    a = ap.parse_args()
    r = measure(a)
    if a.json:
        json.dump(r, open(a.json, "w"), indent=1)
    md = markdown(r)
    if a.md:
        open(a.md, "w").write(md)
    print(md)
