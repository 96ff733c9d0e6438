"""Cost of the segment audit (scvx_segment_audit_f64) next to the PLAN-mode flight check and K2 of the same run, one round of harden
beside one round of robustify, and what hardening by replanning does on the golden starts.

    python tools/bench_audit.py [--plans 1,256,8192] [--launches 10] [--repeats 5] [--json out.json] [--md out.md]

Timing: the flyable problem on the exo and the aero + fins model, K = 50, nsub = 10, B plans after `--plan-steps` solve_steps.  Kernel
times by HIP events in alternating windows of one run, median (min .. max) per launch: the audit launch with and without the reduced
report, scvx_flight_check_f64 in PLAN mode, K2 (scvx_propagate_f64).  Wall times of one round of harden(("thrust", "tilt")) and one
round of robustify(constraints=("thrust", "tilt")) on `--rob-plans` converged plans.
Expectation stated with the feature, not a bar: the audit is K2's parallelisation with the path functions added, so its launch should
cost about what K2 costs at B = 8,192, and far less than the flight check at B <= 256, where the check walks K segments on one lane.

Show: ScvxBatch.harden(("thrust", "tilt"), restart="replan") and restart="guess" on the two golden starts of
tests/golden/oracle_flight_runs.npz: rounds used, statuses, final masses, worst selected G before and after."""
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
    res = {"launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "models": {}}

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

    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    dev = lambda v: torch.tensor(np.ascontiguousarray(v), device="cuda")   # noqa: E731
    f64 = dict(dtype=torch.float64, device="cuda")
    for name in a.models.split(","):
        p = models[name]()
        K = p.K
        c = IntegratorCache(p, npts=10)
        c.set_stream(ts.cuda_stream)
        L, h = c._L, c.handle
        m = {"kernels": {}}
        for B in [int(v) for v in a.plans.split(",")]:
            b = ScvxBatch(c, B).init(mc.disperse_ics(p, 0, B, a.seed))
            for _ in range(a.plan_steps):
                b.solve_step_async()
            x, u, s = b.trajectory()
            b.close()
            dx, du, dsg = (dev(v) for v in (x, u, s))
            seg, rep, xn = torch.empty(B, K, 11, **f64), torch.empty(B, 16, **f64), torch.empty(B, K, 14, **f64)
            m["kernels"][str(B)] = timed({
                "audit": lambda: L.scvx_segment_audit_f64(h, B, K, vp(dx), vp(du), vp(dsg), 10, vp(seg), None),
                "audit_report": lambda: L.scvx_segment_audit_f64(h, B, K, vp(dx), vp(du), vp(dsg), 10, vp(seg), vp(rep)),
                "flight_plan": lambda: L.scvx_flight_check_f64(h, B, K, vp(dx), vp(du), vp(dsg), 10, 1, vp(rep), None),
                "k2": lambda: L.scvx_propagate_f64(h, B, K, vp(dx), vp(du), vp(dsg), 1.0 / (K + 1), vp(xn))})
        # one round on converged plans: harden beside robustify, the same two constraints
        R = a.rob_plans
        S0 = np.broadcast_to(1e-6 * np.eye(14), (R, 14, 14))
        rounds = {}
        for tag, run in (("harden", lambda bb: bb.harden(("thrust", "tilt"), rounds=1)),
                         ("robustify", lambda bb: bb.robustify(S0, rounds=1, constraints=("thrust", "tilt")))):
            bb = ScvxBatch(c, R).init(mc.disperse_ics(p, 0, R, a.seed))
            st = bb.solve()[0]
            torch.cuda.synchronize()
            t = time.perf_counter()
            out = run(bb)
            rounds[tag] = {"ms": 1e3 * (time.perf_counter() - t), "converged_before": int((st == 0).sum()), "converged": int((out[0] == 0).sum()),
                           "steps": [int(v) for v in out[1][:8]], "status": {int(k): int(v) for k, v in zip(*np.unique(out[0], return_counts=True))}}
            bb.close()
        m["round"] = rounds
        res["models"][name] = m
        c.close()
    res["show"] = show()
    return res


def show():
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_flight_runs.npz"))
    p = replace(sp.base_prob_scaled, **FLYABLE)
    c = IntegratorCache(p, npts=10)
    worst = lambda rep: np.max([rep.G_TMIN.max(axis=1), rep.G_TILT.max(axis=1)], axis=0).tolist()   # noqa: E731
    out = {}
    for restart in ("replan", "guess"):
        b = ScvxBatch(c, 2).init(g["ic"])
        st0 = b.solve()[0]
        base = b.audit()
        m0 = b.trajectory()[0][:, -1, 0]
        st, it, nu, dj, rep, used = b.harden(("thrust", "tilt"), rounds=6, restart=restart)
        out[restart] = {"status_before": st0.tolist(), "status": st.tolist(), "rounds_used": used, "last_solve_steps": it.tolist(),
                        "mass_before": m0.tolist(), "mass_after": b.trajectory()[0][:, -1, 0].tolist(), "worst_before": worst(base),
                        "worst_after": worst(rep), "violating_segments_before": [int((base.G_TMIN[t] > 1e-7).sum() + (base.G_TILT[t] > 1e-7).sum())
                                                                                 for t in range(2)]}
        b.close()
    c.close()
    return out


def markdown(r):
    f = lambda v: "%.4f (%.4f .. %.4f)" % tuple(v)   # noqa: E731
    lines = ["## Timings\n", "%s, K = 50, nsub = 10; kernel times in ms per launch by HIP events, %d launches per window, %d alternating windows, "
             "median (min .. max).\n" % (r["device"], r["launches"], r["repeats"]),
             "| model | B | audit | audit + report | flight check (PLAN) | K2 | audit / K2 | audit / flight check |", "|---|---|---|---|---|---|---|---|"]
    for name, m in r["models"].items():
        for B, k in m["kernels"].items():
            lines.append("| %s | %s | %s | %s | %s | %s | %.2f | %.3f |" % (name, B, f(k["audit"]), f(k["audit_report"]), f(k["flight_plan"]),
                                                                          f(k["k2"]), k["audit"][0] / k["k2"][0], k["audit"][0] / k["flight_plan"][0]))
    lines += ["\nOne round on converged plans, wall ms:\n", "| model | harden((\"thrust\", \"tilt\")) | robustify(constraints=(\"thrust\", \"tilt\")) |",
              "|---|---|---|"]
    for name, m in r["models"].items():
        h, rb = m["round"]["harden"], m["round"]["robustify"]
        lines.append("| %s | %.1f (%d converged, %d before; statuses %s; steps %s) | %.1f (%d converged, %d before; statuses %s; steps %s) |" % (
            name, h["ms"], h["converged"], h["converged_before"], h["status"], h["steps"], rb["ms"], rb["converged"], rb["converged_before"],
            rb["status"], rb["steps"]))
    lines += ["\n## Hardening on the two golden starts (the device's)\n", "```", json.dumps(r["show"], indent=1), "```"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", default="1,256,8192")
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
