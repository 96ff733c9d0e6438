"""Cost of the clamp-aware covariance launch (scvx_cov_clamp_f64) beside the plain one (scvx_cov_propagate_f64), measured in the same
run, and what the analysis shows on the golden plans.

    python tools/bench_cov_clamp.py [--plans 8192] [--launches 10] [--repeats 5] [--json out.json] [--md profiles/cov_clamp.md]

Timing: the flyable problem on the exo and the aero + fins model, K = 50, `--plans` plans after `--plan-steps` solve_steps, both forms
of the n-deep products (SCVX_COV_MFMA = 0 / 1, read at every launch).  Kernel times by HIP events in alternating windows of one run,
median (min .. max) per launch, report only (no dense outputs) on both sides.
Expectation stated with the feature, not a bar, and not measured before this tool existed: below +40 % -- the step gains one n-deep
matrix-vector pass, NU + 3 n-deep dot products, two erfc, two exp and two barriers, where the VEH form's extra n^2 pass and two barriers
cost +34 % / +46 %.  The tool prints whether it held.

Show: the two golden plans of tests/golden/oracle_flight_runs.npz under the device's gains, cov_reference.handover_s0's handover at
scales 0.1, 0.3 and 1: SIG_R / SIG_V of the plain call, and SIG, BIAS, RMS, P_LO, P_HI, GAIN_MIN of the clamp-aware one."""
import argparse
import ctypes as C
import json
import os
import sys
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from bench_mc import FLYABLE   # noqa: E402

EXPECTED = 1.40
MARKER = "<!-- tools/bench_cov_clamp.py rewrites everything below this line -->"


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

    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
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
        b.close()
        L, h = c._L, c.handle
        sd = np.zeros(14)
        sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
        sd[7:] = 1e-3
        S0 = np.broadcast_to(np.diag(sd * sd), (B, 14, 14))
        dx, du, dd, dg, d0 = (dev(v) for v in (x, u, deriv, gain, S0))
        rep, srep = torch.empty(B, 16, **f64), torch.empty(B, 16, **f64)
        head = (h, B, K, vp(dx), vp(du), vp(dd), vp(dg), vp(d0), None)

        def form(mf, call):
            def go():
                os.environ["SCVX_COV_MFMA"] = mf
                return call()
            return go
        plain = lambda: L.scvx_cov_propagate_f64(*head, vp(rep), None, None, None)                         # noqa: E731
        clamp = lambda: L.scvx_cov_clamp_f64(*head, None, vp(rep), vp(srep), None, None, None, None, None)   # noqa: E731
        m = timed({"plain_mf0": form("0", plain), "clamp_mf0": form("0", clamp), "plain_mf1": form("1", plain), "clamp_mf1": form("1", clamp)})
        del os.environ["SCVX_COV_MFMA"]
        sr = srep.cpu().numpy()
        fin = np.isfinite(sr).all(axis=1)
        m["finite_rows"] = int(fin.sum())
        m["median_P_LO"], m["median_GAIN_MIN"] = float(np.median(sr[fin, 12])), float(np.median(sr[fin, 14]))
        res["models"][name] = m
        c.close()
    res["show"] = show()
    return res


def show():
    import cov_reference as cr
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.dynamics import IntegratorCache, cov_propagate_batch, linearize_batch, track_gains_batch
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_flight_runs.npz"))
    p = replace(sp.base_prob_scaled, **FLYABLE)
    x, u, s = g["x"], g["u"], g["sigma"]
    c = IntegratorCache(p, npts=10)
    _, d = linearize_batch(c, x, u, s, 1.0 / (p.K + 1))
    L = track_gains_batch(c, d)
    out = {}
    for scale in (0.1, 0.3, 1.0):
        S0 = np.stack([cr.handover_s0(x[b, 0], scale=scale)[0] for b in range(2)])
        lin, sat = cov_propagate_batch(c, x, u, d, L, S0), cov_propagate_batch(c, x, u, d, L, S0, clamp=True)
        row = {"LIN_SIG_R": lin.SIG_R.tolist(), "LIN_SIG_V": lin.SIG_V.tolist()}
        row.update({k: getattr(sat, k).tolist() for k in ("SIG_R", "SIG_V", "BIAS_R", "BIAS_V", "RMS_R", "RMS_V", "P_LO", "P_HI", "GAIN_MIN")})
        out["scale %.1f" % scale] = row
    c.close()
    return out


def markdown(r):
    f = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    lines = ["## Timings\n", "%s, %d plans, K = 50; kernel times in ms per launch by HIP events, %d launches per window, %d alternating windows, "
             "median (min .. max); the report alone on both sides.\n" % (r["device"], r["plans"], r["launches"], r["repeats"]),
             "| model | SCVX_COV_MFMA | plain | clamp-aware | ratio | expectation (below %.2f) |" % EXPECTED, "|---|---|---|---|---|---|"]
    for name, m in r["models"].items():
        for mf in ("0", "1"):
            a, b = m["plain_mf" + mf], m["clamp_mf" + mf]
            lines.append("| %s | %s | %s | %s | %.2f | %s |" % (name, mf, f(a), f(b), b[0] / a[0], "held" if b[0] / a[0] < EXPECTED else "did NOT hold"))
    lines += ["", "Rows with a finite satrep, their median P_LO and GAIN_MIN: " + "; ".join(
        "%s %d, %.3f, %.3f" % (n, m["finite_rows"], m["median_P_LO"], m["median_GAIN_MIN"]) for n, m in r["models"].items()),
        "\n## What the analysis shows on the two golden plans (the device's gains)\n",
        "LIN_*: scvx_cov_propagate_f64; the others: scvx_cov_clamp_f64 with the problem's band; per plan.\n", "```", json.dumps(r["show"], indent=1), "```"]
    return "\n".join(lines) + "\n"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=8192)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--models", default="exo,aero+fins")
    ap.add_argument("--json")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "cov_clamp.md"))
    a = ap.parse_args()
    r = measure(a)
    if a.json:
        json.dump(r, open(a.json, "w"), indent=1)
    md = markdown(r)
    # profiles/cov_clamp.md keeps what stands above its marker line (resources, parity, the reading of the timings)
    old = open(a.md).read() if os.path.exists(a.md) else ""
    keep = old[:old.index(MARKER) + len(MARKER)] + "\n" if MARKER in old else ""
    open(a.md, "w").write(keep + md)
    print(md)
