"""Cost of the flight check (scvx_flight_check_f64) at the headline size, next to what it checks.

    python tools/bench_flight.py [--B 8192] [--nsub 10] [--launches 20] [--md profiles/flight_check.md]

For exo / aero / aero+fins / aero+fins+torque: a dispersed batch (seed 20261004) is stepped `--plan-steps` times to get physical plans,
then SHOOT and PLAN, with and without the dense output xfly, are timed with HIP events around `--launches` launches each after a warm-up,
and in the same process K2 (scvx_propagate_f64) on the same arrays.  For exo also one headline solve_step (mean over one solve_problem
period of 14 steps from create_initial, as bench.py times it).  One JSON line on stdout; --md also writes the table.
Condition stated with the feature: SHOOT with xfly costs less than one solve_step of the same batch in the same run."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--nsub", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.defns import AtmosphericData
    from successiveconvexification_amd.dynamics import IntegratorCache
    z = np.load(os.path.join(ROOT, "tests", "golden", "lift_drag_tables.npz"))
    aero = AtmosphericData(z["drag"], z["lift"], z["torque"])
    models = {"exo": sp.base_prob_scaled, "aero": sp.base_prob_aero_scaled(aero), "aero+fins": sp.base_prob_fin_scaled(aero),
              "aero+fins+torque": sp.base_prob_fin_scaled(aero, torque=True)}
    B = a.B
    ts = torch.cuda.Stream()   # torch's events see kernels on a torch stream: the context runs on one for this tool
    res = {"B": B, "nsub": a.nsub, "launches": a.launches, "device": torch.cuda.get_device_name(0), "models": {}}

    def timed(call, n):
        for _ in range(a.warmup):
            assert call() == 0
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(n):
            call()
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n

    for name, p in models.items():
        K = p.K
        c = IntegratorCache(p, npts=10)
        c.set_stream(ts.cuda_stream)
        b = ScvxBatch(c, B).init(mc.disperse_ics(p, 0, B, a.seed))
        L, out = c._L, {}
        if name == "exo":   # the headline solve_step: one solve_problem period from create_initial, after two warm-up steps
            for _ in range(2):
                b.solve_step_async()
            b.reset()
            c.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(ts)
            for _ in range(p.imax - 1):
                b.solve_step_async()
            t1.record(ts)
            torch.cuda.synchronize()
            out["solve_step_ms"] = t0.elapsed_time(t1) / (p.imax - 1)
            b.reset()
        for _ in range(a.plan_steps):
            b.solve_step_async()
        x, u, s = b.trajectory()
        xd, ud, sd = (torch.tensor(np.ascontiguousarray(v), device="cuda") for v in (x, u, s))
        rep = torch.empty((B, _lib.FLIGHT_NREP), dtype=torch.float64, device="cuda")
        xf = torch.empty((B, K + 1, 14), dtype=torch.float64, device="cuda")
        xn = torch.empty((B, K, 14), dtype=torch.float64, device="cuda")
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        for mode, mname in ((_lib.FLIGHT_SHOOT, "shoot"), (_lib.FLIGHT_PLAN, "plan")):
            for dense in (False, True):
                out["%s%s_ms" % (mname, "_xfly" if dense else "")] = timed(
                    lambda: L.scvx_flight_check_f64(c.handle, B, K, vp(xd), vp(ud), vp(sd), a.nsub, mode, vp(rep), vp(xf) if dense else None),
                    a.launches)
        c.set_npts(a.nsub)
        out["k2_propagate_ms"] = timed(lambda: L.scvx_propagate_f64(c.handle, B, K, vp(xd), vp(ud), vp(sd), C.c_double(1.0 / (K + 1)), vp(xn)),
                                       a.launches)
        r = rep.cpu().numpy()
        out["plan_gap_max"] = float(np.nanmax(r[:, 0]))
        res["models"][name] = out
        c.set_stream(None)
        b.close()
        c.close()
    step = res["models"]["exo"]["solve_step_ms"]
    res["condition_shoot_xfly_lt_solve_step"] = bool(res["models"]["exo"]["shoot_xfly_ms"] < step)
    print(json.dumps(res))
    if a.md:
        cols = ("shoot_ms", "shoot_xfly_ms", "plan_ms", "plan_xfly_ms", "k2_propagate_ms")
        with open(a.md, "w") as f:
            f.write("# Flight check: device time at B = %d, K = 50, nsub = %d\n\n" % (B, a.nsub))
            f.write("`python tools/bench_flight.py`; %s; HIP events around %d launches after %d warm-up launches; fp64.\n\n"
                    % (res["device"], a.launches, a.warmup))
            f.write("| model | SHOOT ms | SHOOT + xfly ms | PLAN ms | PLAN + xfly ms | K2 propagate ms |\n|---|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s |\n" % (name, " | ".join("%.3f" % o[k] for k in cols)))
            f.write("\nHeadline solve_step of the same exo batch in the same run: %.2f ms per step.  SHOOT with xfly costs %.3f ms: "
                    "condition (less than one solve_step) %s.\n" % (step, res["models"]["exo"]["shoot_xfly_ms"],
                                                                     "holds" if res["condition_shoot_xfly_lt_solve_step"] else "DOES NOT hold"))


if __name__ == "__main__":
    main()
