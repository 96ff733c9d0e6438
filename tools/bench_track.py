"""Cost of plan tracking (scvx_track_gains_f64, scvx_track_fly_f64) at the headline size, next to what it builds on.

    python tools/bench_track.py [--B 8192] [--nsub 10] [--launches 20] [--repeats 5] [--md profiles/track.md]

For exo / aero / aero+fins / aero+fins+torque: a dispersed batch (seed 20261004) is stepped `--plan-steps` times to get physical plans;
then, in the same process and on the same arrays, K1 (scvx_linearize_f64, which writes the derivative tiles), the gains kernel on those
tiles (both forms of its 14-deep products, alternating), the closed-loop flight with and without the dense outputs, the SHOOT flight
check, K2 and a plain device-to-device copy of the tile buffer are timed with HIP events: `--repeats` windows of `--launches` launches
each after a warm-up, reported as median (min .. max) of the windows.  For exo also one headline solve_step (mean over one
solve_problem period from create_initial, as bench.py times it).  The gains kernel's read rate is the bytes of the tile buffer over
its time, next to the rate at which the copy reads the same buffer.  One JSON line on stdout; --md also writes the tables.
Condition stated with the feature: the gains launch takes less time than the K1 launch that produced its tiles (exo, npts = 10)."""
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
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--models", default="exo,aero,aero+fins,aero+fins+torque")
    ap.add_argument("--md", default=None)
    a = ap.parse_args()
    import torch
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.defns import AtmosphericData
    from successiveconvexification_amd.dynamics import IntegratorCache
    z = np.load(os.path.join(ROOT, "tests", "golden", "lift_drag_tables.npz"))
    aero = AtmosphericData(z["drag"], z["lift"], z["torque"])
    models = {"exo": lambda: sp.base_prob_scaled, "aero": lambda: sp.base_prob_aero_scaled(aero),
              "aero+fins": lambda: sp.base_prob_fin_scaled(aero), "aero+fins+torque": lambda: sp.base_prob_fin_scaled(aero, torque=True)}
    B = a.B
    ts = torch.cuda.Stream()   # torch's events see kernels on a torch stream: the context runs on one for this tool
    res = {"B": B, "nsub": a.nsub, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "models": {}}

    def timed(call):
        """[median, min, max] ms per launch over the windows"""
        for _ in range(a.warmup):
            rc = call()
            assert rc is None or rc == 0, rc
        w = []
        for _ in range(a.repeats):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(ts)
            for _ in range(a.launches):
                call()
            t1.record(ts)
            torch.cuda.synchronize()
            w.append(t0.elapsed_time(t1) / a.launches)
        return [float(np.median(w)), float(min(w)), float(max(w))]

    for name in a.models.split(","):
        p = models[name]()
        K = p.K
        c = IntegratorCache(p, npts=10)
        c.set_stream(ts.cuda_stream)
        b = ScvxBatch(c, B).init(mc.disperse_ics(p, 0, B, a.seed))
        L, h, out = c._L, c.handle, {}
        nu = c.nu
        n = 14 + nu
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
        b.close()   # its buffers are not needed any more: the tile buffers below are large
        dx0 = mc.disperse_handover(x[:, 0], 0, B, a.seed, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
        xd, ud, sd, d0 = (torch.tensor(np.ascontiguousarray(v), device="cuda") for v in (x, u, s, dx0))
        f64 = dict(dtype=torch.float64, device="cuda")
        ep = torch.empty((B, K, 14), **f64)
        dv = torch.empty((B, K, c.np, 14), **f64)
        dv2 = torch.empty_like(dv)
        gain = torch.empty((B, K, nu, n), **f64)
        p0 = torch.empty((B, n, n), **f64)
        rep = torch.empty((B, _lib.FLIGHT_NREP), **f64)
        xf = torch.empty((B, K + 1, 14), **f64)
        uf = torch.empty((B, K + 1, nu), **f64)
        xn = torch.empty((B, K, 14), **f64)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        q, r, qf = np.ones(14), np.ones(nu), np.full(14, 100.0)
        dt = C.c_double(1.0 / (K + 1))
        c.set_npts(10)
        out["k1_linearize_ms"] = timed(lambda: L.scvx_linearize_f64(h, B, K, vp(xd), vp(ud), vp(sd), dt, vp(ep), vp(dv)))
        gains = lambda: L.scvx_track_gains_f64(h, B, K, vp(dv), dp(q), dp(r), dp(qf), vp(gain), None)   # noqa: E731
        out["gains_ms"] = timed(gains)
        out["gains_p0_ms"] = timed(lambda: L.scvx_track_gains_f64(h, B, K, vp(dv), dp(q), dp(r), dp(qf), vp(gain), vp(p0)))
        # A/B of the two forms of the 14-deep products (SCVX_TRACK_MFMA, read at every launch): alternating windows, and the
        # largest difference between their gains
        ab, keep = {"0": [], "1": []}, {}
        for v in ("0", "1"):
            os.environ["SCVX_TRACK_MFMA"] = v
            for _ in range(a.warmup):
                assert gains() == 0
            torch.cuda.synchronize()
            keep[v] = gain.clone()
        for _ in range(a.repeats):
            for v in ("0", "1"):
                os.environ["SCVX_TRACK_MFMA"] = v
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(ts)
                for _ in range(a.launches):
                    gains()
                t1.record(ts)
                torch.cuda.synchronize()
                ab[v].append(t0.elapsed_time(t1) / a.launches)
        del os.environ["SCVX_TRACK_MFMA"]
        out["gains_lanes_ms"] = [float(np.median(ab["0"])), float(min(ab["0"])), float(max(ab["0"]))]
        out["gains_mfma_ms"] = [float(np.median(ab["1"])), float(min(ab["1"])), float(max(ab["1"]))]
        out["gains_ab_max_diff"] = float((keep["0"] - keep["1"]).abs().max())
        out["gains_max_abs"] = float(keep["0"].abs().max())
        del keep

        def copy_tiles():
            dv2.copy_(dv)

        with torch.cuda.stream(ts):
            out["copy_tiles_ms"] = timed(copy_tiles)
        nbytes = dv.numel() * 8
        out["tile_bytes"] = nbytes
        out["gains_read_GBps"] = nbytes / out["gains_ms"][0] / 1e6
        out["copy_read_GBps"] = nbytes / out["copy_tiles_ms"][0] / 1e6
        for dense in (False, True):
            for clamp in (0, _lib.TRACK_CLAMP):
                out["fly%s%s_ms" % ("_clamp" if clamp else "", "_dense" if dense else "")] = timed(
                    lambda: L.scvx_track_fly_f64(h, B, K, vp(xd), vp(ud), vp(sd), vp(gain), vp(d0), a.nsub, clamp, vp(rep),
                                                 vp(xf) if dense else None, vp(uf) if dense else None))
        r_ = rep.cpu().numpy()
        out["closed_loop_finite_rows"] = int(np.isfinite(r_[:, :13]).all(axis=1).sum())
        out["shoot_xfly_ms"] = timed(lambda: L.scvx_flight_check_f64(h, B, K, vp(xd), vp(ud), vp(sd), a.nsub, _lib.FLIGHT_SHOOT, vp(rep), vp(xf)))
        c.set_npts(a.nsub)
        out["k2_propagate_ms"] = timed(lambda: L.scvx_propagate_f64(h, B, K, vp(xd), vp(ud), vp(sd), dt, vp(xn)))
        out["fly_over_shoot"] = out["fly_dense_ms"][0] / out["shoot_xfly_ms"][0]
        res["models"][name] = out
        del ep, dv, dv2, gain, p0, rep, xf, uf, xn
        torch.cuda.empty_cache()
        c.set_stream(None)
        c.close()
    if "exo" in res["models"]:
        e = res["models"]["exo"]
        res["condition_gains_lt_k1"] = bool(e["gains_ms"][0] < e["k1_linearize_ms"][0])
    print(json.dumps(res))
    if a.md:
        fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
        with open(a.md, "w") as f:
            f.write("# Plan tracking: device time at B = %d, K = 50, nsub = %d\n\n" % (B, a.nsub))
            f.write("`python tools/bench_track.py`; %s; HIP events; per entry %d windows of %d launches after %d warm-up launches, "
                    "median (min .. max) of the windows in ms; fp64; weights q = 1, r = 1, qf = 100; dx0 at 1e-3.\n\n"
                    % (res["device"], a.repeats, a.launches, a.warmup))
            f.write("| model | K1 linearize | gains | gains + P0 | copy of the tiles | gains read GB/s | copy read GB/s |\n|---|---|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s | %s | %s | %s | %.0f | %.0f |\n" % (name, fmt(o["k1_linearize_ms"]), fmt(o["gains_ms"]), fmt(o["gains_p0_ms"]),
                                                                     fmt(o["copy_tiles_ms"]), o["gains_read_GBps"], o["copy_read_GBps"]))
            f.write("\n| model | track_fly | + clamp | + xfly, ufly | + clamp + xfly, ufly | SHOOT + xfly | K2 propagate | fly / SHOOT |\n|---|---|---|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s | %s | %s | %s | %s | %s | %.2f |\n" % (name, fmt(o["fly_ms"]), fmt(o["fly_clamp_ms"]), fmt(o["fly_dense_ms"]),
                                                                         fmt(o["fly_clamp_dense_ms"]), fmt(o["shoot_xfly_ms"]),
                                                                         fmt(o["k2_propagate_ms"]), o["fly_over_shoot"]))
            f.write("\nThe two forms of the 14-deep products W = Pxx D and T = D' W in the gains kernel, alternating windows in the same run "
                    "(`SCVX_TRACK_MFMA=0 / 1`; `gains` above is the default form):\n\n"
                    "| model | one lane per element | v_mfma_f64_16x16x4 tiles | largest difference of the gains | max abs gain |\n|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s | %s | %.3e | %.4g |\n" % (name, fmt(o["gains_lanes_ms"]), fmt(o["gains_mfma_ms"]), o["gains_ab_max_diff"],
                                                            o["gains_max_abs"]))
            if "exo" in res["models"]:
                e = res["models"]["exo"]
                f.write("\nThe tile buffer is %.3f GB (exo).  Headline solve_step of the same exo batch in the same run: %.2f ms per step.  "
                        "Condition (the gains launch takes less time than the K1 launch that produced its tiles, exo, npts = 10): "
                        "%.3f ms against %.3f ms: %s.\n" % (e["tile_bytes"] / 1e9, e["solve_step_ms"], e["gains_ms"][0], e["k1_linearize_ms"][0],
                                                            "holds" if res["condition_gains_lt_k1"] else "DOES NOT hold"))


if __name__ == "__main__":
    main()
