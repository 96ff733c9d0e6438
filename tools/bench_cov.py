"""Cost of the covariance analysis (scvx_cov_propagate_f64) at the headline size, next to what it builds on.

    python tools/bench_cov.py [--B 8192] [--launches 20] [--repeats 5] [--md profiles/cov.md]

For exo / aero / aero+fins / aero+fins+torque: a dispersed batch (seed 20261004) is stepped `--plan-steps` times to get physical plans;
then, in the same process and on the same arrays, K1 (scvx_linearize_f64, which writes the derivative tiles), the gains kernel on those
tiles, the covariance launch without and with each dense output (both forms of its n-deep products, alternating windows) and a plain
device-to-device copy of the tile buffer are timed with HIP events: `--repeats` windows of `--launches` launches each after a
warm-up, reported as median (min .. max) of the windows.  The covariance kernel's read rate is the bytes of the tile buffer and the
gains over its time, next to the rate at which the copy reads the tile buffer.  Float tiles exist only inside a batch
(scvx_batch_set_linearization_f32), so they are timed through scvx_batch_cov, host wall clock of the whole call (gains launch, covariance
launch, copies of S0 in and the report out), fp64 and float tiles alternating.  One JSON line on stdout; --md also writes the tables.
Condition stated with the feature: the covariance launch without dense outputs takes less time than the K1 launch that produced its
tiles (exo, npts = 10)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
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
    res = {"B": B, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "models": {}}
    stat = lambda w: [float(np.median(w)), float(min(w)), float(max(w))]   # noqa: E731

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(a.launches):
            call()
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def timed(call):
        """[median, min, max] ms per launch over the windows"""
        for _ in range(a.warmup):
            rc = call()
            assert rc is None or rc == 0, rc
        return stat([window(call) for _ in range(a.repeats)])

    for name in a.models.split(","):
        p = models[name]()
        K = p.K
        c = IntegratorCache(p, npts=10)
        c.set_stream(ts.cuda_stream)
        b = ScvxBatch(c, B).init(mc.disperse_ics(p, 0, B, a.seed))
        L, h, out = c._L, c.handle, {}
        nu = c.nu
        n = 14 + nu
        for _ in range(a.plan_steps):
            b.solve_step_async()
        x, u, s = b.trajectory()
        sdv = np.zeros(14)
        sdv[1:7] = 1e-3 * np.abs(x[:, 0, 1:7]).max(axis=0)
        sdv[7:] = 1e-3
        S0 = np.ascontiguousarray(np.broadcast_to(np.diag(sdv * sdv), (B, 14, 14)))
        # float tiles against fp64 tiles through the batch-level call (host wall clock of the whole call), alternating
        wall = {0: [], 1: []}
        for rnd in range(a.repeats + 1):
            for f32 in (0, 1):
                b.set_linearization_f32(bool(f32))
                c.synchronize()
                t0 = time.perf_counter()
                b.covariance(S0)
                if rnd:
                    wall[f32].append((time.perf_counter() - t0) * 1e3)
        b.set_linearization_f32(False)
        out["batch_cov_f64_tiles_wall_ms"], out["batch_cov_f32_tiles_wall_ms"] = stat(wall[0]), stat(wall[1])
        b.close()   # its buffers are not needed any more: the tile buffers below are large
        xd, ud, sd, s0d = (torch.tensor(np.ascontiguousarray(v), device="cuda") for v in (x, u, s, S0))
        f64 = dict(dtype=torch.float64, device="cuda")
        ep = torch.empty((B, K, 14), **f64)
        dv = torch.empty((B, K, c.np, 14), **f64)
        dv2 = torch.empty_like(dv)
        gain = torch.empty((B, K, nu, n), **f64)
        rep = torch.empty((B, _lib.COV_NREP), **f64)
        sig = torch.empty((B, K + 1, n), **f64)
        covK = torch.empty((B, n, n), **f64)
        cov = torch.empty((B, K + 1, n, n), **f64)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        q, r, qf = np.ones(14), np.ones(nu), np.full(14, 100.0)
        dt = C.c_double(1.0 / (K + 1))
        out["k1_linearize_ms"] = timed(lambda: L.scvx_linearize_f64(h, B, K, vp(xd), vp(ud), vp(sd), dt, vp(ep), vp(dv)))
        out["gains_ms"] = timed(lambda: L.scvx_track_gains_f64(h, B, K, vp(dv), dp(q), dp(r), dp(qf), vp(gain), None))

        def covcall(s_=None, k_=None, c_=None):
            return lambda: L.scvx_cov_propagate_f64(h, B, K, vp(xd), vp(ud), vp(dv), vp(gain), vp(s0d), None, vp(rep),
                                                    None if s_ is None else vp(s_), None if k_ is None else vp(k_),
                                                    None if c_ is None else vp(c_))

        out["cov_ms"] = timed(covcall())
        out["cov_sig_ms"] = timed(covcall(s_=sig))
        out["cov_covK_ms"] = timed(covcall(k_=covK))
        out["cov_cov_ms"] = timed(covcall(c_=cov))
        out["cov_all_ms"] = timed(covcall(sig, covK, cov))
        # A/B of the two forms of the n-deep products (SCVX_COV_MFMA, read at every launch): alternating windows, and the largest
        # difference between their final covariances
        ab, keep = {"0": [], "1": []}, {}
        for v in ("0", "1"):
            os.environ["SCVX_COV_MFMA"] = v
            for _ in range(a.warmup):
                assert covcall(k_=covK)() == 0
            torch.cuda.synchronize()
            keep[v] = covK.clone()
        for _ in range(a.repeats):
            for v in ("0", "1"):
                os.environ["SCVX_COV_MFMA"] = v
                ab[v].append(window(covcall()))
        del os.environ["SCVX_COV_MFMA"]
        out["cov_lanes_ms"], out["cov_mfma_ms"] = stat(ab["0"]), stat(ab["1"])
        fin = torch.isfinite(keep["0"]).all(dim=2).all(dim=1) & torch.isfinite(keep["1"]).all(dim=2).all(dim=1)
        out["finite_rows"] = int(fin.sum())
        out["cov_ab_max_rel_diff"] = float(((keep["0"][fin] - keep["1"][fin]).abs().amax(dim=(1, 2)) / keep["0"][fin].abs().amax(dim=(1, 2))).max())
        del keep

        def copy_tiles():
            dv2.copy_(dv)

        with torch.cuda.stream(ts):
            out["copy_tiles_ms"] = timed(copy_tiles)
        out["tile_bytes"] = dv.numel() * 8
        out["cov_read_bytes"] = (dv.numel() - B * K * 14 + gain.numel()) * 8   # the Sigma column of a tile is not read
        out["cov_read_GBps"] = out["cov_read_bytes"] / out["cov_ms"][0] / 1e6
        out["gains_read_GBps"] = out["tile_bytes"] / out["gains_ms"][0] / 1e6
        out["copy_read_GBps"] = out["tile_bytes"] / out["copy_tiles_ms"][0] / 1e6
        out["cov_over_gains"] = out["cov_ms"][0] / out["gains_ms"][0]
        res["models"][name] = out
        del ep, dv, dv2, gain, rep, sig, covK, cov
        torch.cuda.empty_cache()
        c.set_stream(None)
        c.close()
    if "exo" in res["models"]:
        e = res["models"]["exo"]
        res["condition_cov_lt_k1"] = bool(e["cov_ms"][0] < e["k1_linearize_ms"][0])
    print(json.dumps(res))
    if a.md:
        fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
        with open(a.md, "w") as f:
            f.write("# Covariance analysis: device time at B = %d, K = 50\n\n" % B)
            f.write("`python tools/bench_cov.py`; %s; HIP events; per entry %d windows of %d launches after %d warm-up launches, "
                    "median (min .. max) of the windows in ms; fp64 tiles; gains of the weights q = 1, r = 1, qf = 100; S0 at 1e-3; w = 0.\n\n"
                    % (res["device"], a.repeats, a.launches, a.warmup))
            f.write("| model | K1 linearize | gains | covariance | cov / gains | copy of the tiles | cov read GB/s | gains read GB/s | copy read GB/s |\n"
                    "|---|---|---|---|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s | %s | %s | %.2f | %s | %.0f | %.0f | %.0f |\n"
                        % (name, fmt(o["k1_linearize_ms"]), fmt(o["gains_ms"]), fmt(o["cov_ms"]), o["cov_over_gains"], fmt(o["copy_tiles_ms"]),
                           o["cov_read_GBps"], o["gains_read_GBps"], o["copy_read_GBps"]))
            f.write("\nThe dense outputs (sig [B][K+1][n], covK [B][n][n], cov [B][K+1][n][n]):\n\n"
                    "| model | report only | + sig | + covK | + cov | + all three |\n|---|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s | %s | %s | %s | %s |\n" % (name, fmt(o["cov_ms"]), fmt(o["cov_sig_ms"]), fmt(o["cov_covK_ms"]),
                                                            fmt(o["cov_cov_ms"]), fmt(o["cov_all_ms"])))
            f.write("\nThe two forms of the n-deep products V = M Sigma and T = V M', alternating windows in the same run (`SCVX_COV_MFMA=0 / 1`; "
                    "`covariance` above is the default form), report only:\n\n"
                    "| model | one lane per element | 16 x 16 corner on v_mfma_f64_16x16x4 | largest relative difference of Sigma_K | rows with a finite Sigma_K |\n"
                    "|---|---|---|---|---|\n")
            for name, o in res["models"].items():
                f.write("| %s | %s | %s | %.3e | %d |\n" % (name, fmt(o["cov_lanes_ms"]), fmt(o["cov_mfma_ms"]), o["cov_ab_max_rel_diff"],
                                                          o["finite_rows"]))
            f.write("\nFloat tiles exist only inside a batch: scvx_batch_cov, host wall clock of the whole call (gains launch, covariance launch, "
                    "S0 in, report out), %d calls alternating after one warm-up each:\n\n| model | fp64 tiles | float tiles |\n|---|---|---|\n" % a.repeats)
            for name, o in res["models"].items():
                f.write("| %s | %s | %s |\n" % (name, fmt(o["batch_cov_f64_tiles_wall_ms"]), fmt(o["batch_cov_f32_tiles_wall_ms"])))
            if "exo" in res["models"]:
                e = res["models"]["exo"]
                f.write("\nThe tile buffer is %.3f GB (exo).  Condition (the covariance launch without dense outputs takes less time than the K1 "
                        "launch that produced its tiles, exo, npts = 10): %.3f ms against %.3f ms: %s.\n"
                        % (e["tile_bytes"] / 1e9, e["cov_ms"][0], e["k1_linearize_ms"][0], "holds" if res["condition_cov_lt_k1"] else "DOES NOT hold"))


if __name__ == "__main__":
    main()
