"""Cost of the navigation-error covariance analysis (scvx_nav_cov_f64) and of the flight on an estimate (scvx_track_fly_nav_f64) at the
headline size, next to what they build on.

    python tools/bench_nav.py [--B 8192] [--launches 20] [--repeats 5] [--md profiles/nav.md]
                              [--track-json PARENT.json THIS.json] [--build-logs PARENT.log THIS.log]

For exo and aero+fins: a dispersed batch (seed 20261004) is stepped `--plan-steps` times to get physical plans; then, in the same
process and on the same arrays, K1 (scvx_linearize_f64, which writes the derivative tiles), the gains kernel on those tiles, the
covariance launch, the navigation launch (m = 6: position and velocity measured; also m = 0 and m = 14, and with each dense output),
the closed-loop flight and the flight on an estimate are timed with HIP events: `--repeats` windows of `--launches` launches each
after a warm-up, reported as median (min .. max) of the windows.  The two flights alternate window by window.  Then the two golden
plans of tests/golden/oracle_flight_runs.npz with the inputs of tests/test_nav_cpu.py: the landing 1 sigma with and without the
navigation term.  One JSON line on stdout; --md also writes the tables.

--track-json: two outputs of tools/bench_track.py, of the parent commit and of this one from the same session: the figures of
scvx_track_fly_f64 side by side (the old path must not have moved).  --build-logs: two outputs of build.build(force=True,
verbose=True): the register figures of every fly_kernel instantiation side by side."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FIGS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]",
        "LDS Size [bytes/block]")


def resource_figures(path, pattern):
    """{demangled kernel name: {figure: value}} from the -Rpass-analysis=kernel-resource-usage remarks of a build log"""
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = None
            if re.search(pattern, m.group(1)):
                cur = subprocess.check_output(["c++filt", m.group(1)], text=True).strip().split("(")[0].replace("void scvx::", "")
                out[cur] = {}
            continue
        m = re.search(r"remark:\s+(.+?): (\d+) \[-Rpass", line)
        if m and cur and m.group(1) in FIGS:
            out[cur][m.group(1)] = int(m.group(2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--nsub", type=int, default=10)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--models", default="exo,aero+fins")
    ap.add_argument("--md", default=None)
    ap.add_argument("--track-json", nargs=2, default=None, metavar=("PARENT", "THIS"))
    ap.add_argument("--build-logs", nargs=2, default=None, metavar=("PARENT", "THIS"))
    ap.add_argument("--no-device", action="store_true", help="write only the sections that need no device (--build-logs, --track-json)")
    a = ap.parse_args()
    report(a, {"B": a.B, "models": {}} if a.no_device else device_figures(a))


def device_figures(a):
    """the timings and the golden-plan figures: needs the device"""
    import torch
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.defns import AtmosphericData
    from successiveconvexification_amd.dynamics import (IntegratorCache, cov_propagate_batch, linearize_batch, nav_cov_batch,
                                                          track_gains_batch)
    z = np.load(os.path.join(ROOT, "tests", "golden", "lift_drag_tables.npz"))
    aero = AtmosphericData(z["drag"], z["lift"], z["torque"])
    models = {"exo": lambda: sp.base_prob_scaled, "aero": lambda: sp.base_prob_aero_scaled(aero),
              "aero+fins": lambda: sp.base_prob_fin_scaled(aero), "aero+fins+torque": lambda: sp.base_prob_fin_scaled(aero, torque=True)}
    B = a.B
    ts = torch.cuda.Stream()   # torch's events see kernels on a torch stream: the context runs on one for this tool
    res = {"B": B, "nsub": a.nsub, "launches": a.launches, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "models": {}}
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
        N = n + 14
        for _ in range(a.plan_steps):
            b.solve_step_async()
        x, u, s = b.trajectory()
        b.close()   # its buffers are not needed any more: the tile buffers below are large
        sdv = np.zeros(14)
        sdv[1:7] = 1e-3 * np.abs(x[:, 0, 1:7]).max(axis=0)
        sdv[7:] = 1e-3
        S0 = np.ascontiguousarray(np.broadcast_to(np.diag(sdv * sdv), (B, 14, 14)))
        N0 = np.ascontiguousarray(0.25 * S0)
        msd = np.full(14, 1e-4)
        msd[1:7] = 3e-2 * sdv[1:7]
        model = {0: (None, None), 6: (np.ascontiguousarray(mc.measurement_rows("rv")), np.ascontiguousarray(msd[1:7] ** 2)),
                 14: (np.ascontiguousarray(np.eye(14)), np.ascontiguousarray(msd ** 2))}
        dx0 = mc.disperse_handover(x[:, 0], 0, B, a.seed, frac_r=1e-3, frac_v=1e-3, rate=1e-3)
        nav = 1e-4 * np.random.default_rng(a.seed).uniform(-1.0, 1.0, (B, K, 14))
        xd, ud, sd, s0d, n0d, d0, navd = (torch.tensor(np.ascontiguousarray(v), device="cuda") for v in (x, u, s, S0, N0, dx0, nav))
        f64 = dict(dtype=torch.float64, device="cuda")
        ep = torch.empty((B, K, 14), **f64)
        dv = torch.empty((B, K, c.np, 14), **f64)
        gain = torch.empty((B, K, nu, n), **f64)
        rep = torch.empty((B, _lib.COV_NREP), **f64)
        navrep = torch.empty((B, _lib.NAV_NREP), **f64)
        sig = torch.empty((B, K + 1, n), **f64)
        navsig = torch.empty((B, K + 1, 14), **f64)
        kf = torch.empty((B, K, 14, 14), **f64)
        joint = torch.empty((B, K + 1, N, N), **f64)
        frep = torch.empty((B, _lib.FLIGHT_NREP), **f64)
        vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
        dp = lambda v: None if v is None else v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
        q, r, qf = np.ones(14), np.ones(nu), np.full(14, 100.0)
        dt = C.c_double(1.0 / (K + 1))
        out["k1_linearize_ms"] = timed(lambda: L.scvx_linearize_f64(h, B, K, vp(xd), vp(ud), vp(sd), dt, vp(ep), vp(dv)))
        out["gains_ms"] = timed(lambda: L.scvx_track_gains_f64(h, B, K, vp(dv), dp(q), dp(r), dp(qf), vp(gain), None))
        out["cov_ms"] = timed(lambda: L.scvx_cov_propagate_f64(h, B, K, vp(xd), vp(ud), vp(dv), vp(gain), vp(s0d), None, vp(rep), None, None, None))

        def navcall(m, s_=None, v_=None, k_=None, j_=None):
            H, rm = model[m]
            opt = lambda t: None if t is None else vp(t)   # noqa: E731
            return lambda: L.scvx_nav_cov_f64(h, B, K, vp(xd), vp(ud), vp(dv), vp(gain), vp(s0d), vp(n0d), m, dp(H), dp(rm), None, vp(rep),
                                              vp(navrep), opt(s_), opt(v_), opt(k_), opt(j_))

        out["nav_m0_ms"] = timed(navcall(0))
        out["nav_ms"] = timed(navcall(6))
        out["nav_m14_ms"] = timed(navcall(14))
        out["nav_sig_ms"] = timed(navcall(6, s_=sig, v_=navsig))
        out["nav_kf_ms"] = timed(navcall(6, k_=kf))
        out["nav_joint_ms"] = timed(navcall(6, j_=joint))
        out["finite_rows"] = int(torch.isfinite(navrep).all(dim=1).sum())
        out["nav_over_cov"] = out["nav_ms"][0] / out["cov_ms"][0]
        # the two flights, alternating window by window
        fly = lambda: L.scvx_track_fly_f64(h, B, K, vp(xd), vp(ud), vp(sd), vp(gain), vp(d0), a.nsub, 0, vp(frep), None, None)   # noqa: E731
        flynav = lambda: L.scvx_track_fly_nav_f64(h, B, K, vp(xd), vp(ud), vp(sd), vp(gain), vp(d0), vp(navd), a.nsub, 0, vp(frep), None,   # noqa: E731
                                                  None)
        for _ in range(a.warmup):
            assert fly() == 0 and flynav() == 0
        w0, w1 = [], []
        for _ in range(a.repeats):
            w0.append(window(fly))
            w1.append(window(flynav))
        out["fly_ms"], out["fly_nav_ms"] = stat(w0), stat(w1)
        res["models"][name] = out
        del ep, dv, gain, rep, navrep, sig, navsig, kf, joint, frep
        torch.cuda.empty_cache()
        c.set_stream(None)
        c.close()

    # what it shows: the two golden plans, inputs of tests/test_nav_cpu.py
    from dataclasses import replace
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_flight_runs.npz"))
    pp = replace(sp.base_prob_scaled, mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    c = IntegratorCache(pp, npts=10)
    x, u, s = g["x"], g["u"], g["sigma"]
    _, d = linearize_batch(c, x, u, s, 1.0 / (pp.K + 1))
    Lg = track_gains_batch(c, d)
    res["golden"] = []
    for b_ in range(2):
        sdg = np.zeros(14)
        sdg[1:7] = 1e-3 * np.abs(x[b_, 0, 1:7])
        sdg[7:] = 1e-3
        Cf = 0.1 * (np.diag(sdg) @ (np.eye(14) + 0.3 * np.random.default_rng(0).standard_normal((14, 14))))
        S0g = Cf @ Cf.T
        msd = np.repeat([3e-5 * np.abs(x[b_, 0, 1:4]).max(), 3e-5 * np.abs(x[b_, 0, 4:7]).max()], 3)
        sl = slice(b_, b_ + 1)
        base = cov_propagate_batch(c, x[sl], u[sl], d[sl], Lg[sl], S0g[None])
        an = nav_cov_batch(c, x[sl], u[sl], d[sl], Lg[sl], S0g[None], 0.25 * S0g[None], mc.measurement_rows("rv"), msd * msd)
        res["golden"].append({"SIG_R_without": float(base.SIG_R[0]), "SIG_R_with": float(an.SIG_R[0]), "NAV_R": float(an.NAV_R[0]),
                              "EST_R": float(an.EST_R[0]), "SIG_V_without": float(base.SIG_V[0]), "SIG_V_with": float(an.SIG_V[0])})
    c.close()
    return res


def report(a, res):
    """one JSON line on stdout and, with --md, the tables"""
    B = res["B"]
    if a.track_json:
        res["track"] = [json.loads(open(f).read().strip().splitlines()[-1]) for f in a.track_json]
    if a.build_logs:
        res["registers"] = [resource_figures(f, "fly_kernel") for f in a.build_logs]
        res["nav_registers"] = resource_figures(a.build_logs[1], "nav_cov_kernel")
    print(json.dumps(res))
    if a.md:
        fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
        with open(a.md, "w") as f:
            f.write("# Navigation-error covariance analysis: device time at B = %d, K = 50\n\n" % B)
            if not res["models"]:
                f.write("Written with `--no-device`: the timing tables and the golden-plan figures of `python tools/bench_nav.py` are not in this "
                        "file; no device figure of the navigation calls has been measured yet.\n")
            else:
                f.write("`python tools/bench_nav.py`; %s; HIP events; per entry %d windows of %d launches after %d warm-up launches, median "
                        "(min .. max) of the windows in ms; fp64 tiles; gains of the weights q = 1, r = 1, qf = 100; S0 at 1e-3, N0 = 0.25 S0; "
                        "m = 6: position and velocity measured at 3e-5; w = 0; report only unless stated.\n\n"
                        % (res["device"], a.repeats, a.launches, a.warmup))
                f.write("| model | K1 linearize | gains | covariance | navigation (m = 6) | nav / cov | m = 0 | m = 14 | rows with finite reports |\n"
                        "|---|---|---|---|---|---|---|---|---|\n")
                for name, o in res["models"].items():
                    f.write("| %s | %s | %s | %s | %s | %.2f | %s | %s | %d |\n"
                            % (name, fmt(o["k1_linearize_ms"]), fmt(o["gains_ms"]), fmt(o["cov_ms"]), fmt(o["nav_ms"]), o["nav_over_cov"],
                               fmt(o["nav_m0_ms"]), fmt(o["nav_m14_ms"]), o["finite_rows"]))
                f.write("\nThe navigation kernel has one form, one lane per output element; there is no matrix-pipe form and no switch.\n")
                f.write("\nThe dense outputs (m = 6; sig [B][K+1][n] and navsig [B][K+1][14], kf [B][K][14][m], joint [B][K+1][N][N]):\n\n"
                        "| model | report only | + sig, navsig | + kf | + joint |\n|---|---|---|---|---|\n")
                for name, o in res["models"].items():
                    f.write("| %s | %s | %s | %s | %s |\n" % (name, fmt(o["nav_ms"]), fmt(o["nav_sig_ms"]), fmt(o["nav_kf_ms"]), fmt(o["nav_joint_ms"])))
                f.write("\nThe closed-loop flight without and with the navigation input (nsub = %d, no dense outputs), alternating windows:\n\n"
                        "| model | scvx_track_fly_f64 | scvx_track_fly_nav_f64 |\n|---|---|---|\n" % a.nsub)
                for name, o in res["models"].items():
                    f.write("| %s | %s | %s |\n" % (name, fmt(o["fly_ms"]), fmt(o["fly_nav_ms"])))
                f.write("\nWhat it shows -- the two converged plans of tests/golden/oracle_flight_runs.npz, default weights, handover S0 of "
                        "cov_reference.handover_s0(scale=0.1), N0 = 0.25 S0, position and velocity measured at every node with 1 sigma of 3e-5 "
                        "of the largest |r| and |v| component of x[0]; closed-loop landing 1 sigma from the device:\n\n"
                        "| plan | SIG_R without the navigation term | SIG_R with it | NAV_R | EST_R | SIG_V without | SIG_V with |\n|---|---|---|---|---|---|---|\n")
                for i, o in enumerate(res["golden"]):
                    f.write("| %d | %.3g | %.3g | %.3g | %.3g | %.3g | %.3g |\n" % (i, o["SIG_R_without"], o["SIG_R_with"], o["NAV_R"], o["EST_R"],
                                                                                o["SIG_V_without"], o["SIG_V_with"]))
            if a.track_json:
                par, this = res["track"]
                f.write("\n## The old path: scvx_track_fly_f64 on the parent commit and on this one\n\n`python tools/bench_track.py` on both "
                        "libraries in the same session (B = %d, nsub = %d), median (min .. max) of the windows in ms:\n\n"
                        "| model | entry | parent | this commit |\n|---|---|---|---|\n" % (this["B"], this["nsub"]))
                for name in this["models"]:
                    for key in ("fly_ms", "fly_clamp_ms", "fly_dense_ms", "fly_clamp_dense_ms", "shoot_xfly_ms"):
                        f.write("| %s | %s | %s | %s |\n" % (name, key[:-3], fmt(par["models"][name][key]), fmt(this["models"][name][key])))
            if a.build_logs:
                par, this = res["registers"]
                f.write("\n## Registers of fly_kernel\n\n`build.build(force=True, verbose=True)` on the parent commit and on this one "
                        "(template arguments: AERO, FIN, TRQ, TRACK, then the navigation pointer where there is one).  Every instantiation "
                        "the parent has keeps its figures: %s.\n\n| instantiation | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR "
                        "spills | waves/SIMD | parent |\n|---|---|---|---|---|---|---|---|---|\n"
                        % ("yes" if all(this.get(k) == v for k, v in par.items()) else "NO"))
                for k, v in this.items():
                    f.write("| %s | %s | %s |\n" % (k, " | ".join(str(v[n]) for n in FIGS[:7]),
                                                    "new" if k not in par else ("the same" if par[k] == v else str(par[k]))))
                f.write("\nnav_cov_kernel:\n\n| instantiation | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR spills | waves/SIMD | "
                        "LDS B/block |\n|---|---|---|---|---|---|---|---|---|\n")
                for k, v in res["nav_registers"].items():
                    f.write("| %s | %s |\n" % (k, " | ".join(str(v[n]) for n in FIGS)))


if __name__ == "__main__":
    main()
