"""Cost of the sampled closed-loop dispersion (scvx_track_mc_f64) next to the sampled check it replaces.

    python tools/bench_mc.py [--nsub 10] [--launches 50] [--repeats 5] [--json out.json]
    python tools/bench_mc.py --from-json out.json [--parent-log LOG --log LOG] --md profiles/mc.md      (no device needed)

For the flyable problem (mdry = 0.55, tf_guess = 8) on the exo and the aero + fins model, K = 50: 128 dispersed plans are stepped
`--plan-steps` times to get physical plans and their gains.  Then, in the same process, B S = 8192 flights are flown in three ways:
  * scvx_track_mc_f64 at B = 128, S = 64 and at B = 8, S = 1024 (device pointers, no dense output): one launch of the flight kernel
    and one of the finishing pass;
  * scvx_track_fly_f64 at B = 8192 on the REPLICATED plans (every plan, sigma and gain copied once per sample, the dx0 the new call
    forms), without and with the dense xfly / ufly the host-side reduction needs, and that reduction itself as the tests make it
    (copy to the host, sample covariance of the landing state and share of node controls outside the thrust band, in numpy).
HIP events, `--repeats` windows of `--launches` launches after a warm-up, median (min .. max) of the windows; the two calls whose
ratio is reported (track_mc and track_fly, both lean) in alternating windows; the host reduction by the wall clock.  Expectation
stated with the feature: per-flight time of the new call at most 1.10 x scvx_track_fly_f64's in the same run.  --parent-log / --log: the outputs of `python -m successiveconvexification_amd.build --force -v` on the parent commit and on
this one, for the resource tables."""
import argparse
import collections
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

FLYABLE = dict(mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
SHAPES = ((128, 64), (8, 1024))
FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "SGPRs Spill", "VGPRs Spill", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]")


def resources(log):
    """{mangled kernel name: {field: value}} from a verbose build log; the translation units compile side by side, so the remarks are
    taken file by file, where they are in order"""
    per = collections.defaultdict(list)
    pat = re.compile(r"(\S+?\.h(?:ip|pp)):\d+:\d+: remark:\s+(Function Name|%s): (\S+)" % "|".join(re.escape(f) for f in FIELDS))
    for line in open(log):
        m = pat.match(line)
        if m:
            per[m.group(1)].append((m.group(2), m.group(3)))
    out = {}
    for items in per.values():
        cur = None
        for k, v in items:
            if k == "Function Name":
                cur = out.setdefault(v, {})
            elif cur is not None:
                cur[k] = v
    return out


def demangled(name):
    """fly_kernel<true, false, ...> from the mangled name of one of the two flight kernels"""
    m = re.match(r"_ZN4scvx\d+(fly_kernel|mc_fly_kernel)I((?:Lb[01]E)+)(J(?:PKd)?E)?", name)
    if not m:
        return name
    args = ["true" if b == "1" else "false" for b in re.findall(r"Lb([01])E", m.group(2))]
    if m.group(3) and "PKd" in m.group(3):
        args.append("double const*")
    return "%s<%s>" % (m.group(1), ", ".join(args))


def resource_section(parent_log, log):
    par, new = resources(parent_log), resources(log)
    same = [n for n in par if par[n] == new.get(n)]
    lines = ["## Resources: parent against this change\n",
             "`python -m successiveconvexification_amd.build --force -v` (`-Rpass-analysis=kernel-resource-usage`) on the parent commit and "
             "on this one.  The parent reports %d kernels; %d of them report the same figures here (every field below), %d differ, %d are "
             "new.  The new kernels are in a translation unit of their own (`csrc/scvx_mc.hip`); `csrc/scvx_flight.hip` is unchanged.  "
             "mc_fly_kernel keeps the plan's values in scalar registers, so it spills more SGPRs (into VGPR lanes, not to scratch) than the "
             "tracking flyer fly_kernel<.., true>; VGPRs, scratch and occupancy are the tracking flyer's.\n"
             % (len(par), len(same), len(par) - len(same), len([n for n in new if n not in par])),
             "| kernel | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR spills | waves/SIMD | LDS B/block | parent |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    rows = [n for n in new if "fly_kernel" in n or "mc_finish" in n]
    for n in sorted(rows, key=lambda n: ("mc_" in n, n)):
        tag = "new" if n not in par else ("the same" if par[n] == new[n] else "WAS " + " ".join(par[n].get(f, "?") for f in FIELDS))
        lines.append("| %s | %s | %s |" % (demangled(n) if "fly_kernel" in n else "mc_finish_kernel", " | ".join(new[n].get(f, "?") for f in FIELDS), tag))
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

    def timed_ab(call_a, call_b):
        """the same for two calls in alternating windows: what a ratio of the two is taken from"""
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

    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
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
        b.close()
        L, h, nu = c._L, c.handle, c.nu
        n = 14 + nu
        sd = np.zeros(14)
        sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
        sd[7:] = 1e-3
        C0 = np.stack([mc.handover_factor(sd)] * PB)
        sw = np.full(14, 1e-5)
        out = {"shapes": {}}
        plan_doubles = (K + 1) * (14 + nu) + 1 + K * nu * n          # x, u, sigma and the gains of one plan
        for B, S in SHAPES:
            xi0, eta = mc.mc_draws(S, K, a.seed, noise=True)
            xd, ud, sg, gd, cd, xid, etd = (dev(v) for v in (x[:B], u[:B], s[:B], gain[:B], C0[:B], xi0, eta))
            rep, xm, xc = torch.empty((B, _lib.MC_NREP), **f64), torch.empty((B, 14), **f64), torch.empty((B, 14, 14), **f64)
            d0 = torch.empty((B, S, 14), **f64)
            o = {}
            call = lambda e, cl, d: L.scvx_track_mc_f64(h, B, K, S, vp(xd), vp(ud), vp(sg), vp(gd), vp(cd), vp(xid), e, dp(sw), None,   # noqa: E731
                                                        a.nsub, cl, 0.0, vp(rep), vp(xm), vp(xc), None, None, d)
            o["mc_noise_ms"] = timed(lambda: call(vp(etd), 0, None))
            o["mc_clamp_ms"] = timed(lambda: call(None, _lib.TRACK_CLAMP, None))
            assert call(None, 0, vp(d0)) == 0
            torch.cuda.synchronize()
            o["finite_flights"] = int(B * S - rep[:, 44].sum().item())
            o["plan_bytes"] = B * plan_doubles * 8
            # the same flights through scvx_track_fly_f64: every plan copied once per sample
            N = B * S
            rp = lambda t: t.repeat_interleave(S, dim=0).contiguous()   # noqa: E731
            xr, ur, sr, gr = rp(xd), rp(ud), rp(sg), rp(gd)
            o["replicated_bytes"] = N * plan_doubles * 8
            frep = torch.empty((N, _lib.FLIGHT_NREP), **f64)
            xf, uf = torch.empty((N, K + 1, 14), **f64), torch.empty((N, K + 1, nu), **f64)
            d0f = d0.reshape(N, 14)
            fly = lambda cl, dn: L.scvx_track_fly_f64(h, N, K, vp(xr), vp(ur), vp(sr), vp(gr), vp(d0f), a.nsub, cl, vp(frep),   # noqa: E731
                                                      vp(xf) if dn else None, vp(uf) if dn else None)
            o["mc_ms"], o["fly_ms"] = timed_ab(lambda: call(None, 0, None), lambda: fly(0, False))
            o["fly_clamp_ms"] = timed(lambda: fly(_lib.TRACK_CLAMP, False))
            o["fly_dense_ms"] = timed(lambda: fly(0, True))
            torch.cuda.synchronize()
            w = []
            for _ in range(a.repeats):   # the reduction of the tests: dense outputs to the host, then numpy
                t0 = time.perf_counter()
                xh, uh = xf.cpu().numpy().reshape(B, S, K + 1, 14), uf.cpu().numpy().reshape(B, S, K + 1, nu)
                e = xh[:, :, -1] - x[:B, None, -1]
                e = e - e.mean(axis=1, keepdims=True)
                cov = np.einsum("bsi,bsj->bij", e, e) / (S - 1)
                t = np.linalg.norm(uh[:, :, 1:, :3], axis=-1)
                outside = ((t < p.Tmin) | (t > p.Tmax)).sum(axis=(1, 2))
                w.append(1e3 * (time.perf_counter() - t0))
            o["host_reduce_ms"] = [float(np.median(w)), float(min(w)), float(max(w))]
            o["xcov_vs_host"] = float(np.abs(xc.cpu().numpy() - cov).max() / np.abs(cov).max())
            o["outside_matches"] = bool(np.array_equal(outside, np.rint((rep[:, 42] + rep[:, 43]).cpu().numpy() * S * K).astype(int)))
            o["ratio"] = o["mc_ms"][0] / o["fly_ms"][0]
            out["shapes"]["%dx%d" % (B, S)] = o
            del xr, ur, sr, gr, frep, xf, uf, d0
            torch.cuda.empty_cache()
        res["models"][name] = out
        c.set_stream(None)
        c.close()
    res["expectation_met"] = bool(all(o["ratio"] <= 1.10 for m in res["models"].values() for o in m["shapes"].values()))
    return res


def write_md(res, a):
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    with open(a.md, "w") as f:
        f.write("# Sampled closed-loop dispersion: device time at B S = 8192 flights, K = 50, nsub = %d\n\n" % res["nsub"])
        f.write("`python tools/bench_mc.py`; %s; HIP events; per entry %d windows of %d launches after %d warm-up launches, median (min .. "
                "max) of the windows in ms; fp64; flyable problem (mdry = 0.55, tf_guess = 8), plans after 3 solve_steps, weights q = 1, "
                "r = 1, qf = 100, handover 1e-3.  `track_mc`: scvx_track_mc_f64 without dense outputs (flight kernel + finishing pass); "
                "`track_fly`: scvx_track_fly_f64 at B = 8192 on the replicated plans, flown from the dx0 the new call formed; these two in "
                "alternating windows.\n\n"
                % (res["device"], res["repeats"], res["launches"], res["warmup"]))
        f.write("| model | B x S | track_mc | + noise | + clamp | track_fly | + clamp | + xfly, ufly | host reduction of xfly, ufly | track_mc / track_fly |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        for name, m in res["models"].items():
            for shp, o in m["shapes"].items():
                f.write("| %s | %s | %s | %s | %s | %s | %s | %s | %s | %.3f |\n"
                        % (name, shp.replace("x", " x "), fmt(o["mc_ms"]), fmt(o["mc_noise_ms"]), fmt(o["mc_clamp_ms"]), fmt(o["fly_ms"]),
                           fmt(o["fly_clamp_ms"]), fmt(o["fly_dense_ms"]), fmt(o["host_reduce_ms"]), o["ratio"]))
        f.write("\nPer flight, and the device memory that holds the plans and their gains in each form:\n\n"
                "| model | B x S | track_mc ns / flight | track_fly ns / flight | track_fly + xfly, ufly + host reduction ns / flight | plans + gains, shared | "
                "plans + gains, replicated |\n|---|---|---|---|---|---|---|\n")
        for name, m in res["models"].items():
            for shp, o in m["shapes"].items():
                N = 8192
                f.write("| %s | %s | %.1f | %.1f | %.1f | %.3f MB | %.1f MB |\n"
                        % (name, shp.replace("x", " x "), 1e6 * o["mc_ms"][0] / N, 1e6 * o["fly_ms"][0] / N,
                           1e6 * (o["fly_dense_ms"][0] + o["host_reduce_ms"][0]) / N, o["plan_bytes"] / 1e6, o["replicated_bytes"] / 1e6))
        f.write("\nIn every shape the device's xcov agrees with the host reduction of the replicated run to %.1e relative, and the number of "
                "node controls outside the band is %s.\n"
                % (max(o["xcov_vs_host"] for m in res["models"].values() for o in m["shapes"].values()),
                   "the same" if all(o["outside_matches"] for m in res["models"].values() for o in m["shapes"].values()) else "NOT the same"))
        worst = max(o["ratio"] for m in res["models"].values() for o in m["shapes"].values())
        f.write("\nExpectation (per-flight time of the new call at most 1.10 x that of scvx_track_fly_f64 in the same run): the largest ratio "
                "is %.3f: %s.\n\n" % (worst, "met" if res["expectation_met"] else "NOT met"))
        if a.parent_log and a.log:
            f.write(resource_section(a.parent_log, a.log))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nsub", type=int, default=10)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--plan-steps", type=int, default=3)
    ap.add_argument("--seed", type=int, default=20261004)
    ap.add_argument("--models", default="exo,aero+fins")
    ap.add_argument("--json", default=None)
    ap.add_argument("--from-json", default=None)
    ap.add_argument("--parent-log", default=None)
    ap.add_argument("--log", default=None)
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
