"""Cost of the order statistics and the per-node samples of the sampled dispersion (scvx_track_mc_q_f64, scvx_order_stats_f64) next to
the plain sampled call, measured in the same run.

    python tools/bench_mc_quantiles.py [--nsub 10] [--launches 20] [--repeats 5] [--json out.json]
    python tools/bench_mc_quantiles.py --from-json out.json [--parent-log LOG --log LOG] --md profiles/mc_quantiles.md   (no device needed)

For the flyable problem (mdry = 0.55, tf_guess = 8) on the exo and the aero + fins model, K = 50, nsub = 10: 128 dispersed plans are
stepped `--plan-steps` times to get physical plans and their gains.  Then B S = 8192 flights as 128 x 64 and as 8 x 1024, device pointers:
  * `mc`: scvx_track_mc_f64, no dense output -- the plain call, in windows alternating with
  * `mc_q`: scvx_track_mc_q_f64 with flightq and pathq for 4 ranks, no dense output (the values live in the context's workspace): the
    flight kernel with the per-node stores, the finishing pass and two order-statistics launches;
  * `mc_q + pathv`: the same with the dense pathv handed to the caller;
  * `order_stats`: scvx_order_stats_f64 alone on the rows of pathv of each shape (B 51 5 rows of S values), and on 16 rows of 8,192.
HIP events, `--repeats` windows of `--launches` launches after a warm-up, median (min .. max) of the windows.  Expectation stated with
the feature, not a bar: the per-node stores are B (K + 1) 5 S doubles = 16.7 MB per launch, so the overhead of mc_q over mc should be a
small fraction of the flight.  --parent-log / --log: the outputs of `python -m successiveconvexification_amd.build --force -v` on the
parent commit and on this one, for the resource tables."""
import argparse
import ctypes as C
import json
import os
import re
import sys
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_mc import FIELDS, FLYABLE, SHAPES, resources   # noqa: E402  the verbose build log's parser and the flyable problem

PROBS = (0.00135, 0.5, 0.99, 0.99865)
LONG_ROWS = (16, 8192)


def _key(name):
    """(kernel<template arguments>, PV) of a flying kernel of the sampled calls from its mangled name, the trailing PV argument (absent
    in the parent) apart; None for every other kernel"""
    m = re.match(r"_ZN4scvx\d+(mc_fly_kernel|mc_nav_fly_kernel)I((?:Lb[01]E)+)([df]?)((?:Lb[01]E)*)E", name)
    if not m:
        return None
    b = ["true" if v == "1" else "false" for v in re.findall(r"Lb([01])E", m.group(2))]
    t = {"d": ["double"], "f": ["float"], "": []}[m.group(3)]
    pv = re.findall(r"Lb([01])E", m.group(4))
    if m.group(1) == "mc_fly_kernel" and len(b) == 4:
        b, pv = b[:3], [{"true": "1", "false": "0"}[b[3]]]
    return "%s<%s>" % (m.group(1), ", ".join(b + t)), (pv[0] == "1") if pv else False


def resource_section(parent_log, log):
    par, new = resources(parent_log), resources(log)
    same = differ = 0
    rows = []
    for n, r in new.items():
        k = _key(n)
        if k is None:
            if n in par:
                same += par[n] == r
                differ += par[n] != r
            elif "order_stats" in n:
                rows.append(("order_stats_kernel", r, "new"))
            continue
        if k[1]:
            rows.append((k[0][:-1] + ", PV>", r, "new"))
            continue
        old = [p for m, p in par.items() if _key(m) == k]
        tag = "the same" if old and old[0] == r else ("WAS " + " ".join(old[0].get(f, "?") for f in FIELDS) if old else "new")
        same += tag == "the same"
        differ += tag.startswith("WAS")
        rows.append((k[0], r, tag))
    lines = ["## Resources: parent against this change\n",
             "`python -m successiveconvexification_amd.build --force -v` (`-Rpass-analysis=kernel-resource-usage`, gfx950) on the parent commit "
             "and on this one.  The parent reports %d kernels; %d of them report the same figures here (every field below), %d differ.  The "
             "two flying kernels gained one compile-time parameter, PV (and one trailing pointer argument): their instantiations with PV off "
             "are matched to the parent's by their other template arguments.  New: the instantiations with PV on and order_stats_kernel "
             "(`csrc/scvx_quantile.hip`; its LDS is dynamic -- 8 min(S, 4096) bytes of keys, and above S = 256 1024 nq bytes of histograms, "
             "per block on top of the static bytes below).  Below: the flying kernels of the sampled calls and the new kernel.\n" % (len(par), same, differ),
             "| kernel | SGPRs | VGPRs | AGPRs | scratch B/lane | SGPR spills | VGPR spills | waves/SIMD | LDS B/block | parent |",
             "|---|---|---|---|---|---|---|---|---|---|"]
    for name, r, tag in sorted(rows, key=lambda t: ("order" in t[0], "nav" in t[0], "PV" in t[0], t[0])):
        lines.append("| %s | %s | %s |" % (name, " | ".join(r.get(f, "?") for f in FIELDS), tag))
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
    res = {"nsub": a.nsub, "launches": a.launches, "repeats": a.repeats, "warmup": a.warmup, "device": torch.cuda.get_device_name(0),
           "probs": list(PROBS), "models": {}}

    def window(call):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(a.launches):
            call()
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / a.launches

    def timed(*calls):
        """[median, min, max] ms per launch over the windows, per call; several calls: alternating windows"""
        for call in calls:
            for _ in range(a.warmup):
                assert call() == 0
        w = [[] for _ in calls]
        for _ in range(a.repeats):
            for i, call in enumerate(calls):
                w[i].append(window(call))
        out = [[float(np.median(v)), float(min(v)), float(max(v))] for v in w]
        return out if len(calls) > 1 else out[0]

    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    dev = lambda v: torch.tensor(np.ascontiguousarray(v), device="cuda")   # noqa: E731
    f64 = dict(dtype=torch.float64, device="cuda")
    ip = C.POINTER(C.c_int)
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
        L, h = c._L, c.handle
        sd = np.zeros(14)
        sd[1:7] = 1e-3 * np.abs(x[0, 0, 1:7])
        sd[7:] = 1e-3
        C0 = np.stack([mc.handover_factor(sd)] * PB)
        out = {"shapes": {}}
        for B, S in SHAPES:
            xi0, _ = mc.mc_draws(S, K, a.seed)
            xd, ud, sg, gd, cd, xid = (dev(v) for v in (x[:B], u[:B], s[:B], gain[:B], C0[:B], xi0))
            rep, xm, xc = torch.empty((B, _lib.MC_NREP), **f64), torch.empty((B, 14), **f64), torch.empty((B, 14, 14), **f64)
            rk = np.ascontiguousarray(mc.quantile_ranks(PROBS, S), np.int32)
            nq = int(rk.size)
            fq, pq = torch.empty((B, 16, nq), **f64), torch.empty((B, K + 1, 5, nq), **f64)
            pv = torch.empty((B, K + 1, 5, S), **f64)
            head = (h, B, K, S, vp(xd), vp(ud), vp(sg), vp(gd), vp(cd), vp(xid), None, None, None, a.nsub, 0, 0.0, vp(rep), vp(xm), vp(xc),
                    None, None, None)
            plain = lambda: L.scvx_track_mc_f64(*head)   # noqa: E731
            q = lambda: L.scvx_track_mc_q_f64(*head, nq, rk.ctypes.data_as(ip), vp(fq), vp(pq), None)   # noqa: E731
            qd = lambda: L.scvx_track_mc_q_f64(*head, nq, rk.ctypes.data_as(ip), vp(fq), vp(pq), vp(pv))   # noqa: E731
            pvonly = lambda: L.scvx_track_mc_q_f64(*head, 0, None, None, None, vp(pv))   # noqa: E731
            o = {"ranks": rk.tolist()}
            o["mc_ms"], o["mc_q_ms"] = timed(plain, q)
            o["mc_q_dense_ms"] = timed(qd)
            o["mc_pathv_only_ms"] = timed(pvonly)
            R = B * (K + 1) * 5
            o["order_stats_rows"] = R
            o["order_stats_ms"] = timed(lambda: L.scvx_order_stats_f64(h, R, S, vp(pv), S, 1, nq, rk.ctypes.data_as(ip), vp(pq)))
            o["flight_stats_ms"] = timed(lambda: L.scvx_order_stats_f64(h, B * 16, S, vp(pv), S, 1, nq, rk.ctypes.data_as(ip), vp(fq)))
            torch.cuda.synchronize()
            o["finite_flights"] = int(B * S - rep[:, 44].sum().item())
            ref = np.sort(pv.cpu().numpy(), axis=-1)[..., rk]
            o["pathq_is_numpy"] = bool(np.array_equal(pq.cpu().numpy(), ref, equal_nan=True))
            o["pathv_bytes"] = R * S * 8
            o["overhead"] = o["mc_q_ms"][0] / o["mc_ms"][0] - 1.0
            out["shapes"]["%dx%d" % (B, S)] = o
        res["models"][name] = out
        c.set_stream(None)
        if name == a.models.split(",")[0]:
            Rl, Sl = LONG_ROWS
            v = torch.randn((Rl, Sl), **f64)
            rk = np.ascontiguousarray(mc.quantile_ranks(PROBS, Sl), np.int32)
            o8 = torch.empty((Rl, rk.size), **f64)
            c.set_stream(ts.cuda_stream)
            res["long_rows_ms"] = timed(lambda: L.scvx_order_stats_f64(h, Rl, Sl, vp(v), Sl, 1, int(rk.size), rk.ctypes.data_as(ip), vp(o8)))
            torch.cuda.synchronize()
            res["long_rows_is_numpy"] = bool(np.array_equal(o8.cpu().numpy(), np.sort(v.cpu().numpy(), axis=-1)[:, rk]))
            c.set_stream(None)
        c.close()
    return res


def write_md(res, a):
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    with open(a.md, "w") as f:
        f.write("# Order statistics and per-node samples of the sampled dispersion\n\n")
        f.write("Device time at B S = 8192 flights, K = 50, nsub = %d.  `python tools/bench_mc_quantiles.py`; %s; HIP events; per entry %d windows "
                "of %d launches after %d warm-up launches, median (min .. max) of the windows in ms; fp64; flyable problem (mdry = 0.55, "
                "tf_guess = 8), plans after 3 solve_steps, weights q = 1, r = 1, qf = 100, handover 1e-3, no noise, no clamp; 4 ranks, those of "
                "p = %s.  `mc`: scvx_track_mc_f64 without dense outputs, the plain call, in windows alternating with `mc_q`: "
                "scvx_track_mc_q_f64 with flightq and pathq (values in the context's workspace); `+ pathv`: the same with the dense pathv; "
                "`pathv only`: the per-node stores without any order statistic; `order_stats`: scvx_order_stats_f64 alone on the B 51 5 rows "
                "of that pathv, and on its first B 16 rows (the cost of flightq's launch shape).\n\n"
                % (res["nsub"], res["device"], res["repeats"], res["launches"], res["warmup"], ", ".join("%g" % v for v in res["probs"])))
        f.write("| model | B x S | mc | mc_q | mc_q / mc - 1 | + pathv | pathv only | order_stats, B 51 5 rows | order_stats, B 16 rows | pathv |\n"
                "|---|---|---|---|---|---|---|---|---|---|\n")
        for name, m in res["models"].items():
            for shp, o in m["shapes"].items():
                f.write("| %s | %s | %s | %s | %+.1f %% | %s | %s | %s | %s | %.1f MB |\n"
                        % (name, shp.replace("x", " x "), fmt(o["mc_ms"]), fmt(o["mc_q_ms"]), 100 * o["overhead"], fmt(o["mc_q_dense_ms"]),
                           fmt(o["mc_pathv_only_ms"]), fmt(o["order_stats_ms"]), fmt(o["flight_stats_ms"]), o["pathv_bytes"] / 1e6))
        every = [o for m in res["models"].values() for o in m["shapes"].values()]
        f.write("\n%d rows of %d values, 4 ranks (the keys read from global memory eight times, S > 4096): %s ms; equal to numpy's sort and "
                "rank: %s.  In every shape above pathq is bitwise numpy's sort and rank of the same launch's pathv (%s) and every flight is "
                "finite (%s).\n"
                % (LONG_ROWS[0], LONG_ROWS[1], fmt(res["long_rows_ms"]), res["long_rows_is_numpy"], all(o["pathq_is_numpy"] for o in every),
                   all(o["finite_flights"] == 8192 for o in every)))
        lo, hi = min(o["overhead"] for o in every), max(o["overhead"] for o in every)
        f.write("\nExpectation stated with the feature (not a bar): the per-node stores are 16.7 MB per launch, so the overhead of mc_q over "
                "the plain call of the same run should be a small fraction of the flight.  Measured: %+.1f %% .. %+.1f %%.\n\n" % (100 * lo, 100 * hi))
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
