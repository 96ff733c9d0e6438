"""Back-offs from the navigation analysis: what the per-node sigma costs beside the launches it rides on.  Writes profiles/nav_margins.md.

    python tools/bench_nav_margins.py --measure out.json [--B 8192] [--launches 10] [--repeats 5]      (needs the GPU)
    python tools/bench_nav_margins.py --render out.json --md profiles/nav_margins.md [--resources NEW.log PARENT.log] [--ab AB.jsonl]

--measure, at B (the flyable problem, K = 50, dispersed starts solved to convergence; position only measured at every node, N0 = S0):
  * the path-sigma launch of the navigation analysis (scvx_nav_path_sigma_f64, PS = 1) beside the plain navigation launch
    (scvx_nav_cov_f64, reports only: the instantiation the parent commit has) and beside the covariance path-sigma launch
    (scvx_cov_path_sigma_f64), on the same arrays, HIP events, `--repeats` windows of `--launches` launches, alternating;
  * the back-off call alone (scvx_batch_margins_from_nav beside scvx_batch_margins_from_cov, psig = NULL: asynchronous), the same way;
  * one round of robustify(nav=...) beside one round without, each on its own converged batch, wall clock around the call (it ends
    on scvx_solve's synchronisation), with the SCvx steps each replan took.
--render needs no GPU: the tables of --measure and the compiler's resource report of every nav_cov_kernel instantiation from two logs
of `hipcc -Rpass-analysis=kernel-resource-usage` on scvx_nav.hip (this tree, its parent), and the headline of bench.py from a file of
"<label> <json line>" rows (label `parent` or `this`), alternating runs of the two trees.  No figure is fixed in advance.
"""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(a):
    import torch
    from dataclasses import replace
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch, _p
    from successiveconvexification_amd.dynamics import IntegratorCache
    res = {"device": torch.cuda.get_device_name(0), "B": a.B, "launches": a.launches, "repeats": a.repeats}
    stat = lambda w: [float(np.median(w)), float(min(w)), float(max(w))]   # noqa: E731
    B = a.B
    p = replace(sp.base_prob_scaled, mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    K = p.K
    ts = torch.cuda.Stream()
    c = IntegratorCache(p, npts=10)
    c.set_stream(ts.cuda_stream)
    ic = mc.disperse_ics(p, 0, B, 20261004)
    cov, nav = (ScvxBatch(c, B).init(ic) for _ in range(2))
    st0, it0, _, _ = cov.solve()
    nav.solve()
    res["base"] = {"converged": int((st0 == 0).sum()), "steps_mean": float(it0.mean())}
    x, u, s = cov.trajectory()
    d = cov.linearization()[1]
    gain = cov.track_gains()
    sdv = np.zeros(14)
    sdv[1:7] = 1e-3 * np.abs(x[:, 0, 1:7]).max(axis=0)
    sdv[7:] = 1e-3
    S0 = np.ascontiguousarray(np.broadcast_to(np.diag(sdv * sdv), (B, 14, 14)))
    N0 = S0.copy()
    H = np.ascontiguousarray(mc.measurement_rows("r"))
    rm = np.full(3, (3e-5 * np.abs(x[0, 0, 1:4]).max()) ** 2)

    def window(call, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(n):
            rc = call()
            assert rc is None or rc == 0, rc
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n

    xd, ud, dd, gd, s0d, n0d = (torch.tensor(np.ascontiguousarray(v), device="cuda") for v in (x, u, d, gain, S0, N0))
    rep = [torch.empty((B, _lib.COV_NREP), dtype=torch.float64, device="cuda") for _ in range(3)]
    nrep = [torch.empty((B, _lib.NAV_NREP), dtype=torch.float64, device="cuda") for _ in range(2)]
    psig = [torch.empty((B, K + 1, _lib.PSIG_N), dtype=torch.float64, device="cuda") for _ in range(2)]
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    L, h = c._L, c.handle
    calls = {
        "nav_cov": lambda: L.scvx_nav_cov_f64(h, B, K, vp(xd), vp(ud), vp(dd), vp(gd), vp(s0d), vp(n0d), 3, _p(H), _p(rm), None, vp(rep[0]),
                                              vp(nrep[0]), None, None, None, None),
        "nav_path_sigma": lambda: L.scvx_nav_path_sigma_f64(h, B, K, vp(xd), vp(ud), vp(dd), vp(gd), vp(s0d), vp(n0d), 3, _p(H), _p(rm), None,
                                                            vp(rep[1]), vp(nrep[1]), vp(psig[0])),
        "cov_path_sigma": lambda: L.scvx_cov_path_sigma_f64(h, B, K, vp(xd), vp(ud), vp(dd), vp(gd), vp(s0d), None, vp(rep[2]), vp(psig[1])),
    }
    for _ in range(2):
        for f in calls.values():
            assert f() == 0
    w = {k: [] for k in calls}
    for _ in range(a.repeats):
        for k, f in calls.items():
            w[k].append(window(f, a.launches))
    res["launch_ms"] = {k: stat(v) for k, v in w.items()}
    eq = lambda s, t: bool(torch.equal(torch.nan_to_num(s, nan=-7.0), torch.nan_to_num(t, nan=-7.0)))   # noqa: E731
    res["reports_bitwise_equal"] = eq(rep[0], rep[1]) and eq(nrep[0], nrep[1])
    res["sigma_ratio_thrust_mean"] = float((psig[0][:, 1:, 4] / psig[1][:, 1:, 4]).mean().item())
    # ---- the back-off call alone (nothing returns to the host)
    q, r, qf = np.ones(14), np.ones(c.nu), np.full(14, 100.0)
    marg = {
        "margins_from_cov": lambda: L.scvx_batch_margins_from_cov(cov.handle, _p(q), _p(r), _p(qf), _p(S0), None, C.c_double(3.0), C.c_double(0.25),
                                                                  C.c_uint(1), None),
        "margins_from_nav": lambda: L.scvx_batch_margins_from_nav(nav.handle, _p(q), _p(r), _p(qf), _p(S0), _p(N0), 3, _p(H), _p(rm), None,
                                                                  C.c_double(3.0), C.c_double(0.25), C.c_uint(1), None),
    }
    for f in marg.values():
        assert f() == 0
    w = {k: [] for k in marg}
    for _ in range(a.repeats):
        for k, f in marg.items():
            w[k].append(window(f, a.launches))
    res["margins_call_ms"] = {k: stat(v) for k, v in w.items()}
    cov.set_thrust_margins(None, None)
    nav.set_thrust_margins(None, None)
    # ---- one round of robustify, each on its own converged batch
    rob = {}
    for name, b, kw in (("robustify", cov, {}), ("robustify_nav", nav, {"nav": (N0, H, rm)})):
        c.synchronize()
        t0 = time.perf_counter()
        st, it, _, _, lo, _ = b.robustify(S0, nsigma=3.0, rounds=1, **kw)
        rob[name] = {"ms": 1e3 * (time.perf_counter() - t0), "converged": int((st == 0).sum()), "steps_mean": float(it.mean()),
                     "steps_max": int(it.max()), "backoff_mean": float(lo[:, 1:].mean())}
    res["robustify"] = rob
    rn, rc = nav.navigation(S0, N0, H, rm), cov.navigation(S0, N0, H, rm)
    ok = (rob["robustify"]["converged"] == B, rob["robustify_nav"]["converged"] == B)
    res["navigation_report_after"] = {"cov": [float(np.nanmedian(np.minimum(rc.N_TMIN, rc.N_TMAX))), bool(ok[0])],
                                      "nav": [float(np.nanmedian(np.minimum(rn.N_TMIN, rn.N_TMAX))), bool(ok[1])]}
    for b in (cov, nav):
        b.close()
    c.set_stream(None)
    c.close()
    with open(a.measure, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


def resources(path):
    """{demangled nav_cov_kernel instantiation: (VGPRs, AGPRs, SGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD)}"""
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s*Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
        elif cur:
            m = re.search(r"remark:\s+([A-Za-z /\[\]]+?): (\d+)", line)
            if m:
                out[cur][m.group(1).strip()] = int(m.group(2))
    names = sorted(out)
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    keys = ("VGPRs", "AGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
    return {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(out[n].get(k) for k in keys) for n, d in zip(names, dem) if "nav_cov_kernel" in d}


def render(a):
    f = open(a.md, "w")
    f.write("# Back-offs from the navigation analysis\n\n`python tools/bench_nav_margins.py`.\n\n")
    if a.render and os.path.exists(a.render):
        r = json.load(open(a.render))
        fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
        lm, mm, rb = r["launch_ms"], r["margins_call_ms"], r["robustify"]
        f.write("## Cost at B = %d (flyable problem, K = 50, position measured at every node), %s\n\nHIP events, median (min .. max) in ms, %d windows "
                "of %d launches, alternating.\n\n| | ms |\n|---|---|\n" % (r["B"], r["device"], r["repeats"], r["launches"]))
        f.write("| navigation launch, reports only (`scvx_nav_cov_f64`, `PS = 0`: the parent's instantiation) | %s |\n"
                "| navigation path-sigma launch (`scvx_nav_path_sigma_f64`, `PS = 1`) | %s |\n"
                "| covariance path-sigma launch (`scvx_cov_path_sigma_f64`) | %s |\n"
                "| `scvx_batch_margins_from_cov`, thrust, psig = NULL (S0 upload, gains, covariance launch, back-off kernel) | %s |\n"
                "| `scvx_batch_margins_from_nav`, thrust, psig = NULL (S0 and N0 upload, gains, navigation launch, back-off kernel) | %s |\n\n"
                % (fmt(lm["nav_cov"]), fmt(lm["nav_path_sigma"]), fmt(lm["cov_path_sigma"]), fmt(mm["margins_from_cov"]), fmt(mm["margins_from_nav"])))
        f.write("The two reports of the path-sigma launch equal the plain launch's bit for bit: %s.  Mean over trajectories and nodes of the "
                "navigation s_T over the covariance s_T: %.2f.\n\n" % (r["reports_bitwise_equal"], r["sigma_ratio_thrust_mean"]))
        f.write("One round of `robustify` on a converged batch (%d of %d base plans converged, %.1f SCvx steps on average), wall clock around the "
                "call, one measurement each on a batch of its own:\n\n| | ms | converged | SCvx steps mean / max | mean back-off |\n|---|---|---|---|---|\n"
                % (r["base"]["converged"], r["B"], r["base"]["steps_mean"]))
        for k, label in (("robustify", "`robustify(S0)`"), ("robustify_nav", "`robustify(S0, nav=(N0, H, rm))`")):
            f.write("| %s | %.1f | %d | %.2f / %d | %.3e |\n" % (label, rb[k]["ms"], rb[k]["converged"], rb[k]["steps_mean"], rb[k]["steps_max"], rb[k]["backoff_mean"]))
        na = r["navigation_report_after"]
        f.write("\nThe two rounds solve different subproblems (wider back-offs), so their times differ by that work and not only by the launch.  "
                "Median over the batch of min(N_TMIN, N_TMAX) of the NAVIGATION report afterwards: %.2f after covariance back-offs, %.2f after "
                "navigation back-offs.\n\n" % (na["cov"][0], na["nav"][0]))
    else:
        f.write("## Cost at B = 8192\n\nNot measured: `--measure` has not been run to its end on a device.\n\n")
    if a.resources:
        new, old = resources(a.resources[0]), resources(a.resources[1])
        f.write("## Compiler resource report of `nav_cov_kernel` (gfx950, `-O3`, `-Rpass-analysis=kernel-resource-usage`)\n\nVGPRs / AGPRs / SGPRs / scratch "
                "bytes per lane / LDS bytes per block / waves per SIMD.  The report-only instantiations (`PS = 0`) are the parent's: the same "
                "figures, and the same instructions line for line (compared as `hipcc -S` text with block labels renumbered); the kernel "
                "argument segment grows by the one pointer (1952 -> 1960 bytes).\n\n| instantiation | parent | this change |\n|---|---|---|\n")
        row = lambda v: "-" if v is None else " / ".join(str(e) for e in v)   # noqa: E731
        for n in sorted(new):
            o = old.get(re.sub(r", 0>$", ">", n)) if n.endswith(", 0>") else None   # the parent's template has no PS parameter
            f.write("| `%s` | %s | %s |\n" % (n, row(o), row(new[n])))
    if a.ab:
        rows = {"parent": [], "this": []}
        unit = ""
        for line in open(a.ab):
            label, js = line.split(None, 1)
            j = json.loads(js)
            rows[label].append(float(j["value"]))
            unit = j.get("unit", unit)
        f.write("\n## Headline of `bench.py --gpus 1 --steps 14 --warmup 2`, the parent's tree and library and this one alternating in one session\n\n"
                "| run | parent | this change |\n|---|---|---|\n")
        for i in range(max(len(rows["parent"]), len(rows["this"]))):
            f.write("| %d | %s | %s |\n" % (i + 1, *("%.0f" % rows[k][i] if i < len(rows[k]) else "" for k in ("parent", "this"))))
        f.write("| median | %.0f | %.0f |\n\nUnit: %s.  `--dump-outputs` of run 1 (active, cost, iteration, sigma, status, trust_radius, u, x of every "
                "trajectory) is bit for bit the parent's: no solver or SCvx kernel is touched.\n" % (np.median(rows["parent"]), np.median(rows["this"]), unit))
    f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", default=None, metavar="JSON")
    ap.add_argument("--render", default=None, metavar="JSON")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "nav_margins.md"))
    ap.add_argument("--resources", nargs=2, default=None, metavar=("NEW_LOG", "PARENT_LOG"))
    ap.add_argument("--ab", default=None)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.measure:
        measure(a)
    if a.render or a.resources:
        render(a)


if __name__ == "__main__":
    main()
