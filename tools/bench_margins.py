"""Thrust-band back-offs and covariance-driven replanning: what they cost and what they buy.  Writes profiles/margins.md.

    python tools/bench_margins.py --measure out.json [--B 8192] [--launches 20] [--repeats 5]      (needs the GPU)
    python tools/bench_margins.py --render out.json --md profiles/margins.md [--resources NEW.log PARENT.log] [--ab AB.jsonl]

--measure:
  * robustify on the fixture trajectories (tests/golden/oracle_margin_runs.npz, the flyable problem): N_TMIN / N_TMAX / S_THRUST and
    the final mass before and after one round at nsigma = 3, the replan's step count, and the number of commanded node controls
    outside [Tmin, Tmax] over 256 Gaussian starts per plan (one seed) flown closed loop on the base and on the robustified plan;
  * at B (exo, dispersed batch stepped 3 times): the path-sigma launch (scvx_cov_path_sigma_f64) beside the covariance launch
    (scvx_cov_propagate_f64) on the same arrays, HIP events, `--repeats` windows of `--launches` launches, alternating;
  * at B: a solve_step under back-offs beside one without, two batches from the same start, alternating single steps from
    scvx_batch_reset (the same subproblems every time), HIP events.
--render needs no GPU: the tables of --measure, the compiler's resource report of every socp_* and covariance kernel from two logs of
`python -m successiveconvexification_amd.build --force -v` (this tree, its parent), and the headline of bench.py from a file of
"<label> <json line>" rows (label `parent` or `this`), alternating runs of the two libraries.
"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))


def measure(a):
    import torch
    import cov_reference as cr
    from dataclasses import replace
    from successiveconvexification_amd import _lib, montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    res = {"device": torch.cuda.get_device_name(0), "B": a.B, "launches": a.launches, "repeats": a.repeats}
    stat = lambda w: [float(np.median(w)), float(min(w)), float(max(w))]   # noqa: E731
    # ---- robustify on the fixture trajectories
    g = np.load(os.path.join(ROOT, "tests", "golden", "oracle_margin_runs.npz"))
    p = replace(sp.base_prob_scaled, mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    c = IntegratorCache(p, npts=10)
    ic = g["ic"]
    P, N = ic.shape[0], 256
    base, rob = (ScvxBatch(c, P).init(ic) for _ in range(2))
    st0, it0, _, _ = base.solve()
    rob.solve()
    S0 = np.stack([cr.handover_s0(x0, 0, 1e-3)[0] for x0 in base.trajectory()[0][:, 0]])
    before = base.covariance(S0)
    st, it, nu, dj, lo, hi = rob.robustify(S0, nsigma=3.0, rounds=1)
    after = rob.covariance(S0)
    fleet = ScvxBatch(c, N * P).init(np.repeat(ic, N, axis=0))
    dx0 = np.concatenate([mc.gaussian_handover(S0[i], 0, N, 20261018) for i in range(P)])
    out = {}
    for name, b in (("base", base), ("robustified", rob)):
        x, u, s = b.trajectory()
        fleet.set_trajectory(np.repeat(x, N, axis=0), np.repeat(u, N, axis=0), np.repeat(s, N, axis=0))
        t = np.linalg.norm(fleet.track(dx0, dense=True).ufly[:, :, :3], axis=-1).reshape(P, N, -1)
        out[name] = ((t < p.Tmin) | (t > p.Tmax)).sum(axis=(1, 2)).tolist()
    res["robustify"] = {
        "plans": g["plans"].tolist(), "base_status": st0.tolist(), "base_steps": it0.tolist(), "status": st.tolist(), "replan_steps": it.tolist(),
        "N_TMIN": [before.N_TMIN.tolist(), after.N_TMIN.tolist()], "N_TMAX": [before.N_TMAX.tolist(), after.N_TMAX.tolist()],
        "S_THRUST": [before.S_THRUST.tolist(), after.S_THRUST.tolist()],
        "mass": [base.trajectory()[0][:, -1, 0].tolist(), rob.trajectory()[0][:, -1, 0].tolist()], "backoff_max": lo.max(axis=1).tolist(),
        "oracle_N_TMIN": g["replan_rep"][:, cr.IDX["N_TMIN"]].tolist(), "oracle_N_TMAX": g["replan_rep"][:, cr.IDX["N_TMAX"]].tolist(),
        "oracle_mass": g["replan_x"][:, -1, 0].tolist(), "oracle_steps": (g["replan_accepted"] >= 0).sum(axis=1).tolist(),
        "starts_per_plan": N, "nodes": p.K + 1, "out_of_band": out}
    for b in (base, rob, fleet):
        b.close()
    c.close()
    # ---- timings at B
    B, p = a.B, sp.base_prob_scaled
    K = p.K
    ts = torch.cuda.Stream()
    c = IntegratorCache(p, npts=10)
    c.set_stream(ts.cuda_stream)
    icB = mc.disperse_ics(p, 0, B, 20261004)

    def window(call, n):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record(ts)
        for _ in range(n):
            rc = call()
            assert rc is None or rc == 0, rc
        t1.record(ts)
        torch.cuda.synchronize()
        return t0.elapsed_time(t1) / n

    plain, marg = (ScvxBatch(c, B).init(icB) for _ in range(2))
    band = p.Tmax - p.Tmin
    marg.set_thrust_margins(0.05 * band, 0.05 * band)
    w = {"plain": [], "margined": []}
    for rnd in range(a.repeats + 1):
        for name, b in (("plain", plain), ("margined", marg)):
            b.reset()
            c.synchronize()
            t = window(b.solve_step_async, 1)
            if rnd:
                w[name].append(t)
    res["solve_step_ms"] = {k: stat(v) for k, v in w.items()}
    res["solve_step_ipm_iters"] = {"plain": float(plain.solver_stats()[1].mean()), "margined": float(marg.solver_stats()[1].mean())}
    marg.close()
    for _ in range(2):
        plain.solve_step_async()
    x, u, s = plain.trajectory()
    d = plain.linearization()[1]
    gain = plain.track_gains()
    plain.close()
    sdv = np.zeros(14)
    sdv[1:7] = 1e-3 * np.abs(x[:, 0, 1:7]).max(axis=0)
    sdv[7:] = 1e-3
    S0 = np.ascontiguousarray(np.broadcast_to(np.diag(sdv * sdv), (B, 14, 14)))
    xd, ud, dd, gd, s0d = (torch.tensor(np.ascontiguousarray(v), device="cuda") for v in (x, u, d, gain, S0))
    rep = torch.empty((B, _lib.COV_NREP), dtype=torch.float64, device="cuda")
    rep2 = torch.empty_like(rep)
    psig = torch.empty((B, K + 1, _lib.PSIG_N), dtype=torch.float64, device="cuda")
    vp = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    L, h = c._L, c.handle
    cov = lambda: L.scvx_cov_propagate_f64(h, B, K, vp(xd), vp(ud), vp(dd), vp(gd), vp(s0d), None, vp(rep), None, None, None)   # noqa: E731
    pth = lambda: L.scvx_cov_path_sigma_f64(h, B, K, vp(xd), vp(ud), vp(dd), vp(gd), vp(s0d), None, vp(rep2), vp(psig))   # noqa: E731
    for _ in range(3):
        assert cov() == 0 and pth() == 0
    w = {"cov": [], "path_sigma": []}
    for _ in range(a.repeats):
        w["cov"].append(window(cov, a.launches))
        w["path_sigma"].append(window(pth, a.launches))
    torch.cuda.synchronize()
    res["cov_ms"], res["path_sigma_ms"] = stat(w["cov"]), stat(w["path_sigma"])
    res["report_bitwise_equal"] = bool(torch.equal(torch.nan_to_num(rep, nan=-7.0), torch.nan_to_num(rep2, nan=-7.0)))
    c.set_stream(None)
    c.close()
    with open(a.measure, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


def resources(path):
    """{demangled kernel name without arguments: (VGPRs, AGPRs, scratch bytes per lane, LDS bytes per block, waves per SIMD, spilled VGPRs)}"""
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
    keys = ("VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]", "VGPRs Spill")
    return {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(out[n].get(k) for k in keys) for n, d in zip(names, dem)
            if re.search(r"socp|cov_propagate|margins_from_psig|replan_scalars", d)}


def render(a):
    r = json.load(open(a.render))
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    f = open(a.md, "w")
    f.write("# Thrust-band back-offs and covariance-driven replanning\n\n`python tools/bench_margins.py`; %s.\n\n" % r["device"])
    q = r["robustify"]
    f.write("## What one round of `robustify` buys (flyable problem, the trajectories of `tests/golden/oracle_margin_runs.npz`: plans %s of "
            "`oracle_flight_runs.npz`)\n\nnsigma = 3, cap = 0.25, S0 = `cov_reference.handover_s0(x0, 0, 1e-3)`, default weights.  The last "
            "column is the CPU oracle's re-plan of the same plan under the back-offs of ITS base plan (another run of another solver: "
            "for orientation, not a parity figure).\n\n| | base plan (device) | after one round (device) | CPU oracle's re-plan |\n|---|---|---|---|\n" % q["plans"])
    f.write("| N_TMIN | %s | %s | %s |\n| N_TMAX | %s | %s | %s |\n" % (q["N_TMIN"][0], q["N_TMIN"][1], q["oracle_N_TMIN"], q["N_TMAX"][0], q["N_TMAX"][1], q["oracle_N_TMAX"]))
    f.write("| S_THRUST | %s | %s | |\n| final mass | %s | %s | %s |\n| SCvx steps | %s | %s | %s |\n| status | %s | %s | |\n| largest back-off | | %s | |\n"
            % (q["S_THRUST"][0], q["S_THRUST"][1], q["mass"][0], q["mass"][1], q["oracle_mass"], q["base_steps"], q["replan_steps"], q["oracle_steps"],
               q["base_status"], q["status"], q["backoff_max"]))
    f.write("\nCommanded node controls outside [Tmin, Tmax] in the closed loop (`track(dx0, dense=True)`, no clamp), %d Gaussian starts per plan "
            "(`montecarlo.gaussian_handover`, seed 20261018) x %d nodes: base plan %s, robustified plan %s.\n\n"
            % (q["starts_per_plan"], q["nodes"], q["out_of_band"]["base"], q["out_of_band"]["robustified"]))
    if "cov_ms" not in r:
        f.write("## Cost at B = 8192\n\nNot measured yet: `--measure` has not been run to its end on a device.\n\n")
    else:
        render_cost(f, r, fmt)
    render_rest(f, a)
    f.close()


def render_cost(f, r, fmt):
    f.write("## Cost at B = %d (exo, K = 50), HIP events, median (min .. max) in ms\n\n" % r["B"])
    f.write("| | ms |\n|---|---|\n| covariance launch, report only (`scvx_cov_propagate_f64`) | %s |\n| path-sigma launch (`scvx_cov_path_sigma_f64`) | %s |\n"
            % (fmt(r["cov_ms"]), fmt(r["path_sigma_ms"])))
    f.write("| first `solve_step` from `scvx_batch_reset`, no back-offs | %s |\n| the same under back-offs of 5 %% of the band on both sides | %s |\n"
            % (fmt(r["solve_step_ms"]["plain"]), fmt(r["solve_step_ms"]["margined"])))
    f.write("\n%d windows of %d launches (covariance), %d single steps each (solve_step), alternating.  Interior-point iterations per solve: %.2f "
            "without, %.2f with back-offs (another subproblem: the step times differ by that much work, not by the two loads).  The report "
            "of the path-sigma launch equals the covariance launch's bit for bit: %s.\n\n"
            % (r["repeats"], r["launches"], r["repeats"], r["solve_step_ipm_iters"]["plain"], r["solve_step_ipm_iters"]["margined"], r["report_bitwise_equal"]))


def render_rest(f, a):
    if not a.ab:
        f.write("## Headline of `bench.py`, parent against this change\n\nNot measured yet: no file of alternating runs was given (`--ab`).\n\n")
    if a.ab:
        rows = {"parent": [], "this": []}
        unit = ""
        for line in open(a.ab):
            label, js = line.split(None, 1)
            j = json.loads(js)
            rows[label].append(float(j["value"]))
            unit = j.get("unit", unit)
        f.write("## Headline of `bench.py --gpus 1 --steps 14 --warmup 2`, the parent's library and this one alternating in one session\n\n"
                "| run | parent | this change |\n|---|---|---|\n")
        for i in range(max(len(rows["parent"]), len(rows["this"]))):
            f.write("| %d | %s | %s |\n" % (i + 1, *("%.1f" % rows[k][i] if i < len(rows[k]) else "" for k in ("parent", "this"))))
        f.write("| median | %.1f | %.1f |\n| min .. max | %.1f .. %.1f | %.1f .. %.1f |\n\nUnit: %s.\n\n"
                % (np.median(rows["parent"]), np.median(rows["this"]), min(rows["parent"]), max(rows["parent"]), min(rows["this"]), max(rows["this"]), unit))
    if a.resources:
        new, old = resources(a.resources[0]), resources(a.resources[1])
        f.write("## Compiler resource report (gfx950, `-Rpass-analysis=kernel-resource-usage`)\n\nVGPRs / AGPRs / scratch bytes per lane / LDS bytes "
                "per block / waves per SIMD / spilled VGPRs.  The conic kernels gain one pointer in the solver frame (16 bytes of LDS per "
                "wavefront); the covariance kernel's report-only instantiations (`PS = 0`) are the parent's.\n\n| kernel | parent | this change |\n|---|---|---|\n")
        strip = lambda n: re.sub(r", 0>$", ">", n)   # noqa: E731  the parent's covariance template has no PS parameter
        for n in sorted(new):
            o = old.get(n, old.get(strip(n))) if not n.endswith(", 1>") or n in old else None
            row = lambda v: "-" if v is None else " / ".join(str(e) for e in v)   # noqa: E731
            f.write("| `%s` | %s | %s |\n" % (n, row(o), row(new[n])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", default=None, metavar="JSON")
    ap.add_argument("--render", default=None, metavar="JSON")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "margins.md"))
    ap.add_argument("--resources", nargs=2, default=None, metavar=("NEW_LOG", "PARENT_LOG"))
    ap.add_argument("--ab", default=None)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.measure:
        measure(a)
    if a.render:
        render(a)


if __name__ == "__main__":
    main()
