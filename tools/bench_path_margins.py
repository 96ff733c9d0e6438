"""Path-constraint back-offs (mass, glide slope, tilt, rate): what they cost and what they buy.  Writes profiles/path_margins.md.

    python tools/bench_path_margins.py --measure out.json [--B 8192] [--repeats 5]                      (needs the GPU)
    python tools/bench_path_margins.py --render out.json --md profiles/path_margins.md [--resources NEW.log PARENT.log] [--ab AB.jsonl]

--measure:
  * robustify(constraints=("thrust", "tilt")) on the device's own converged plans of the flyable problem (the starts of
    tests/golden/oracle_flight_runs.npz): the six margins and the final mass before and after one round at nsigma = 3, the replan's
    step count and the largest back-offs;
  * at B (exo, dispersed batch): a solve_step under path back-offs of 5 % of each width beside one without, two batches from the same
    start, alternating single steps from scvx_batch_reset (the same subproblems every time), HIP events.
--render needs no GPU: the tables of --measure (or "not measured" where a table is missing), the compiler's resource report of every
conic kernel from two logs of `python -m successiveconvexification_amd.build --force -v` (this tree, its parent), and the headline of
bench.py from a file of "<label> <json line>" rows (label `parent` or `this`), alternating runs of the two libraries.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

COLS = ("N_MASS", "N_GLIDE", "N_TILT", "N_RATE", "N_TMAX", "N_TMIN")


def measure(a):
    import torch
    import cov_reference as cr
    from dataclasses import replace
    from successiveconvexification_amd import montecarlo as mc, sample_problems as sp
    from successiveconvexification_amd.batch import ScvxBatch
    from successiveconvexification_amd.dynamics import IntegratorCache
    res = {"device": torch.cuda.get_device_name(0), "B": a.B, "repeats": a.repeats}
    stat = lambda w: [float(np.median(w)), float(min(w)), float(max(w))]   # noqa: E731
    # ---- robustify on the device's own plans
    p = replace(sp.base_prob_scaled, mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    c = IntegratorCache(p, npts=10)
    ic = np.load(os.path.join(ROOT, "tests", "golden", "oracle_flight_runs.npz"))["ic"]
    base, rob = (ScvxBatch(c, ic.shape[0]).init(ic) for _ in range(2))
    st0, it0, _, _ = base.solve()
    rob.solve()
    S0 = np.stack([cr.handover_s0(x0, 0, 1e-3)[0] for x0 in base.trajectory()[0][:, 0]])
    before = base.covariance(S0)
    st, it, nu, dj, lo, hi = rob.robustify(S0, nsigma=3.0, rounds=1, constraints=("thrust", "tilt"))
    pm = rob.path_margins()
    after = rob.covariance(S0)
    plan = rob.flight_check(mode="plan")
    res["robustify"] = {"base_status": st0.tolist(), "base_steps": it0.tolist(), "status": st.tolist(), "replan_steps": it.tolist(),
                        "mass": [base.trajectory()[0][:, -1, 0].tolist(), rob.trajectory()[0][:, -1, 0].tolist()],
                        "thrust_backoff_max": lo.max(axis=1).tolist(), "tilt_backoff_max": pm[:, :, 2].max(axis=1).tolist(),
                        "G_TILT": np.asarray(plan.G_TILT).tolist(),
                        **{k: [getattr(before, k).tolist(), getattr(after, k).tolist()] for k in COLS}}
    for b in (base, rob):
        b.close()
    c.close()
    # ---- one solve_step at B, with and without path back-offs
    B, p = a.B, sp.base_prob_scaled
    ts = torch.cuda.Stream()
    c = IntegratorCache(p, npts=10)
    c.set_stream(ts.cuda_stream)
    icB = mc.disperse_ics(p, 0, B, 20261004)
    plain, marg = (ScvxBatch(c, B).init(icB) for _ in range(2))
    sqcm = float(np.sqrt((1 - np.cos(np.radians(p.thetaMax))) / 2))
    marg.set_path_margins(mass=0.05 * (p.mwet - p.mdry), glide=0.05 * float(icB[:, 0].min()), tilt=0.05 * sqcm, rate=0.05 * p.omMax)
    w = {"plain": [], "margined": []}
    for rnd in range(a.repeats + 1):
        for name, b in (("plain", plain), ("margined", marg)):
            b.reset()
            c.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record(ts)
            b.solve_step_async()
            t1.record(ts)
            torch.cuda.synchronize()
            if rnd:
                w[name].append(t0.elapsed_time(t1))
    res["solve_step_ms"] = {k: stat(v) for k, v in w.items()}
    res["solve_step_ipm_iters"] = {"plain": float(plain.solver_stats()[1].mean()), "margined": float(marg.solver_stats()[1].mean())}
    res["solve_step_status"] = {"plain": np.bincount(plain.flags()[0], minlength=8).tolist(), "margined": np.bincount(marg.flags()[0], minlength=8).tolist()}
    plain.close(), marg.close()
    c.set_stream(None)
    c.close()
    with open(a.measure, "w") as f:
        json.dump(res, f)
    print(json.dumps(res))


def render(a):
    from bench_margins import resources   # the parser of the compiler's remarks
    r = json.load(open(a.render)) if a.render != "none" else {}
    fmt = lambda v: "%.3f (%.3f .. %.3f)" % tuple(v)   # noqa: E731
    f = open(a.md, "w")
    f.write("# Path-constraint back-offs: mass, glide slope, tilt, rate\n\n`python tools/bench_path_margins.py`%s.\n\n"
            % ("; " + r["device"] if r else ""))
    if "robustify" in r:
        q = r["robustify"]
        f.write("## What one round of `robustify(constraints=(\"thrust\", \"tilt\"))` buys (flyable problem, the device's own converged plans from "
                "the starts of `tests/golden/oracle_flight_runs.npz`)\n\nnsigma = 3, cap = 0.25, S0 = `cov_reference.handover_s0(x0, 0, 1e-3)`, "
                "default weights; measured on the device.\n\n| | base plans | after one round |\n|---|---|---|\n")
        for k in COLS:
            f.write("| %s | %s | %s |\n" % (k, q[k][0], q[k][1]))
        f.write("| final mass | %s | %s |\n| SCvx steps | %s | %s |\n| status | %s | %s |\n| largest thrust back-off | | %s |\n| largest tilt back-off | | %s |\n"
                "| G_TILT of the flight check of the plan as flown (all samples: node 0, which has no back-off, and between nodes) | | %s |\n\n"
                % (q["mass"][0], q["mass"][1], q["base_steps"], q["replan_steps"], q["base_status"], q["status"], q["thrust_backoff_max"],
                   q["tilt_backoff_max"], q["G_TILT"]))
    else:
        f.write("## What one round of `robustify(constraints=(\"thrust\", \"tilt\"))` buys\n\nNot measured on the device yet.\n\n")
    f.write("The CPU reference (the independent oracle, `tests/golden/make_oracle_path_margin_runs.py`; CPU figures, not device figures): plan 0 "
            "solved from the straight-line guess under the tilt back-offs min(3 s_tilt, 0.25 sqcm) of its base plan takes 13 steps "
            "(arrrrrrraaaaa), ends at mass 0.903985 with N_TILT = 3.0 (base plan: 6.9e-5) and resolves the tightened cone to 6e-8.\n\n")
    if "solve_step_ms" in r:
        f.write("## Cost at B = %d (exo, K = 50), HIP events, median (min .. max) in ms\n\n| | ms |\n|---|---|\n" % r["B"])
        f.write("| first `solve_step` from `scvx_batch_reset`, no back-offs | %s |\n| the same under path back-offs of 5 %% of each width | %s |\n"
                % (fmt(r["solve_step_ms"]["plain"]), fmt(r["solve_step_ms"]["margined"])))
        ms, it = r["solve_step_ms"], r["solve_step_ipm_iters"]
        f.write("\n%d single steps each, alternating.  The margined step takes %.1f %% longer, far more than the spread of either row.  It is "
                "another subproblem: its interior-point method needs %.2f iterations per solve against %.2f (%.1f %% more; tightened cones "
                "are active where the plain ones are slack); the rest of the difference is not attributed by this tool.  "
                "The cost of the four set-up stores and of the four per-node loads of a cone pass, which a solve without back-offs pays "
                "too, shows in the headline below.  Step statuses (count per SCVX_ST_* value): %s without, %s with.\n\n"
                % (r["repeats"], 100.0 * (ms["margined"][0] / ms["plain"][0] - 1.0), it["margined"], it["plain"],
                   100.0 * (it["margined"] / it["plain"] - 1.0), r["solve_step_status"]["plain"], r["solve_step_status"]["margined"]))
    else:
        f.write("## Cost at B = 8192\n\nNot measured on the device yet.\n\n")
    if a.ab:
        rows, unit = {"parent": [], "this": []}, ""
        for line in open(a.ab):
            label, js = line.split(None, 1)
            j = json.loads(js)
            rows[label].append(float(j["value"]))
            unit = j.get("unit", unit)
        f.write("## Headline of `bench.py --gpus 1 --steps 14 --warmup 2`, the parent's library and this one alternating (rows in the order measured; "
                "a jump of both columns marks another session on another machine)\n\n| run | parent | this change |\n|---|---|---|\n")
        for i in range(max(len(rows["parent"]), len(rows["this"]))):
            f.write("| %d | %s | %s |\n" % (i + 1, *("%.1f" % rows[k][i] if i < len(rows[k]) else "" for k in ("parent", "this"))))
        f.write("| median | %.1f | %.1f |\n\nUnit: %s.\n\n" % (np.median(rows["parent"]), np.median(rows["this"]), unit))
    else:
        f.write("## Headline of `bench.py`, parent against this change\n\nNot measured yet: no file of alternating runs was given (`--ab`).\n\n")
    if a.resources:
        new, old = ({k: v for k, v in resources(log).items() if "socp" in k} for log in a.resources)
        f.write("## Compiler resource report of the conic kernels (gfx950, `-Rpass-analysis=kernel-resource-usage`)\n\nVGPRs / AGPRs / scratch bytes "
                "per lane / LDS bytes per block / waves per SIMD / spilled VGPRs.  The solver frame gains three pointers (the four path "
                "arrays behind one, the back-offs, and solve()'s `ic`, which the ladder of attempts now reads back from the frame): 16 bytes "
                "of LDS per wavefront after alignment.  Registers and occupancy are the parent's everywhere.  The two-wavefront kernels "
                "spill two more VGPRs in the kernel body (around the calls of the attempt ladder, once per solve attempt, never inside an "
                "interior-point iteration) and the double-tile ones take 16 more bytes of scratch; with `ic` held in registers across the "
                "ladder, as before, it was six more.  No routine of the solver spills: with four separate arrays `cone_map` did (four to six "
                "callee-saved registers), which is why a node's four values are interleaved in one 32-byte line.\n\n"
                "| kernel | parent | this change |\n|---|---|---|\n")
        row = lambda v: "-" if v is None else " / ".join(str(e) for e in v)   # noqa: E731
        for n in sorted(new):
            f.write("| `%s` | %s | %s |\n" % (n, row(old.get(n)), row(new[n])))
    f.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--measure", default=None, metavar="JSON")
    ap.add_argument("--render", default=None, metavar="JSON", help="the file --measure wrote, or `none`")
    ap.add_argument("--md", default=os.path.join(ROOT, "profiles", "path_margins.md"))
    ap.add_argument("--resources", nargs=2, default=None, metavar=("NEW_LOG", "PARENT_LOG"))
    ap.add_argument("--ab", default=None)
    ap.add_argument("--B", type=int, default=8192)
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    if a.measure:
        measure(a)
    if a.render:
        render(a)


if __name__ == "__main__":
    main()
