"""Regenerates tests/golden/oracle_endgame_runs.npz (layout: tests/endgame_reference.py): oracle.scvx.solve_problem re-run step by step
on runs that converge -- the flyable variant on the two starts of oracle_flight_runs.npz and its aero variant on the first of them,
tol 1e-8, nsub 10 -- with, per step, the pre-step state, the oracle's subproblem solution re-solved at 1e-9 and the CPU-only
distances TO / R of the conic solver's parity twin.  No GPU.  About 10 minutes.

    python tests/golden/make_oracle_endgame_runs.py

Asserted here: the exo runs end bit for bit on the x, u, sigma and steps of oracle_flight_runs.npz; every run converges; every rho
(of the run and of the re-solved subproblem) is at least 0.05 from rh0, rh1 and rh2, so that no accept / shrink / keep / grow decision
is a near-tie -- but for the steps of endgame_reference.NEAR_TIES, where the twin's rho must keep that clearance on the oracle's
side; the re-solved subproblem takes the run's decision."""
import os
import sys
from dataclasses import replace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import endgame_reference as er  # noqa: E402


def clearance(p, rho):
    return np.inf if np.isnan(rho) else min(abs(rho - t) for t in (p.rh0, p.rh1, p.rh2))


def one_run(run):
    from oracle import scvx
    po, ic = er.oracle_problem(run), er.start(run)
    it = scvx.create_initial(po, er.NSUB, ic[:3], ic[3:])
    p = it.problem
    cnu = cdel = np.inf
    n = 1
    iterates, rows = [], {k: [] for k in er.STEP_KEYS}
    sub32 = {k: [] for k in ("xr", "ur", "dsr", "nur", "pobj", "gap", "TO", "R")}
    while (p.nuTol < cnu or p.delTol < cdel) and n < p.imax:
        pre = it
        it, cnu, cdel = scvx.solve_step(pre, er.RUN_TOL)
        if not iterates or iterates[-1][0] is not pre.x:
            iterates.append((pre.x, pre.u, pre.sigma))
        accepted = it.x is not pre.x
        last = it.last
        status, ref = er.oracle_sub(pre, er.SUB_TOL)
        tol = er.SUB_TOL
        if status != "optimal":
            tol, ref = er.RUN_TOL, dict(xr=last["xr"], ur=last["ur"], dsr=last["dsr"], nur=last["nur"][1:].copy(), pobj=float(last["sol"].pobj), Jtr=last["Jtr"],
                                       gap=float(last["sol"].gap), pres=float(last["sol"].pres), dres=float(last["sol"].dres))
        fig = er.step_figures(po, pre, ref)
        run_rho = last.get("rho", np.nan)
        clear = min(clearance(p, run_rho), clearance(p, fig["rho"]))
        if clear < er.RHO_CLEARANCE:
            print("      NEAR-TIE: rho %.6f (run) %.6f (re-solved) within %.4f of a threshold" % (run_rho, fig["rho"], clear))
        assert np.isinf(fig["dJ"]) == (not accepted or np.isinf(pre.cost)), (run, n, fig, accepted)
        m = er.measure_step(po, ic, pre, ref, tol)
        if clear < er.RHO_CLEARANCE:     # only where tests/endgame_reference.py says why, and only with the twin clear and on the oracle's side
            trho = m["twin_step"][2]
            assert (run, n) in er.NEAR_TIES and clearance(p, trho) >= er.RHO_CLEARANCE, (run, n, run_rho, fig["rho"], trho)
            assert [trho < t for t in (p.rh0, p.rh1, p.rh2)] == [run_rho < t for t in (p.rh0, p.rh1, p.rh2)]
        else:
            assert (run, n) not in er.NEAR_TIES
        row = dict(rk=pre.rk, cost=pre.cost, iter=pre.iter, sub_tol=tol, tmin_nodes=er.tmin_nodes(po, ref["ur"]), accepted=accepted, next_rk=it.rk,
                   run_rho=run_rho, run_nu_norm=cnu, run_dJ=cdel, ipm_iters=last["sol"].iters, rho_clearance=clear, iterate_of=len(iterates) - 1, **ref, **fig, **m)
        for k in er.STEP_KEYS:
            rows[k].append(row[k])
        print("%s step %2d %s rk %-8.4g rho %-9.4g |nu| %.1e dJ %.1e Jtr %.3e Tmin nodes %2d ipm %2d twin %2d (status %d) sub_tol %.0e"
              % (run, n, "a" if accepted else "r", pre.rk, fig["rho"], fig["nu_norm"], fig["dJ"], ref["Jtr"], row["tmin_nodes"], last["sol"].iters,
                 m["twin_iters"], m["twin_status"], tol))
        print("      TO %s | R %s | step TO %s | step R %s" % tuple(" ".join("%.1e" % v for v in m[k]) for k in ("TO", "R", "step_TO", "step_R")))
        if run == "exo2" and n in er.SUB32_STEPS:
            it32 = replace(pre, deriv=pre.deriv.astype(np.float32).astype(np.float64))
            st32, r32 = er.oracle_sub(it32, tol)
            assert st32 == "optimal", st32
            m32 = er.measure_step(po, ic, pre, r32, tol, lin32=True)   # the twin rounds the tiles itself
            for k in ("xr", "ur", "dsr", "nur", "pobj", "gap"):
                sub32[k].append(r32[k])
            sub32["TO"].append(m32["TO"]), sub32["R"].append(m32["R"])
            print("      float tiles: TO %s | R %s" % (" ".join("%.1e" % v for v in m32["TO"]), " ".join("%.1e" % v for v in m32["R"])))
        n += 1
    assert cnu <= p.nuTol and cdel <= p.delTol, (run, cnu, cdel)
    out = {"%s_%s" % (run, k): np.array(v) for k, v in rows.items()}
    for k in ("accepted", "tmin_nodes", "ipm_iters", "twin_iters", "twin_status", "iterate_of", "iter"):
        out["%s_%s" % (run, k)] = out["%s_%s" % (run, k)].astype(np.int16)
    out.update({run + "_ic": ic, run + "_iterate_x": np.stack([i[0] for i in iterates]), run + "_iterate_u": np.stack([i[1] for i in iterates]),
                run + "_iterate_sigma": np.array([i[2] for i in iterates]), run + "_final_x": it.x, run + "_final_u": it.u, run + "_final_sigma": np.array(it.sigma)})
    if sub32["xr"]:
        out.update({"%s_sub32_%s" % (run, k): np.array(v) for k, v in sub32.items()})
    return out, it, len(rows["rk"])


def main():
    flight = np.load(os.path.join(HERE, "oracle_flight_runs.npz"))
    out = dict(runs=np.array(list(er.RUNS)), groups=np.array(er.GROUPS), step_groups=np.array(er.STEP_GROUPS), sub32_steps=np.array(er.SUB32_STEPS),
               nsub=np.array(er.NSUB), run_tol=np.array(er.RUN_TOL))
    for run, spec in er.RUNS.items():
        o, it, n = one_run(run)
        if spec["flight"] is not None:
            f = spec["flight"]
            assert np.array_equal(it.x, flight["x"][f]) and np.array_equal(it.u, flight["u"][f]) and it.sigma == flight["sigma"][f] and n == flight["steps"][f], run
            assert np.array_equal(o[run + "_ic"], flight["ic"][f])
        print("%s: converged in %d steps (%s), final mass %.6f" % (run, n, "".join("a" if a else "r" for a in o[run + "_accepted"]), it.x[-1, 0]))
        out.update(o)
    np.savez_compressed(er.FIXTURE, **out)
    print("wrote %s (%d bytes)" % (er.FIXTURE, os.path.getsize(er.FIXTURE)))


if __name__ == "__main__":
    main()
