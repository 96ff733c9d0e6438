"""Regenerates tests/golden/oracle_margin_runs.npz: the plans of oracle_flight_runs.npz solved again by the CPU ORACLE under
thrust-band back-offs (tests/margin_reference.py: oracle.socp.build with two edits of h, oracle.ipm, oracle.scvx.solve_step), for
test_margins_cpu.py / test_gpu_margins.py.

    python tests/golden/make_oracle_margin_runs.py

Problem: the flyable variant of make_oracle_flight_runs.py with that file's dispersed starts (the undispersed nominal start does not
converge on the oracle).  Per plan: S0 = cov_reference.handover_s0(x0, 0, 1e-3), gains = track_reference.gains at default weights,
psig from cov_reference.propagate (float64 and longdouble); back-offs lo_k = hi_k = min(3 s_T(k), 5e-3) of the BASE plan; then
  * "guess": solve_problem's loop from the straight-line guess under the back-offs (tol 1e-8, nsub 10),
  * "replan": the same loop from the converged base plan (trajectory kept, rk = 100, cost = Inf, iter = 0), at tol 1e-9: at 1e-8 the
    oracle's own interior-point method ends "max_iter" on the third subproblem of plan 0,
each with its per-step log and final x / u / sigma and the covariance report of the margined plan.  The two margined plans are
different local optima: nothing may compare them with each other.  Also stored: the oracle's solution (tol 1e-9) of the FIRST
subproblem under the back-offs at the straight-line guess, for the reference's model (on its double tiles, and on those tiles rounded
to float) and for the fin model (control_dim = 5, no
aerodynamics, nominal start, the back-offs of plan 0).  A plan on which the oracle does not converge under back-offs is left out
and named in `dropped`: plan 1 is (from the straight-line guess its interior-point method ends "kkt_singular").  About 2 minutes per plan and run.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

NSUB = 10
NSIGMA = 3.0
CLIP = 5.0e-3


def first_subproblem(mr, it, lo, hi):
    sol, ix = mr.solve_socp(it, lo, hi, tol=1e-9)
    assert sol.status == "optimal", sol.status
    z = sol.x
    return dict(x=z[ix.xv].T.copy(), u=z[ix.uv].T.copy(), dsig=float(z[ix.dsig]), nu=z[ix.nuv].T[1:].copy(), pobj=float(sol.pobj))


def main():
    import cov_reference as cr
    import margin_reference as mr
    import track_reference as tr
    from make_oracle_flight_runs import flyable_problem
    from oracle import dynamics as od, model, scvx
    g = np.load(os.path.join(HERE, "oracle_flight_runs.npz"))
    p = flyable_problem()
    K = p.K
    par = od.Params(p)
    X, U, S, IC = g["x"], g["u"], g["sigma"], g["ic"]
    out, kept, dropped = {}, [], []
    rows = {k: [] for k in ("lo", "hi", "psig", "psig_ld", "s0", "base_rep")}
    runs = {"guess": {k: [] for k in ("x", "u", "sigma", "rep", "psig")}, "replan": {k: [] for k in ("x", "u", "sigma", "rep", "psig")}}
    logs = {"guess": [], "replan": []}
    sub, sub32 = [], []
    for t in range(X.shape[0]):
        x, u, s = X[t:t + 1], U[t:t + 1], S[t:t + 1]
        _, d = od.linearize(par, x, u, s, 1.0 / (K + 1), NSUB)
        L, _ = tr.gains(d, K)
        S0, _ = cr.handover_s0(x[0, 0], 0, 1e-3)
        rep, cov, _ = cr.run(p, x, u, d, K, L, S0[None])
        ps = mr.path_sigma(p, x, u, cov)
        psld = mr.path_sigma(p, x, u, cr.propagate(d, K, L, S0[None], None, np.longdouble), np.longdouble)
        lo = hi = np.minimum(NSIGMA * ps[0, :, 4], CLIP)
        print("plan %d: base N_TMIN %.3g N_TMAX %.3g S_THRUST %.3g mass %.6f, back-offs up to %.3g"
              % (t, rep[0, cr.IDX["N_TMIN"]], rep[0, cr.IDX["N_TMAX"]], rep[0, cr.IDX["S_THRUST"]], x[0, -1, 0], lo.max()))
        res = {}
        try:
            it0 = scvx.create_initial(p, NSUB, IC[t, :3], IC[t, 3:])
            first = first_subproblem(mr, it0, lo, hi)
            # the same subproblem on derivative tiles rounded to float (scvx_batch_set_linearization_f32 rounds each entry once)
            from dataclasses import replace as _rep
            first32 = first_subproblem(mr, _rep(it0, deriv=it0.deriv.astype(np.float32).astype(np.float64)), lo, hi)
            for name, start, tol in (("guess", it0, 1e-8), ("replan", mr.restart(p, x[0], u[0], s[0], IC[t], NSUB), 1e-9)):
                it, cnu, cdel, log = mr.solve(start, lo, hi, tol=tol)
                if not (cnu <= p.nuTol and cdel <= p.delTol):
                    raise RuntimeError("%s: imax reached at |nu| = %.3e, dJ = %.3e" % (name, cnu, cdel))
                _, dm = od.linearize(par, it.x[None], it.u[None], np.array([it.sigma]), 1.0 / (K + 1), NSUB)
                Lm, _ = tr.gains(dm, K)
                S0m, _ = cr.handover_s0(it.x[0], 0, 1e-3)
                rm, cm, _ = cr.run(p, it.x[None], it.u[None], dm, K, Lm, S0m[None])
                bl, bh = mr.band_margins(p, it.u, lo, hi)
                print("plan %d %s: %d steps (%s), band held to %.1e / %.1e, mass %.6f, N_TMIN %.3f N_TMAX %.3f"
                      % (t, name, len(log), "".join("a" if e["accepted"] else "r" for e in log), -min(bl, 0), -min(bh, 0), it.x[-1, 0],
                         rm[0, cr.IDX["N_TMIN"]], rm[0, cr.IDX["N_TMAX"]]))
                res[name] = (it, log, rm[0], mr.path_sigma(p, it.x[None], it.u[None], cm)[0])
        except RuntimeError as e:   # the oracle's own verdict (a non-optimal conic solve, or imax): anything else is a bug here
            print("plan %d: the oracle does not converge under back-offs (%s): left out" % (t, e))
            dropped.append(t)
            continue
        kept.append(t)
        sub.append(first)
        sub32.append(first32)
        for k, v in (("lo", lo), ("hi", hi), ("psig", ps[0]), ("psig_ld", psld[0].astype(np.float64)), ("s0", S0), ("base_rep", rep[0])):
            rows[k].append(v)
        for name, (it, log, rm, pm) in res.items():
            for k, v in (("x", it.x), ("u", it.u), ("sigma", it.sigma), ("rep", rm), ("psig", pm)):
                runs[name][k].append(v)
            logs[name].append(log)
    out.update({k: np.stack(v) for k, v in rows.items()})
    for name in runs:
        out.update({"%s_%s" % (name, k): np.stack(v) for k, v in runs[name].items()})
        n = max(len(l) for l in logs[name])
        acc = np.full((len(kept), n), -1, np.int8)          # 1 accepted, 0 rejected, -1 past the end
        cnu, cdel, rk = (np.full((len(kept), n), np.nan) for _ in range(3))
        for i, l in enumerate(logs[name]):
            for j, e in enumerate(l):
                acc[i, j], cnu[i, j], cdel[i, j], rk[i, j] = e["accepted"], e["cnu"], e["cdel"], e["rk"]
        out.update({"%s_accepted" % name: acc, "%s_cnu" % name: cnu, "%s_cdel" % name: cdel, "%s_rk" % name: rk})
    for k in ("x", "u", "dsig", "nu", "pobj"):
        out["sub_%s" % k] = np.stack([np.asarray(f[k]) for f in sub])
        out["sub32_%s" % k] = np.stack([np.asarray(f[k]) for f in sub32])
    # the fin model's first subproblem (control_dim = 5, no aerodynamics) at its nominal straight-line guess, back-offs of plan 0
    pf = model.base_prob_fin_scaled()
    ff = first_subproblem(mr, scvx.create_initial(pf, NSUB), rows["lo"][0], rows["hi"][0])
    out.update({"fin_%s" % k: np.asarray(v) for k, v in ff.items()})
    np.savez(os.path.join(HERE, "oracle_margin_runs.npz"), plans=np.array(kept), dropped=np.array(dropped, int), ic=IC[kept],
             base_x=X[kept], base_u=U[kept], base_sigma=S[kept], nsigma=np.array(NSIGMA), clip=np.array(CLIP), nsub=np.array(NSUB), **out)


if __name__ == "__main__":
    main()
