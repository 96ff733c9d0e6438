"""Regenerates tests/golden/oracle_nav_margin_runs.npz: the per-node standard deviations of the path functions under NAVIGATION errors
for the plans of oracle_flight_runs.npz, and the plans replanned by the CPU ORACLE (tests/margin_reference.py) under thrust-band
back-offs taken from them and, beside, from the covariance analysis -- for test_nav_margins_cpu.py / test_gpu_nav_margins.py.

    python tests/golden/make_oracle_nav_margin_runs.py

Problem: the flyable variant of make_oracle_flight_runs.py.  Per plan: S0 = cov_reference.handover_s0(x0, 0, 1e-3), the navigation
handover N0 = S0, gains = track_reference.gains at default weights, POSITION ONLY measured at every node
(nav_margin_reference.position_model of plan 0's start, shared by the plans as H and rm are shared by a batch).  Stored: S0, N0, H, rm,
the navigation psig (float64 and longdouble) and the covariance psig of every plan; then, per plan the oracle converges on, two
thrust-only replans from the converged plan (margin_reference.solve from margin_reference.restart, tol 1e-9) under
lo_k = hi_k = min(3 s_T(k), 0.25 (Tmax - Tmin)), "nav" with the navigation s_T and "cov" with the covariance s_T of the base plan, each
with its accept / reject log, final x / u / sigma and BOTH reports (navigation and covariance) of the replanned plan.  A plan on
which the oracle does not converge under either set is left out of the replans and named in `dropped`.  Thrust + tilt + rate replans are
not asked for: from the converged plan the oracle's own interior-point method ends "kkt_singular" / "max_iter" on both plans.
About a minute per plan.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

NSUB = 10
NSIGMA = 3.0
CAP = 0.25


def main():
    import cov_reference as cr
    import margin_reference as mr
    import nav_margin_reference as nm
    import nav_reference as nr
    import track_reference as tr
    from make_oracle_flight_runs import flyable_problem
    from oracle import dynamics as od
    g = np.load(os.path.join(HERE, "oracle_flight_runs.npz"))
    p = flyable_problem()
    K = p.K
    par = od.Params(p)
    X, U, S, IC = g["x"], g["u"], g["sigma"], g["ic"]
    B = X.shape[0]
    H, rm = nm.position_model(X[0, 0])
    _, D = od.linearize(par, X, U, S, 1.0 / (K + 1), NSUB)
    L, _ = tr.gains(D, K)
    S0 = np.stack([cr.handover_s0(X[t, 0], 0, 1e-3)[0] for t in range(B)])
    N0 = S0.copy()
    ps_nav = nm.path_sigma(p, X, U, D, K, L, S0, N0, H, rm)
    ps_nav_ld = nm.path_sigma(p, X, U, D, K, L, S0, N0, H, rm, dtype=np.longdouble)
    ps_cov = mr.path_sigma(p, X, U, cr.propagate(D, K, L, S0))
    base_nav = nr.run(p, X, U, D, K, L, S0, N0, H, rm)
    base_cov = cr.run(p, X, U, D, K, L, S0)[0]
    for t in range(B):
        r = ps_nav[t, 1:] / np.where(ps_cov[t, 1:] > 0, ps_cov[t, 1:], np.nan)
        print("plan %d: navigation / covariance s, mean over nodes: thrust %.2f (max %.1f) tilt %.2f; expected outside of the band per 256 "
              "flights: %.0f" % (t, np.nanmean(r[:, 4]), np.nanmax(r[:, 4]), np.nanmean(r[:, 2]), nm.outside_band(p, U[t], ps_nav[t])))
    kept, dropped = [], []
    runs = {k: {f: [] for f in ("x", "u", "sigma", "lo", "navrep_cov", "navrep_nav", "covrep", "psig_nav", "outside")} for k in ("nav", "cov")}
    logs = {"nav": [], "cov": []}
    for t in range(B):
        res = {}
        try:
            for name, ps in (("nav", ps_nav), ("cov", ps_cov)):
                lo = nm.backoffs(p, ps[t], NSIGMA, CAP)
                it, cnu, cdel, log = mr.solve(mr.restart(p, X[t], U[t], S[t], IC[t], NSUB), lo, lo, tol=1e-9)
                if not (cnu <= p.nuTol and cdel <= p.delTol):
                    raise RuntimeError("%s: imax reached at |nu| = %.3e, dJ = %.3e" % (name, cnu, cdel))
                x1, u1 = it.x[None], it.u[None]
                _, d1 = od.linearize(par, x1, u1, np.array([it.sigma]), 1.0 / (K + 1), NSUB)
                L1, _ = tr.gains(d1, K)
                nav1 = nr.run(p, x1, u1, d1, K, L1, S0[t:t + 1], N0[t:t + 1], H, rm)
                cov1 = cr.run(p, x1, u1, d1, K, L1, S0[t:t + 1])[0]
                ps1 = nm.path_sigma(p, x1, u1, d1, K, L1, S0[t:t + 1], N0[t:t + 1], H, rm)[0]
                out = nm.outside_band(p, it.u, ps1)
                print("plan %d under %s back-offs (up to %.3g): %d steps (%s), mass %.6f; navigation report N_TMIN %.2f N_TMAX %.2f, covariance "
                      "report %.2f / %.2f; expected outside %.0f"
                      % (t, name, lo.max(), len(log), "".join("a" if e["accepted"] else "r" for e in log), it.x[-1, 0],
                         nav1["report"][0, cr.IDX["N_TMIN"]], nav1["report"][0, cr.IDX["N_TMAX"]], cov1[0, cr.IDX["N_TMIN"]],
                         cov1[0, cr.IDX["N_TMAX"]], out))
                res[name] = (log, dict(x=it.x, u=it.u, sigma=it.sigma, lo=lo, navrep_cov=nav1["report"][0], navrep_nav=nav1["navrep"][0],
                                       covrep=cov1[0], psig_nav=ps1, outside=out))
        except RuntimeError as e:   # the oracle's own verdict (a non-optimal conic solve, or imax): anything else is a bug here
            print("plan %d: the oracle does not converge under back-offs (%s): left out" % (t, e))
            dropped.append(t)
            continue
        kept.append(t)
        for name, (log, vals) in res.items():
            logs[name].append(log)
            for k, v in vals.items():
                runs[name][k].append(v)
    out = {}
    for name in runs:
        out.update({"%s_%s" % (name, k): np.stack(v) for k, v in runs[name].items()})
        n = max(len(l) for l in logs[name])
        acc = np.full((len(kept), n), -1, np.int8)          # 1 accepted, 0 rejected, -1 past the end
        cnu, cdel, rk = (np.full((len(kept), n), np.nan) for _ in range(3))
        for i, l in enumerate(logs[name]):
            for j, e in enumerate(l):
                acc[i, j], cnu[i, j], cdel[i, j], rk[i, j] = e["accepted"], e["cnu"], e["cdel"], e["rk"]
        out.update({"%s_accepted" % name: acc, "%s_cnu" % name: cnu, "%s_cdel" % name: cdel, "%s_rk" % name: rk})
    np.savez(os.path.join(HERE, "oracle_nav_margin_runs.npz"), plans=np.array(kept), dropped=np.array(dropped, int), ic=IC, base_x=X,
             base_u=U, base_sigma=S, S0=S0, N0=N0, H=H, rm=rm, psig_nav=ps_nav, psig_nav_ld=ps_nav_ld.astype(np.float64), psig_cov=ps_cov,
             base_navrep_cov=base_nav["report"], base_navrep_nav=base_nav["navrep"], base_covrep=base_cov,
             base_outside=np.array([nm.outside_band(p, U[t], ps_nav[t]) for t in range(B)]),
             nsigma=np.array(NSIGMA), cap=np.array(CAP), nsub=np.array(NSUB), **out)


if __name__ == "__main__":
    main()
