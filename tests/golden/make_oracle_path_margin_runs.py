"""Regenerates tests/golden/oracle_path_margin_runs.npz: the CPU ORACLE under path-constraint back-offs (tests/path_margin_reference.py:
oracle.socp.build with the edits of b and h, oracle.ipm, oracle.scvx.solve_step), for test_path_margins_cpu.py /
test_gpu_path_margins.py.

    python tests/golden/make_oracle_path_margin_runs.py
    python tests/golden/make_oracle_path_margin_runs.py --k100     # oracle_path_margin_k100.npz only: group "k100" of step 1 at K = 100

Problem: the flyable variant of make_oracle_flight_runs.py with that file's dispersed starts.

1. FIRST SUBPROBLEMS at the straight-line guess (tol 1e-9), in four groups of three trajectories with different back-offs each:
   "k50" (the reference's model, K = 50), "k50f" (the same on derivative tiles rounded to float), "fin" (control_dim = 5, mdry = 0.55 and tf_guess = 8 as in the flyable variant) and "k9"
   (K = 9: odd, so a two-ended factorisation has a middle node).  The back-offs are chosen from the oracle's solution of the
   UNMARGINED subproblem: per kind, at the admissible node with the smallest slack (node K/2 for the mass), the back-off is that
   slack plus an excess (a fraction of the row's width, at most half of the norm it bounds), so the unmargined optimum violates the
   tightened row and -- the problem being convex -- the tightened
   optimum has it active.  That every kind is active at one node or more (tightened slack < 1e-7) is asserted.  If the oracle does
   not solve all four kinds at once for a start, that start is solved once per kind instead, and the dropped attempt is recorded.
2. A COMPLETE RUN of plan 0 from the straight-line guess (tol 1e-8, nsub 10) under the tilt back-offs t_k = min(3 s_tilt(k),
   0.25 sqcm) of the BASE plan (s_tilt from cov_reference at the handover covariance handover_s0(x0, 0, 1e-3), default weights), with
   its per-step log, the final iterate, the accuracy to which the run resolves the tightened cone (|smallest slack|, `viol`) and the
   covariance report of the margined plan.  Plan 1 is run the same way and kept if the oracle converges on it.

The oracle's own interior-point method is fragile under back-offs: the runs attempted and dropped are listed in `dropped_runs` with
the oracle's verdict (a dropped run is never replaced by anything else).  About 10 minutes in all.
"""
import os
import sys
from dataclasses import replace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

NSUB = 10
NSIGMA = 3.0
CAP = 0.25
ACTIVE = 1e-7
# how far past the unmargined optimum's slack a back-off goes, per kind (mass, glide, tilt, rate), as a fraction of the width
EXCESS = (0.02, 0.05, 0.05, 0.05)


def first_subproblem(pr, it, pm):
    sol, ix = pr.solve_socp(it, pm, tol=1e-9)
    if sol.status != "optimal":
        raise RuntimeError(sol.status)
    z = sol.x
    return dict(x=z[ix.xv].T.copy(), u=z[ix.uv].T.copy(), dsig=float(z[ix.dsig]), nu=z[ix.nuv].T[1:].copy(), pobj=float(sol.pobj))


def choose(pr, p, x0, kinds, shift):
    """back-offs for `kinds` from the unmargined solution x0; shift moves the chosen node along the ranking (different per trajectory)"""
    K = p.K
    tggs, sqcm = pr.consts(p)
    s = pr.slacks(p, x0)
    width = (p.mwet - p.mdry, None, sqcm, p.omMax)
    pm = np.zeros((K + 1, 4))
    for c in kinds:
        if c == pr.MASS:
            k = K // 2 + shift
            pm[k, c] = s[k, c] + min(EXCESS[c] * width[c], 0.5 * (p.mwet - x0[k, 0]))   # at most half of the propellant burnt by then
            continue
        lo = 0 if c == pr.TILT else 1
        sl = {pr.GLIDE: slice(2, 4), pr.TILT: slice(9, 11), pr.RATE: slice(11, 14)}[c]
        nrm = np.linalg.norm(x0[:, sl], axis=1)
        w = x0[:, 1] / tggs if c == pr.GLIDE else np.full(K + 1, width[c])
        k = sorted(range(lo, K), key=lambda k: s[k, c])[shift]
        # the new bound lies inside the unmargined optimum's norm at that node, and never beyond its half: the tightened cone keeps its axis
        pm[k, c] = s[k, c] + min(EXCESS[c] * w[k], 0.5 * nrm[k])
    return pr.check_contract(p, pm)


def group(pr, scvx, p, ics, name, dropped, f32=False):
    """the cases of one group: list of dict(ic, pm, x, u, dsig, nu, pobj)"""
    cases = []
    for t, ic in enumerate(ics):
        it = scvx.create_initial(p, NSUB, ic[:3], ic[3:])
        if f32:
            it = replace(it, deriv=it.deriv.astype(np.float32).astype(np.float64))
        free = first_subproblem(pr, it, np.zeros((p.K + 1, 4)))
        tries = [tuple(range(4))] + [(c,) for c in range(4)]
        for kinds in tries:
            pm = choose(pr, p, free["x"], kinds, t)
            try:
                sol = first_subproblem(pr, it, pm)
                s = pr.slacks(p, sol["x"], pm)
                act = [bool(((s[:, c] < ACTIVE) & (pm[:, c] > 0)).any()) for c in kinds]   # active at a node that has a back-off
                if not all(act):
                    raise RuntimeError("not every kind active: %s" % act)
            except RuntimeError as e:
                print("%s start %d kinds %s: %s: dropped" % (name, t, kinds, e))
                dropped.append("%s start %d kinds %s: %s" % (name, t, "".join(pr.KINDS[c][0] for c in kinds), e))
                if len(kinds) == 4:
                    continue
                raise
            print("%s start %d kinds %s: optimal, smallest tightened slacks %s, moved x by %.3e, violation %.1e"
                  % (name, t, kinds, s.min(axis=0), np.abs(sol["x"] - free["x"]).max(), -min(s.min(), 0)))
            assert np.abs(sol["x"] - free["x"]).max() > 1e-4
            cases.append(dict(ic=np.asarray(ic, float), pm=pm, kinds=sum(1 << c for c in kinds), **sol))
            if len(kinds) == 4:
                break
    return cases


def main():
    import cov_reference as cr
    import margin_reference as mr
    import path_margin_reference as pr
    import track_reference as tr
    from make_oracle_flight_runs import flyable_problem
    from oracle import dynamics as od, model, scvx
    g = np.load(os.path.join(HERE, "oracle_flight_runs.npz"))
    p = flyable_problem()
    K = p.K
    out, dropped = {}, []
    ics = np.concatenate([g["ic"], np.concatenate([p.rIi, p.vIi])[None]])
    pf = replace(model.base_prob_fin_scaled(), mdry=0.55, tf_guess=8.0)   # the fin model made flyable like the other: the sample's mwet - mdry is 1e-3
    p9 = replace(p, K=9)
    for name, prob, starts, f32 in (("k9", p9, ics, False), ("k50", p, ics, False), ("k50f", p, ics, True),
                                    ("fin", pf, np.concatenate([np.concatenate([pf.rIi, pf.vIi])[None], model.disperse_ics(pf, 2, 7)]), False)):
        cases = group(pr, scvx, prob, starts, name, dropped, f32)
        for k in ("ic", "pm", "kinds", "x", "u", "dsig", "nu", "pobj"):
            out["%s_%s" % (name, k)] = np.stack([np.asarray(c[k]) for c in cases])
    # ---- the complete run: plan 0 under the tilt back-offs of the base plan
    par = od.Params(p)
    X, U, S, IC = g["x"], g["u"], g["sigma"], g["ic"]
    for t in range(X.shape[0]):
        x, u, s = X[t:t + 1], U[t:t + 1], S[t:t + 1]
        _, d = od.linearize(par, x, u, s, 1.0 / (K + 1), NSUB)
        L, _ = tr.gains(d, K)
        S0, _ = cr.handover_s0(x[0, 0], 0, 1e-3)
        rep, cov, _ = cr.run(p, x, u, d, K, L, S0[None])
        ps = mr.path_sigma(p, x, u, cov)
        pm = pr.margins_from_sigma(p, x[0], ps[0], NSIGMA, CAP, ("tilt",))
        print("plan %d: base N_TILT %.3g N_GLIDE %.3g N_RATE %.3g N_MASS %.3g, largest s_tilt %.3g, tilt back-offs up to %.3g"
              % (t, rep[0, cr.IDX["N_TILT"]], rep[0, cr.IDX["N_GLIDE"]], rep[0, cr.IDX["N_RATE"]], rep[0, cr.IDX["N_MASS"]], ps[0, :, 2].max(),
                 pm[:, 2].max()))
        out["base_rep_%d" % t] = rep[0]
        out["base_psig_%d" % t] = ps[0]
        try:
            it, cnu, cdel, log = pr.solve(scvx.create_initial(p, NSUB, IC[t, :3], IC[t, 3:]), pm, tol=1e-8)
            if not (cnu <= p.nuTol and cdel <= p.delTol):
                raise RuntimeError("imax reached at |nu| = %.3e, dJ = %.3e" % (cnu, cdel))
        except RuntimeError as e:
            print("plan %d from the guess under tilt back-offs: %s: dropped" % (t, e))
            dropped.append("plan %d from the guess under tilt back-offs: %s" % (t, e))
            continue
        _, dm = od.linearize(par, it.x[None], it.u[None], np.array([it.sigma]), 1.0 / (K + 1), NSUB)
        Lm, _ = tr.gains(dm, K)
        S0m, _ = cr.handover_s0(it.x[0], 0, 1e-3)
        rm, _, _ = cr.run(p, it.x[None], it.u[None], dm, K, Lm, S0m[None])
        # How exactly the oracle's own run resolves the tightened cone: the distance of its most active node from the boundary.  An
        # interior-point iterate sits inside (a positive slack), so this is an accuracy, not an excess; the tests allow the device
        # ten times as much on the other side.
        viol = float(abs(pr.slacks(p, it.x, pm)[:, pr.TILT].min()))
        seq = "".join("a" if e["accepted"] else "r" for e in log)
        print("plan %d: %d steps (%s), tightened tilt cone resolved to %.1e, mass %.6f, N_TILT %.3f"
              % (t, len(log), seq, viol, it.x[-1, 0], rm[0, cr.IDX["N_TILT"]]))
        out.update({"run%d_%s" % (t, k): v for k, v in (
            ("ic", IC[t]), ("pm", pm), ("s0", S0), ("x", it.x), ("u", it.u), ("sigma", np.array(it.sigma)), ("rep", rm[0]),
            ("viol", np.array(viol)), ("accepted", np.array([e["accepted"] for e in log], np.int8)),
            ("cnu", np.array([e["cnu"] for e in log])), ("cdel", np.array([e["cdel"] for e in log])), ("rk", np.array([e["rk"] for e in log])))})
    assert "run0_x" in out, "the run of plan 0 under tilt back-offs must be kept"
    np.savez(os.path.join(HERE, "oracle_path_margin_runs.npz"), nsigma=np.array(NSIGMA), cap=np.array(CAP), nsub=np.array(NSUB),
             dropped_runs=np.array(dropped if dropped else ["none"]), **out)


K100_KEYS = ("ic", "pm", "kinds", "x", "u", "dsig", "nu", "pobj")


def main_k100():
    """group "k100" alone (replace(p, K=100), the three starts of "k50"), into oracle_path_margin_k100.npz: oracle_path_margin_runs.npz
    is neither read for its groups nor written.  About 3 minutes."""
    import path_margin_reference as pr
    from make_oracle_flight_runs import flyable_problem
    from oracle import scvx
    g = np.load(os.path.join(HERE, "oracle_flight_runs.npz"))
    p = flyable_problem()
    ics = np.concatenate([g["ic"], np.concatenate([p.rIi, p.vIi])[None]])
    dropped = []
    cases = group(pr, scvx, replace(p, K=100), ics, "k100", dropped)
    assert not dropped and len(cases) == 3, dropped
    np.savez(os.path.join(HERE, "oracle_path_margin_k100.npz"),
             **{"k100_%s" % k: np.stack([np.asarray(c[k]) for c in cases]) for k in K100_KEYS})


if __name__ == "__main__":
    if sys.argv[1:] == ["--k100"]:
        main_k100()
    else:
        main()
