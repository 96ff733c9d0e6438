"""Regenerates tests/golden/oracle_flight_runs.npz: two plans the CPU ORACLE itself converges on, and the reference flight reports
of both (tests/flight_reference.py), for test_gpu_flight.py / test_flight_cpu.py.

    python tests/golden/make_oracle_flight_runs.py

The problem is the flyable variant of test_flyable_problem_converges (mdry = 0.55, nuTol = 1e-6, delTol = 1e-3, imax = 40,
tf_guess = 8) with model.disperse_ics(p, 4, 7); oracle.scvx.solve_problem at tol 1e-8, nsub 10.  Trajectories 2 and 3 are kept:
on 0 and 1 of that seed the oracle's own interior-point solver ends "stalled" / "max_iter".  About 40 s per run.
"""
import os
import sys
from dataclasses import replace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

KEEP = (2, 3)
NSUB = 10


def flyable_problem():
    from oracle import model
    return replace(model.base_prob_scaled(), mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)


def main():
    import flight_reference as fr
    from oracle import dynamics as od, model, scvx
    p = flyable_problem()
    ic = model.disperse_ics(p, 4, 7)
    xs, us, ss, iters = [], [], [], []
    for t in KEEP:
        log = []
        it, cnu, cdel = scvx.solve_problem(p, nsub=NSUB, rIi=ic[t, :3], vIi=ic[t, 3:], tol=1e-8, log=log)
        assert cnu <= p.nuTol and cdel <= p.delTol, (t, cnu, cdel)
        print("trajectory %d: converged in %d steps, |nu| = %.3e, dJ = %.3e" % (t, len(log), cnu, cdel))
        xs.append(it.x), us.append(it.u), ss.append(it.sigma), iters.append(len(log))
    x, u, sigma = np.stack(xs), np.stack(us), np.array(ss)
    rs, _ = fr.fly(od, p, x, u, sigma, NSUB, fr.SHOOT)
    rp, _ = fr.fly(od, p, x, u, sigma, NSUB, fr.PLAN)
    r40, _ = fr.fly(od, p, x, u, sigma, 40, fr.SHOOT)
    for name, r in (("SHOOT", rs), ("PLAN", rp), ("SHOOT nsub 40", r40)):
        print(name, "GAP", r[:, fr.IDX["GAP"]], "G_TMIN", r[:, fr.IDX["G_TMIN"]])
    np.savez(os.path.join(HERE, "oracle_flight_runs.npz"), x=x, u=u, sigma=sigma, ic=ic[list(KEEP)], steps=np.array(iters),
             report_shoot=rs, report_plan=rp, report_shoot_nsub40=r40, nsub=np.array(NSUB))


if __name__ == "__main__":
    main()
