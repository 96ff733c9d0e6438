"""Regenerates tests/golden/oracle_audit_runs.npz: the CPU ORACLE hardened between the nodes by back-offs taken from the segment audit
(tests/audit_reference.py: flight_reference.chain in PLAN mode, the back-off rule in numpy, path_margin_reference.solve from
oracle.scvx.create_initial), for test_audit_cpu.py / test_gpu_audit.py.

    python tests/golden/make_oracle_audit_runs.py

For both plans of oracle_flight_runs.npz (the flyable problem of make_oracle_flight_runs.py), kinds thrust + tilt, gain 1.5, tol 1e-7,
cap 0.25, nsub 10, at most 4 rounds, every round FROM THE STRAIGHT-LINE GUESS under the accumulated back-offs (solver tol 1e-8):
  seg_<t>                      the base plan's audit [K][11]
  rounds_<t>                   the rounds the plan took until no selected G exceeds tol
  r<t>_<j>_lo, _pm             the back-offs of round j (thrust lo [K+1]; pm [K+1][4]; hi stays 0)
  r<t>_<j>_accepted, _cnu, _cdel, _rk   the step log of the round's run
  r<t>_<j>_x, _u, _sigma, _seg          the round's final plan and its audit
A run the oracle does not converge on is listed in `dropped_runs` with its verdict and ends that plan's rounds (a dropped run is never
replaced by anything else).  Numeric arrays only.  About 3 minutes.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

NSUB = 10
GAIN = 1.5
TOL = 1e-7
CAP = 0.25
KINDS = ("thrust", "tilt")
ROUNDS = 4


def main():
    import audit_reference as ar
    from make_oracle_flight_runs import flyable_problem
    from oracle import dynamics as od
    g = np.load(os.path.join(HERE, "oracle_flight_runs.npz"))
    p = flyable_problem()
    out, dropped = {}, []
    for t in range(g["x"].shape[0]):
        x, u, s, ic = g["x"][t], g["u"][t], float(g["sigma"][t]), g["ic"][t]
        done = []
        try:
            base, done = ar.harden(p, ic, x, u, s, KINDS, GAIN, TOL, CAP, NSUB, ROUNDS)
        except RuntimeError as e:
            print("plan %d: %s: dropped" % (t, e))
            dropped.append("plan %d: %s" % (t, e))
            base = ar.audit(od, p, x[None], u[None], np.array([s]), NSUB)[0][0]
        out["seg_%d" % t] = base
        out["rounds_%d" % t] = np.array(len(done))
        print("plan %d base: %s, mass %.6f" % (t, ar.violations(base, KINDS, TOL), x[-1, 0]))
        for j, r in enumerate(done):
            seq = "".join("a" if a else "r" for a in r["accepted"])
            print("plan %d round %d: %d steps (%s), %s, mass %.6f" % (t, j + 1, len(seq), seq, ar.violations(r["seg"], KINDS, TOL), r["x"][-1, 0]))
            out.update({"r%d_%d_%s" % (t, j, k): v for k, v in r.items()})
    np.savez(os.path.join(HERE, "oracle_audit_runs.npz"), nsub=np.array(NSUB), gain=np.array(GAIN), tol=np.array(TOL), cap=np.array(CAP),
             kinds=np.array([1, 0, 0, 1, 0], np.int8), dropped_runs=np.array(dropped if dropped else ["none"]), **out)


if __name__ == "__main__":
    main()
