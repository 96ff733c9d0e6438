"""Full Rocketland.solve_problem runs (14 solve_steps, tol 1e-8, npts 10) of the oracle's SCvx loop (oracle/scvx.py: socp.build, ipm.solve,
the trust-region rules) on the discretisation WITH the aerodynamic body torque (SCVX_MODEL_AERO_TORQUE, include/scvx.h).  oracle/ knows no
torque, so its `od` (oracle.dynamics) is replaced by the torch restatement tests/aero_torque_reference.py (automatic differentiation of
the segment map); everything else is the oracle's.

    python tests/golden/make_oracle_torque_runs.py [workers]

writes
    tests/golden/oracle_scvx_aero_torque_batch4_tol1e-08.npz    BASELINE configs[2] with the torque: aero, B = 256, seed 20261003
                                                                (model.disperse_ics streams), trajectories 0, 68, 161 and 255
    tests/golden/oracle_scvx_aerofin_torque_tol1e-08.npz         aero + fins + torque, K = 50, the problem's own initial condition
in the layout of oracle_scvx_aero_batch8_tol1e-08.npz: per trajectory and step the log (iteration counter, |nu|, |delta|, radius, cost,
sigma, rho) and the iterate x / u (sigma is log[..., 5])."""
import os
import sys
from multiprocessing import Pool
from unittest import mock

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

SEED, B, TOL, NSUB = 20261003, 256, 1e-8, 10
INDEX = [0, 68, 161, 255]
OUT_AERO = os.path.join(HERE, "oracle_scvx_aero_torque_batch4_tol1e-08.npz")
OUT_AEROFIN = os.path.join(HERE, "oracle_scvx_aerofin_torque_tol1e-08.npz")


def problem(fins):
    from oracle import model
    z = np.load(os.path.join(HERE, "lift_drag_tables.npz"))
    aero = model.AeroData(z["drag"], z["lift"], z["torque"])
    return model.base_prob_fin_scaled(aero) if fins else model.base_prob_scaled(aero)


def initial_conditions(p):
    from oracle import model
    return model.disperse_ics(p, B, SEED)[INDEX]


def run_steps(p, ic, nsteps, tol=TOL):
    """the oracle's create_initial + solve_step on the torque discretisation; returns log [n][7], xs [n][K+1][14], us [n][K+1][nu]"""
    import aero_torque_reference as ref
    from oracle import scvx
    log, xs, us = [], [], []
    with mock.patch.object(scvx, "od", ref.shim(torque=True)):
        it = scvx.create_initial(p, NSUB, ic[:3], ic[3:])
        for _ in range(nsteps):
            it, cnu, cdel = scvx.solve_step(it, tol)
            log.append((it.iter, cnu, cdel, it.rk, it.cost, it.sigma, float(it.last.get("rho", np.nan))))
            xs.append(it.x.copy())
            us.append(it.u.copy())
    return np.array(log), np.array(xs), np.array(us)


def run(job):
    fins, ic = job
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import torch
    torch.set_num_threads(1)
    p = problem(fins)
    log, xs, us = run_steps(p, ic, p.imax - 1)
    print("%s done: rk %s" % ("aero+fins+torque" if fins else "aero+torque", list(log[:, 3])), flush=True)
    return log, xs, us


if __name__ == "__main__":
    workers = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    pa, pf = problem(False), problem(True)
    ics = initial_conditions(pa)
    icf = np.concatenate([pf.rIi, pf.vIi])
    with Pool(workers) as pool:
        out = pool.map(run, [(False, ic) for ic in ics] + [(True, icf)], chunksize=1)
    np.savez_compressed(OUT_AERO, index=np.array(INDEX), ic=ics, log=np.array([o[0] for o in out[:4]]),
                        xs=np.array([o[1] for o in out[:4]]), us=np.array([o[2] for o in out[:4]]), tol=TOL, seed=SEED, B=B)
    np.savez_compressed(OUT_AEROFIN, index=np.array([-1]), ic=icf[None], log=out[4][0][None], xs=out[4][1][None], us=out[4][2][None],
                        tol=TOL, seed=-1, B=1)
    print("wrote", OUT_AERO, OUT_AEROFIN)
