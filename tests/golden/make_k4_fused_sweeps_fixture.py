"""Record tests/golden/k4_fused_sweeps_mix32.npz: the host twin (parity build) on the bench mix -- 32 dispersed trajectories of seed
20261004 x 14 solve_steps with warm start (what tools/twin_mix.py 32 runs) -- and, next to it, the rounding-order yardstick of the
checkout it runs in: the distance between that checkout's own two builds of the same source, the parity build (-O2 -ffp-contract=off) and
the native one (-O3 -march=native, contraction on).  Run it AT THE COMMIT THE FIXTURE SPEAKS FOR (the parent of the change under test):
    python tests/golden/make_k4_fused_sweeps_fixture.py [out.npz]"""
import os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import oracle
from oracle import model, port


def run(native):
    oracle.use_native(native)
    p = model.base_prob_scaled()
    ic = model.disperse_ics(p, 32, 20261004)
    return port.scvx_steps(p, ic, p.imax - 1, warm_start=True)


def groups(a, b):
    """max |a - b| per component group: mass / position / velocity, quaternion / body rate, u, sigma"""
    return np.array([np.abs(a["x"][..., :7] - b["x"][..., :7]).max(), np.abs(a["x"][..., 7:] - b["x"][..., 7:]).max(),
                     np.abs(a["u"] - b["u"]).max(), np.abs(np.asarray(a["sigma"]) - np.asarray(b["sigma"])).max()])


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "k4_fused_sweeps_mix32.npz")
    par, nat = run(False), run(True)
    oracle.use_native(False)
    yard = groups(par, nat)
    same = np.array_equal(np.array(par["iters"]), np.array(nat["iters"])) and np.array_equal(np.array(par["rejected"]), np.array(nat["rejected"]))
    print("parity vs native build of this checkout: iteration counts and rejections identical: %s; |dx| mrv %.2e, qw %.2e, |du| %.2e, |dsigma| %.2e; %.2f its/solve"
          % (same, yard[0], yard[1], yard[2], yard[3], np.array(par["iters"]).mean()))
    np.savez_compressed(out, x=par["x"], u=par["u"], sigma=np.asarray(par["sigma"]), iters=np.array(par["iters"]).astype(np.int32),
                        rejected=np.array(par["rejected"]).astype(np.int8), yardstick=yard, yardstick_counts_identical=np.array(same))
    print("saved", out)
