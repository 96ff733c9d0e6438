"""The conic solver's host twin on the bench mix, against a record of the commit BEFORE kkt_solve's node-local passes were fused
into sweeps (Solver::front_sweep, csrc/scvx_ipm_core.hpp).  CPU only.

Workload: 32 dispersed trajectories of seed 20261004 x 14 solve_steps with warm start -- 448 conic solves, what tools/twin_mix.py 32
runs -- on the parity build of the twin (oracle.build(): -O2 -ffp-contract=off).  The fixture tests/golden/k4_fused_sweeps_mix32.npz
was written by tests/golden/make_k4_fused_sweeps_fixture.py in a checkout of the parent commit 0b8107b: final x, u, sigma, the
interior-point iteration count of every solve, every rejection.

Asserted: the same rejections and the same iteration count for every one of the 448 solves, and final iterates within 10 x the
solver's own rounding-order noise.  That noise is measured on the PARENT, not on the code under test: the distance between the
parent's two builds of one source, the parity build and the native one (-O3 -march=native, contraction on); the factor of 10 allows
for a different set of re-ordered sums than contraction touches, the exact-equality conditions carry the weight (the parent's own two
builds meet them).  Per component group, parent 0b8107b:

                                   where the change was specified     re-measured where the fixture was recorded
    mass / position / velocity     2.0e-10                            2.04e-10
    quaternion / body rate         2.7e-8                             2.67e-8
    u                              4.4e-9                             4.39e-9
    sigma                          6.4e-10                            6.44e-10
    (both: all 448 iteration counts and all rejections identical between the two builds; 11.13 iterations per solve)

The bounds below are 10 x the right-hand column, written out so that they do not move with the fixture file.  Measured with the front
sweep in place: every difference is exactly 0 -- the sweep keeps each row's order of summation, and the parity build does not
contract.  (The device library is compiled with contraction and is not bit-identical to its parent: over the 114,688 solves of the
benchmark's timed region it takes 1,277,282 interior-point iterations against 1,277,281, with identical rejections, warm starts and
failures -- profiles/k4_fused_sweeps.md, section 5.)"""
import os

import numpy as np

import oracle
from oracle import model, port

from conftest import GOLDEN

# 10 x (parity build vs native build of the parent commit), see the docstring
BOUND_MRV, BOUND_QW, BOUND_U, BOUND_SIGMA = 2.04e-9, 2.67e-7, 4.39e-8, 6.44e-9


def test_bench_mix_keeps_iteration_counts_rejections_and_iterates():
    g = np.load(os.path.join(GOLDEN, "k4_fused_sweeps_mix32.npz"))
    # the yardstick recorded with the fixture is the one the bounds were taken from
    assert bool(g["yardstick_counts_identical"])
    assert np.allclose(g["yardstick"] * 10.0, [BOUND_MRV, BOUND_QW, BOUND_U, BOUND_SIGMA], rtol=5e-3)
    oracle.use_native(False)
    p = model.base_prob_scaled()
    ic = model.disperse_ics(p, 32, 20261004)
    o = port.scvx_steps(p, ic, p.imax - 1, warm_start=True)
    its, rej = np.array(o["iters"]), np.array(o["rejected"])
    assert its.size == 448 and its.shape == g["iters"].shape
    d = [np.abs(o["x"][..., :7] - g["x"][..., :7]).max(), np.abs(o["x"][..., 7:] - g["x"][..., 7:]).max(),
         np.abs(o["u"] - g["u"]).max(), np.abs(np.asarray(o["sigma"]) - g["sigma"]).max()]
    print("iterations per solve %.2f (record %.2f), solves with another count %d, rejections differing %d; |dx| mrv %.2e qw %.2e |du| %.2e |dsigma| %.2e"
          % (its.mean(), g["iters"].mean(), int((its != g["iters"]).sum()), int((rej != g["rejected"]).sum()), d[0], d[1], d[2], d[3]))
    assert np.array_equal(rej.astype(np.int8), g["rejected"])
    assert np.array_equal(its.astype(np.int32), g["iters"])
    assert d[0] <= BOUND_MRV and d[1] <= BOUND_QW and d[2] <= BOUND_U and d[3] <= BOUND_SIGMA, d
