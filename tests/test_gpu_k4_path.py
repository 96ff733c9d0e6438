"""The conic kernel (K4: socp_kernel_t / socp_block_kernel) against its CPU twin ALONG the interior-point path, on the MI355X.

An interior-point method corrects itself: a Newton direction that is slightly wrong costs an iteration or two and lands on the same
flat optimum, so a comparison of finished solves (1e-6 / 2e-6 / "counts within 1" elsewhere in the suite) is next to blind to a bad
element of an MFMA fragment map, a coupling tile off at one end of the two-ended chain or a reduction that drops a lane.  Here every
solve is also stopped after n = 1, 2, 3, 4, 6, 8, 10, 12 iterations (scvx_solver_opts.max_iter = n, retries = 0: the best iterate so
far, status 1) and compared with the parity twin stopped at the same depth, on the DEVICE'S OWN linearisation (K1 does not enter).

Bounds, none of them taken from the device (tests/k4_path_reference.py, fixture tests/golden/k4_path_yardstick.npz written by
tests/golden/make_k4_path_yardstick.py from the twin alone; tests/test_k4_path_cpu.py keeps the fixture honest and holds the depth
lists):
  * truncated depths: status and iteration count equal the twin's; every group (dx, du, dsigma, nu absolute; merit, pobj relative)
    within max(10 Y(case, n, group), floor), Y = the larger of parity-vs-native build of the twin and parity twin vs itself on inputs
    perturbed by one ulp relative, floor = 2^-52 (K+1) (14+2NU+1) max|entry of the group| -- the first-order bound on re-ordering the
    longest sums the start point goes through (the depth-1 yardstick is 1e-16; the device contracts and sums in MFMA order).  The
    factor 10 is the convention of tests/test_k4_fused_sweeps_twin.py;
  * full depth (max_iter 60): status 0 on both sides; iteration counts equal the twin's, with the cap of the last test -- over all
    (case, executor, trajectory) triples at most 5 % may differ and none by more than 1 (the twin's two builds: 0 of 320);
    trajectories with equal counts meet 10 Y(case, full), those with another count the 1e-6 of test_gpu_scvx.py;
  * a trajectory the twin reports infeasible at node 1 (status 5; two of the eight starts of the fuzz class) is compared by status only.
The aero case uses the yardstick of a CPU aero linearisation (oracle.dynamics with the spline tables), not the exo K = 50 one.

Y per case as recorded (largest over the depths <= 12 | full depth), written out so that the bounds do not move with the file:

    case                      dx       du       dsigma   nu       merit    pobj    |  dx       du       dsigma   nu       merit    pobj
    exo K=50                  2.4e-10  6.1e-11  6.3e-11  8.5e-13  2.8e-09  4.3e-11 |  8.7e-10  9.2e-10  3.2e-11  1.0e-11  4.9e-04  2.3e-13
    exo K=4                   2.5e-10  5.4e-11  1.1e-11  8.2e-12  3.1e-07  5.9e-12 |  8.3e-09  1.8e-09  2.9e-10  8.2e-11  7.3e-05  8.6e-14
    exo K=8                   2.4e-10  4.7e-11  1.4e-11  2.9e-12  1.1e-06  1.3e-11 |  4.6e-10  8.5e-11  7.5e-11  9.9e-11  3.4e-04  1.1e-13
    exo K=9                   1.6e-10  3.3e-11  2.1e-11  4.2e-12  1.2e-06  1.9e-11 |  4.5e-10  5.6e-11  2.4e-11  4.5e-10  1.9e-04  8.3e-14
    exo K=31                  2.2e-10  1.2e-10  3.7e-11  2.4e-12  5.5e-08  3.7e-11 |  6.3e-10  4.2e-10  3.0e-11  1.5e-11  6.7e-05  3.4e-15
    fins K=50                 4.7e-10  2.2e-10  9.5e-11  1.3e-12  2.0e-08  4.7e-11 |  2.8e-10  3.2e-10  1.6e-11  1.4e-11  6.2e-05  2.8e-14
    fins K=9                  2.2e-10  4.6e-11  1.7e-11  6.1e-12  1.5e-06  1.9e-11 |  3.3e-09  6.2e-10  6.2e-11  2.0e-10  4.6e-04  1.5e-13
    fuzz class 3 (dp cone)    2.1e-12  8.6e-13  1.1e-11  3.2e-14  1.1e-09  3.7e-12 |  2.8e-10  2.8e-10  5.0e-11  2.5e-13  1.1e-05  4.0e-15
    float tiles               1.8e-10  5.2e-11  5.6e-11  8.4e-13  2.9e-09  4.9e-11 |  8.5e-10  9.0e-10  3.9e-11  1.1e-11  5.4e-04  2.6e-13
    aero K=50                 2.1e-10  6.8e-11  4.8e-11  8.6e-13  2.3e-09  4.0e-11 |  1.8e-09  1.9e-09  5.6e-11  2.2e-11  8.2e-04  3.9e-13
    thrust back-offs          8.9e-10  2.6e-10  6.7e-10  2.2e-12  8.3e-09  4.2e-10 |  5.4e-11  1.1e-11  1.9e-12  3.1e-14  1.2e-05  2.9e-14
    (all 11 cases x 9 depths: iteration counts and statuses identical between the twin's two builds)

Measured on one MI355X when the test was added (profiles/k4_path_parity.md): every status and truncated iteration count equal, 0 of 237 full
solves with another iteration count than the twin, worst distance / bound 0.37 (1 / 2 / 4 wavefronts: 0.22 / 0.37 / 0.33) -- the two-ended
executors need no bound of their own.

The device side of the comparison is tests/k4_path_device.py (shared with tests/test_gpu_endgame.py, which adds rules of its own for
finished solves; none applies here).
Every comparison prints its figures before it asserts (one markdown row per case, executor and depth: profiles/k4_path_parity.md)."""
import pytest

import k4_path_device as kd
import k4_path_reference as kp

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("waves", kd.WAVES)
@pytest.mark.parametrize("case", list(kp.CASES))
def test_device_takes_the_twins_path(case, waves, monkeypatch):
    monkeypatch.setenv("SCVX_K4_WAVES", waves)
    kd.check_path(case, waves)


def test_iteration_counts_of_full_solves_equal_the_twins_within_the_cap(monkeypatch):
    """over all (case, executor, trajectory) triples: at most 5 % of the full solves take another iteration count than the twin, and
    none differs by more than 1.  A condition, not a measurement: the twin's two builds differ in 0 of 320."""
    kd.check_counts(kp.CASES, monkeypatch)
