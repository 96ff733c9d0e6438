"""Writes tests/golden/k0_path_yardstick.npz: the yardstick of the 3-DoF initialiser's interior-point path comparison
(tests/k0_path_reference.py), from the CPU twin alone -- its parity build against its native build and against itself on starts
perturbed by one ulp relative -- with the twin's statuses and iteration counts per depth for both builds and the magnitudes of each
group.  No GPU, seconds.
    python tests/golden/make_k0_path_yardstick.py
It refuses to write unless the twin's own two builds meet the iteration-count rule the device is held to (full solves of the cases with
K >= 3: at most 5 % with another count, none by more than 1) and agree on every status outside K = 1 and 2.  A full-depth distance
is taken over the starts on which the two runs compared end with the same status after the same number of iterations; the full-depth
row of K = 1 and 2 is written for the reader only (k0_path_reference.TINY)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import k0_path_reference as kp  # noqa: E402


def main():
    out = dict(depths=np.array(kp.DEPTHS), groups=np.array(kp.GROUPS), cases=np.array(list(kp.CASES)))
    pairs = []
    for case in kp.CASES:
        m = kp.measure(case)
        k = kp.key(case)
        for name in ("native", "perturb", "mag"):
            out[name + "_" + k] = m[name]
        for name in ("iters", "native_iters"):
            out[name + "_" + k] = m[name].astype(np.int16)
        for name in ("status", "native_status"):
            out[name + "_" + k] = m[name].astype(np.int8)
        same = np.array_equal(m["iters"], m["native_iters"]) and np.array_equal(m["status"], m["native_status"])
        Y = np.maximum(m["native"], m["perturb"])
        print("%-14s counts and statuses identical between the builds: %s; full depth: statuses %s / %s, iterations %s / %s"
              % (case, same, m["status"][-1], m["native_status"][-1], m["iters"][-1], m["native_iters"][-1]))
        print("    groups    %s" % " ".join("%-7s" % g for g in kp.GROUPS))
        for i, n in enumerate(kp.DEPTHS):
            print("    depth %2d  %s   (iterations %s / %s)" % (n, " ".join("%.1e" % v for v in Y[i]), m["iters"][i], m["native_iters"][i]))
        if case in kp.COUNTED:
            assert np.array_equal(m["status"], m["native_status"]), (case, m["status"], m["native_status"])
            assert np.all(m["status"][-1] == 0), (case, m["status"][-1])
            pairs += list(zip(m["iters"][-1], m["native_iters"][-1]))
        else:
            assert np.all(np.isin(m["status"][-1], (0, 4))) and np.all(np.isin(m["native_status"][-1], (0, 4))), (case, m["status"][-1], m["native_status"][-1])
    differ, total, worst, holds = kp.count_rule(pairs)
    print("full solves of the cases with K >= 3 on which the twin's two builds take another iteration count: %d of %d (largest difference %d)"
          % (differ, total, worst))
    assert holds, "the twin's own builds miss the iteration-count rule: no fixture written"
    np.savez_compressed(kp.FIXTURE, **out)
    print("wrote %s (%d bytes)" % (kp.FIXTURE, os.path.getsize(kp.FIXTURE)))


if __name__ == "__main__":
    main()
