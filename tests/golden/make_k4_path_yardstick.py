"""Writes tests/golden/k4_path_yardstick.npz: the yardstick of the interior-point path comparison (tests/k4_path_reference.py), from the
CPU twin alone -- its parity build against its native build and against itself on inputs perturbed by one ulp relative -- with the
twin's iteration counts, statuses and merit per depth.  No GPU, seconds.
    python tests/golden/make_k4_path_yardstick.py"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import k4_path_reference as kp  # noqa: E402


def main():
    out = dict(depths=np.array(kp.DEPTHS), groups=np.array(kp.GROUPS), cases=np.array(list(kp.CASES)))
    for case in kp.CASES:
        m = kp.measure(case)
        k = kp.key(case)
        for name in ("native", "perturb"):
            out[name + "_" + k] = m[name]
        out["iters_" + k] = m["iters"].astype(np.int16)
        out["status_" + k] = m["status"].astype(np.int8)
        out["merit_" + k] = m["merit"]
        same = np.array_equal(m["iters"], m["native_iters"]) and np.array_equal(m["status"], m["native_status"])
        out["counts_identical_" + k] = np.array(same)
        Y = np.maximum(m["native"], m["perturb"])
        print("%-24s counts identical between the builds: %s; statuses at full depth %s, iterations %s" % (case, same, m["status"][-1], m["iters"][-1]))
        for i, n in enumerate(kp.DEPTHS):
            print("    depth %2d  native %s  perturbed %s" % (n, " ".join("%.1e" % v for v in m["native"][i]), " ".join("%.1e" % v for v in m["perturb"][i])))
        print("    max over depths <= 12: %s ; full: %s" % (" ".join("%.1e" % v for v in Y[:-1].max(axis=0)), " ".join("%.1e" % v for v in Y[-1])))
    np.savez_compressed(kp.FIXTURE, **out)
    print("wrote %s (%d bytes)" % (kp.FIXTURE, os.path.getsize(kp.FIXTURE)))


if __name__ == "__main__":
    main()
