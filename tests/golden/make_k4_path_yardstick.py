"""Writes tests/golden/k4_path_yardstick.npz: the yardstick of the interior-point path comparison (tests/k4_path_reference.py), from the
CPU twin alone -- its parity build against its native build and against itself on inputs perturbed by one ulp relative -- with the
twin's iteration counts, statuses and merit per depth.  No GPU, seconds.
    python tests/golden/make_k4_path_yardstick.py
With the argument `endgame` it writes tests/golden/k4_endgame_yardstick.npz for k4_path_reference.ENDGAME_CASES instead (it needs
tests/golden/oracle_endgame_runs.npz) and leaves k4_path_yardstick.npz alone: the native build differs by machine, so the two files are
regenerated independently.
    python tests/golden/make_k4_path_yardstick.py endgame"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import k4_path_reference as kp  # noqa: E402


def main(endgame=False):
    cases, depths, fixture = (kp.ENDGAME_CASES, kp.ENDGAME_DEPTHS, kp.ENDGAME_FIXTURE) if endgame else (kp.CASES, kp.DEPTHS, kp.FIXTURE)
    out = dict(depths=np.array(depths), groups=np.array(kp.GROUPS), cases=np.array(list(cases)))
    for case in cases:
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
        for i, n in enumerate(depths):
            print("    depth %2d  native %s  perturbed %s" % (n, " ".join("%.1e" % v for v in m["native"][i]), " ".join("%.1e" % v for v in m["perturb"][i])))
        print("    max over the truncated depths: %s ; full: %s" % (" ".join("%.1e" % v for v in Y[:-1].max(axis=0)), " ".join("%.1e" % v for v in Y[-1])))
    np.savez_compressed(fixture, **out)
    print("wrote %s (%d bytes)" % (fixture, os.path.getsize(fixture)))


if __name__ == "__main__":
    main(sys.argv[1:] == ["endgame"])
