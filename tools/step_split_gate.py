"""Gate of profiles/step_split.md: what free-running halves of the bench batch gain with NO library change.  Two IntegratorCache
objects (each context owns its own HIP stream), each with a ScvxBatch over one half of the bench's dispersed initial conditions,
stepped alternately with solve_step_async / reset exactly as bench.py's timed_steps does (2 warm-up steps, back to create_initial,
one solve_problem period of 14 steps), against ONE batch of the whole size in the same process; the two forms are timed in turn,
`reps` times each.  The halves never join on the host inside the timed region, so a half that drains or runs its small kernels
leaves the device to the other half's conic solve.
    python tools/step_split_gate.py [B [parts [reps]]]      (defaults 8192 2 5)
Prints one line per repetition and a JSON summary line (ms per step of either form, the gain and the whole form's min-max range)."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from successiveconvexification_amd import sample_problems as sp
from successiveconvexification_amd.batch import ScvxBatch
from successiveconvexification_amd.dynamics import IntegratorCache
import bench

B = int(sys.argv[1]) if len(sys.argv) > 1 else 8192
M = int(sys.argv[2]) if len(sys.argv) > 2 else 2
REPS = int(sys.argv[3]) if len(sys.argv) > 3 else 5
WARMUP, STEPS = 2, 14
p = sp.base_prob_scaled
period = max(p.imax - 1, 1)
ic = bench.disperse_ics(p, 0, B, 20261004)


def timed_steps(batches, caches):
    """bench.py's timed_steps over a list of batches that together are one step"""
    def each(f):
        for b in batches:
            f(b)

    def barrier():
        for c in caches:
            c.synchronize()
    cnt = 0
    for _ in range(WARMUP):
        if cnt and cnt % period == 0:
            each(lambda b: b.reset())
        each(lambda b: b.solve_step_async())
        cnt += 1
    each(lambda b: b.reset())
    cnt = 0
    barrier()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        if cnt and cnt % period == 0:
            each(lambda b: b.reset())
        each(lambda b: b.solve_step_async())
        cnt += 1
    barrier()
    return 1e3 * (time.perf_counter() - t0) / STEPS


whole_c = [IntegratorCache(p)]
whole_b = [ScvxBatch(whole_c[0], B).init(ic)]
cut = [(B // M) * m + min(m, B % M) for m in range(M + 1)]     # contiguous parts, the first B mod M one longer
part_c = [IntegratorCache(p) for _ in range(M)]
part_b = [ScvxBatch(part_c[m], cut[m + 1] - cut[m]).init(ic[cut[m]:cut[m + 1]]) for m in range(M)]
whole, parts = [], []
for rep in range(REPS):
    whole.append(timed_steps(whole_b, whole_c))
    parts.append(timed_steps(part_b, part_c))
    print("rep %d  whole %.3f ms/step   %d parts %.3f ms/step" % (rep, whole[-1], M, parts[-1]), flush=True)
# the halves compute what the whole batch computes: same trajectories, bit for bit (the executor is the same at these sizes)
import numpy as np
rec = whole_b[0].trajectory_record()
same = bool(np.array_equal(rec, np.concatenate([b.trajectory_record() for b in part_b])))
mean = lambda v: sum(v) / len(v)   # noqa: E731
print(json.dumps({"B": B, "parts": M, "whole_ms_per_step": whole, "parts_ms_per_step": parts, "whole_mean": mean(whole),
                  "parts_mean": mean(parts), "gain_ms": mean(whole) - mean(parts), "whole_range": max(whole) - min(whole),
                  "bar_3x_range": 3 * (max(whole) - min(whole)), "no_overlap": max(parts) < min(whole), "records_equal": same}))
for b in whole_b + part_b:
    b.close()
for c in whole_c + part_c:
    c.close()
