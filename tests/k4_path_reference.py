"""Case table and helpers of the interior-point PATH comparison of the conic kernel (K4) with its CPU twin: a solve truncated after n
iterations (scvx_solver_opts.max_iter = n / port.socp(max_iter=n), retries = 0) returns the best iterate so far, so the device and
the twin can be compared at every depth of the path and not only at its self-correcting end.

Used by tests/golden/make_k4_path_yardstick.py (writes tests/golden/k4_path_yardstick.npz from the twin alone),
tests/test_k4_path_cpu.py (the method, no GPU) and tests/test_gpu_k4_path.py (the device).

Yardstick Y(case, depth, group): the larger of
  * the distance between the twin's parity build (-O2 -ffp-contract=off) and its native build (-O3 -march=native, contraction on),
  * the distance between the parity twin and itself with every entry of deriv and endpoint multiplied by 1 + 2^-52 U(-1, 1)
    (three seeded draws),
per group, maximised over the trajectories: dx, du, dsigma, nu by largest absolute difference, merit and pobj relative.

ENDGAME_CASES is a second, separate table: the same comparison at iterates of runs that converge (tests/endgame_reference.py, fixture
tests/golden/oracle_endgame_runs.npz), with the trust radius of the recorded step instead of create_initial's 100; its yardstick is
tests/golden/k4_endgame_yardstick.npz (tests/golden/make_k4_path_yardstick.py endgame).  CASES and k4_path_yardstick.npz do not depend on it."""
import functools
import os
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "k4_path_yardstick.npz")

FULL = 60                                   # max_iter of the untruncated solve
DEPTHS = (1, 2, 3, 4, 6, 8, 10, 12, FULL)
GROUPS = ("dx", "du", "ds", "nu", "merit", "pobj")
SEED = 20261004
EPS = 2.0 ** -52
PERTURB_SEEDS = (1, 2, 3)
FACTOR = 10.0                               # the project's convention (tests/test_k4_fused_sweeps_twin.py)

# name -> model ("exo" / "fin" / "fuzz3" / "aero" / "flyable"), K (None: the model's own), B, nsub of the linearisation (None: the
# back-off fixture's), float tiles, back-offs.  The smallest shapes at which each code path can still go wrong: the odd and tiny
# horizons move the middle node of the two-ended chain, the fin cases have 24-column operands, the fuzz class adds the dynamic-pressure
# cone group and two starts that are infeasible at node 1 (status 5: compared by status only).
CASES = {
    "exo K=50": dict(model="exo", K=50, B=8, nsub=4),
    "exo K=4": dict(model="exo", K=4, B=8, nsub=4),
    "exo K=8": dict(model="exo", K=8, B=8, nsub=4),
    "exo K=9": dict(model="exo", K=9, B=8, nsub=4),
    "exo K=31": dict(model="exo", K=31, B=8, nsub=4),
    "fins K=50": dict(model="fin", K=50, B=8, nsub=4),
    "fins K=9": dict(model="fin", K=9, B=8, nsub=4),
    "fuzz class 3 (dp cone)": dict(model="fuzz3", K=None, B=8, nsub=4),
    "float tiles": dict(model="exo", K=50, B=8, nsub=4, lin32=True),
    "aero K=50": dict(model="aero", K=50, B=8, nsub=4),
    "thrust back-offs": dict(model="flyable", K=None, B=1, nsub=None, margins=True),
}
# case -> truncated depths dropped: a depth is kept only where the twin's merit is below the merit of every earlier depth by more than
# a relative 1e-6 (the solver returns the BEST iterate: a near-tie could be decided differently by the device).
# tests/test_k4_path_cpu.py checks this table, on the CPU; nothing is dropped on the GPU.  Depth 2: on these cases the second iteration of some trajectories does not
# improve on the first (merit 1579.463 after both on trajectory 3 of exo K = 50; on the fin cases of none), so the solve truncated
# there hands back iterate 1 again
DROPPED_DEPTHS = {c: (2,) for c in ("exo K=50", "exo K=8", "exo K=9", "fins K=50", "fins K=9", "float tiles", "aero K=50")}


# ---- the converging regime: B = 2 as pairs (step of run exo2, step of run exo3), steps 1-based, -1 = the run's last; the aero case B = 1.
# Both sides solve at 1e-9 (the tolerance of the fixture's subproblem record: up to 26 iterations), hence the two further depths.
ENDGAME_FIXTURE = os.path.join(GOLDEN, "k4_endgame_yardstick.npz")
ENDGAME_DEPTHS = (1, 2, 3, 4, 6, 8, 10, 12, 16, 20, FULL)
ENDGAME_TOL = 1e-9
ENDGAME_CASES = {
    "trust region binds": dict(runs=("exo2", "exo3"), steps=(9, 2)),
    "nu at the vertex": dict(runs=("exo2", "exo3"), steps=(11, 4)),
    "last step": dict(runs=("exo2", "exo3"), steps=(13, -1)),
    "nu at the vertex, float tiles": dict(runs=("exo2", "exo3"), steps=(11, 4), lin32=True),
    "aero, last step": dict(runs=("aero2",), steps=(13,)),
}
# the rule of DROPPED_DEPTHS, and one more: a truncated depth at which some trajectory of the twin has already finished (status 0) is
# dropped too -- a finished solve is compared at full depth, where an iteration count one off has its own rule.  Decided on the CPU
# (tests/test_endgame_cpu.py), never on the GPU.
# Depth 20: the trajectories of these cases finish after 17 to 19 iterations.  Depths 4 and 6 of "last step": iterations 4 to 6 of the
# exo3 trajectory do not improve on the third (merit 8.8188 after each).
ENDGAME_DROPPED_DEPTHS = {"trust region binds": (20,), "nu at the vertex": (20,), "nu at the vertex, float tiles": (20,), "last step": (4, 6)}


def spec_of(case):
    return CASES[case] if case in CASES else ENDGAME_CASES[case]


def all_depths(case):
    return DEPTHS if case in CASES else ENDGAME_DEPTHS


def tol_of(case):
    return 1e-8 if case in CASES else ENDGAME_TOL


def depths_of(case):
    drop = DROPPED_DEPTHS.get(case, ()) if case in CASES else ENDGAME_DROPPED_DEPTHS.get(case, ())
    return tuple(n for n in all_depths(case) if n not in drop)


@functools.lru_cache(maxsize=None)
def endgame_states(case):
    """(ic [B][6], x, u, sigma, rk [B]) of an endgame case: the recorded pre-step states (read once per case; do not write to them)"""
    import endgame_reference as er
    g = er.load()
    c = ENDGAME_CASES[case]
    st = [er.state(g, r, (er.steps_of(g, r) if s < 0 else s) - 1) for r, s in zip(c["runs"], c["steps"])]
    return (np.stack([g[r + "_ic"] for r in c["runs"]]), np.stack([s[0] for s in st]), np.stack([s[1] for s in st]), np.array([s[2] for s in st]),
            np.array([s[3] for s in st]))


def rk_of(case):
    """the trust radius the case's subproblem is solved under: create_initial's 100, or the recorded steps' [B]"""
    return 100.0 if case in CASES else endgame_states(case)[4]


def key(case):
    return case.replace(" ", "_").replace("=", "").replace("(", "").replace(")", "")


def _aero_tables():
    z = np.load(os.path.join(GOLDEN, "lift_drag_tables.npz"))
    return z["drag"], z["lift"], z["torque"]


def _fuzz_class(cls):
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import k4_fuzz
    from oracle import model
    rng = np.random.default_rng(1)
    base = model.base_prob_scaled()
    for _ in range(cls + 1):
        po = k4_fuzz.draw_class(rng, base)
    return po


def oracle_problem(case):
    """(oracle DescentProblem, ic [B][6], back-offs [B][K+1][2] or None, nsub) of a case"""
    from oracle import model
    if case in ENDGAME_CASES:
        import endgame_reference as er
        return er.oracle_problem(ENDGAME_CASES[case]["runs"][0]), endgame_states(case)[0], None, er.NSUB
    c = CASES[case]
    marg = None
    nsub = c["nsub"]
    if c["model"] == "exo":
        po = model.base_prob_scaled()
    elif c["model"] == "fin":
        po = model.base_prob_fin_scaled()
    elif c["model"] == "aero":
        po = model.base_prob_scaled(model.AeroData(*_aero_tables()))
    elif c["model"] == "fuzz3":
        po = _fuzz_class(3)
        assert po.K == 50 and po.enforce_dp
    else:
        po = replace(model.base_prob_scaled(), mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    if c["K"] is not None:
        po = replace(po, K=c["K"])
    if c.get("margins"):
        g = np.load(os.path.join(GOLDEN, "oracle_margin_runs.npz"))
        ic = g["ic"][:c["B"]]
        marg = np.ascontiguousarray(np.stack([g["lo"][:c["B"]], g["hi"][:c["B"]]], axis=-1))
        nsub = int(g["nsub"])
    else:
        ic = model.disperse_ics(po, c["B"], SEED)
    return po, ic, marg, nsub


def device_problem(case):
    """the product's DescentProblem of a case (successiveconvexification_amd.sample_problems), matching oracle_problem(case)"""
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    if case in ENDGAME_CASES:
        import endgame_reference as er
        return er.device_problem(ENDGAME_CASES[case]["runs"][0])
    c = CASES[case]
    if c["model"] == "exo":
        pp = sp.base_prob_scaled
    elif c["model"] == "fin":
        pp = sp.base_prob_fin_scaled()
    elif c["model"] == "aero":
        pp = sp.base_prob_aero_scaled(AtmosphericData(*_aero_tables()))
    elif c["model"] == "fuzz3":
        po = _fuzz_class(3)
        pp = replace(sp.base_prob_scaled, K=po.K, mdry=po.mdry, Tmin=po.Tmin, deltaMax=po.deltaMax, thetaMax=po.thetaMax,
                     gammaGs=po.gammaGs, omMax=po.omMax, tf_guess=po.tf_guess,
                     model_flags=sp.base_prob_scaled.model_flags | (1 if po.enforce_dp else 0))
    else:
        pp = replace(sp.base_prob_scaled, mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)
    if c["K"] is not None:
        pp = replace(pp, K=c["K"])
    return pp


def cpu_inputs(case):
    """create_initial's straight-line iterate (an endgame case: the recorded iterates) and the ORACLE's linearisation of it:
    (po, ic, marg, xbar, ubar, sigma, endpoint, deriv)"""
    from oracle import dynamics as od, model
    po, ic, marg, nsub = oracle_problem(case)
    B, K = ic.shape[0], po.K
    if case in ENDGAME_CASES:
        _, x, u, sg, _ = endgame_states(case)
        e, d = od.linearize(od.Params(po), x, u, sg, 1.0 / (K + 1), nsub)
        return po, ic, marg, x, u, sg, e, d
    x = np.zeros((B, K + 1, 14))
    u = np.zeros((B, K + 1, po.nu))
    for t in range(B):
        x[t], u[t] = model.linear_points(po, ic[t, :3], ic[t, 3:])
    sg = np.full(B, po.tf_guess)
    e, d = od.linearize(od.Params(po), x, u, sg, 1.0 / (K + 1), nsub)
    return po, ic, marg, x, u, sg, e, d


def run_twin(case, po, ic, marg, xb, ub, e, d, depth, **kw):
    """the twin (whichever build oracle.use_native selected) stopped after `depth` iterations, one attempt"""
    from oracle import port
    return port.socp(po, xb, ub, e, d, rk_of(case), ic, tol=tol_of(case), max_iter=int(depth), retries=0, lin32=bool(spec_of(case).get("lin32")), marg=marg,
                     **kw)


def _rel(a, b):
    a, b = np.asarray(a, float), np.asarray(b, float)
    den = np.maximum(np.maximum(np.abs(a), np.abs(b)), 1e-300)
    return np.abs(a - b) / den


def distance(a, b, keep=None):
    """per group of GROUPS, maximised over the trajectories of `keep` (bool [B]; None: all): dx, du, ds, nu absolute, merit and pobj
    relative.  a, b: dicts as port.socp returns them."""
    B = a["dx"].shape[0]
    keep = np.ones(B, bool) if keep is None else np.asarray(keep, bool)
    if not keep.any():
        return np.zeros(len(GROUPS))
    out = []
    for g in GROUPS:
        x, y = np.asarray(a[g])[keep], np.asarray(b[g])[keep]
        out.append(float(_rel(x, y).max()) if g in ("merit", "pobj") else float(np.abs(x - y).max()))
    return np.array(out)


def magnitudes(a, keep=None):
    """largest |entry| per group (what the reordering floor scales with)"""
    B = a["dx"].shape[0]
    keep = np.ones(B, bool) if keep is None else np.asarray(keep, bool)
    if not keep.any():
        return np.zeros(len(GROUPS))
    return np.array([1.0 if g in ("merit", "pobj") else float(np.abs(np.asarray(a[g])[keep]).max()) for g in GROUPS])


def floor(K, NU, mag):
    """2^-52 (K+1) (14+2NU+1) max|entry of the group|: the first-order bound on re-ordering the longest sums the start point goes
    through (the depth-1 yardstick is 1e-16, and the device contracts and sums in MFMA order)"""
    return EPS * (K + 1) * (14 + 2 * NU + 1) * np.asarray(mag, float)


def perturbed(e, d, seed):
    rng = np.random.default_rng(seed)
    return e * (1.0 + EPS * rng.uniform(-1.0, 1.0, e.shape)), d * (1.0 + EPS * rng.uniform(-1.0, 1.0, d.shape))


def measure(case, depths=None):
    """The yardstick of a case on this machine, from the twin alone.  Returns dict(native, perturb [depth][group], iters, status
    [depth][B], merit [depth][B], native_iters, native_status)."""
    import oracle
    oracle.use_native(False)
    depths = all_depths(case) if depths is None else depths
    po, ic, marg, xb, ub, sg, e, d = cpu_inputs(case)
    par, per = {}, {}
    for n in depths:
        par[n] = run_twin(case, po, ic, marg, xb, ub, e, d, n)
        per[n] = [run_twin(case, po, ic, marg, xb, ub, *perturbed(e, d, s), n) for s in PERTURB_SEEDS]
    oracle.use_native(True)
    try:
        nat = {n: run_twin(case, po, ic, marg, xb, ub, e, d, n) for n in depths}
    finally:
        oracle.use_native(False)
    keep = par[depths[-1]]["status"] != 5
    return dict(native=np.array([distance(par[n], nat[n], keep) for n in depths]),
                perturb=np.array([np.max([distance(par[n], q, keep) for q in per[n]], axis=0) for n in depths]),
                iters=np.array([par[n]["iters"] for n in depths]), status=np.array([par[n]["status"] for n in depths]),
                merit=np.array([par[n]["merit"] for n in depths]),
                native_iters=np.array([nat[n]["iters"] for n in depths]), native_status=np.array([nat[n]["status"] for n in depths]))


def yardstick(case, fixture=None):
    """Y [depth of all_depths(case)][group] of a case from the committed fixture"""
    g = np.load(FIXTURE if case in CASES else ENDGAME_FIXTURE) if fixture is None else fixture
    k = key(case)
    return np.maximum(g["native_" + k], g["perturb_" + k])
