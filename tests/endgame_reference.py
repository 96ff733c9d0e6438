"""The conic solve (K4) and the SCvx step (K1, K2, K3, K5) in the CONVERGING regime -- a helper module, not a test file.

Every other subproblem the suite compares with something outside the device is the FIRST one (the straight-line guess, rk = 100,
cost = Inf).  Here the independent oracle (oracle.scvx: oracle.socp.build + oracle.ipm) is re-run step by step on runs that converge,
and every subproblem and every step of them is recorded (tests/golden/oracle_endgame_runs.npz, written by
tests/golden/make_oracle_endgame_runs.py): the nu-cone collapsed onto its vertex, a dozen nodes riding Tmin, a trust region that binds,
steps of 1e-7.

Runs (RUNS): the flyable variant of tests/golden/make_oracle_flight_runs.py on its two dispersed starts ("exo2", "exo3": trajectories
2 and 3 of model.disperse_ics(p, 4, 7), the plans of oracle_flight_runs.npz) and its aero variant on trajectory 2 ("aero2"); tol 1e-8,
nsub 10.

Per run r and step s (1-based in the text, 0-based in the arrays) the fixture holds
  * the pre-step state: r_iterate_x / _u / _sigma [distinct iterates] with r_iterate_of [step] (a rejected step keeps its iterate),
    r_rk, r_cost, r_iter;
  * the oracle's subproblem solution re-solved at SUB_TOL = 1e-9 (r_xr, r_ur, r_dsr, r_nur [K][14], r_pobj, r_Jtr, and its certificates
    r_gap, r_pres, r_dres), or, where that solve is not "optimal", the run's own 1e-8 solution, with the tolerance in r_sub_tol;
  * of that solution: r_jK, r_lK, r_rho, r_dJ, r_nu_norm, r_tmin_nodes; of the run itself (1e-8): r_accepted, r_next_rk, r_run_rho,
    r_run_nu_norm, r_run_dJ, r_ipm_iters;
  * measured on the CPU alone, per group of GROUPS (x, u, dsigma, nu absolute; objective relative):
      r_TO  the parity twin (port.socp) on the oracle's linearisation against the oracle, both at sub_tol,
      r_R   the twin's response to the device's K1 not being the oracle's: the twin on tiles and endpoints multiplied by
            1 + 1e-11 U(-1, 1) (three seeded draws) against itself -- 1e-11 is the K1 parity bound of tests/test_gpu_discretize.py,
    and per group of STEP_GROUPS (cost, dJ, rho, |nu|; absolute) of a whole twin step (twin_step) from the recorded state:
      r_step_TO, r_step_R, with the twin's own figures in r_twin_step [step][4] and its iterations / status in r_twin_iters, r_twin_status.
      The twin step is NOT port.scvx_steps, which can start from create_initial only: it is the twin's conic solve (port.socp) at the
      recorded state pushed through the ORACLE's propagation and the formulas of rocketland.jl:289-297 (step_figures).  So step_TO and
      step_R hold no K2 / K3 difference of their own, only what the conic solve's difference does to cost, dJ and rho: the step bounds
      are tighter for it, not wider;
  * exo2_sub32_* at SUB32_STEPS: the oracle's solve on tiles rounded to float, with TO / R of the twin's float-tile build.

Nothing here reads the device."""
import functools
import os
from dataclasses import replace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FIXTURE = os.path.join(GOLDEN, "oracle_endgame_runs.npz")

NSUB = 10
RUN_TOL = 1e-8                               # the tolerance of oracle_flight_runs.npz
SUB_TOL = 1e-9
RUNS = {"exo2": dict(model="exo", traj=2, flight=0), "exo3": dict(model="exo", traj=3, flight=1), "aero2": dict(model="aero", traj=2, flight=None)}
GROUPS = ("x", "u", "ds", "nu", "obj")
STEP_GROUPS = ("cost", "dJ", "rho", "nu_norm")
K1_BOUND = 1e-11                             # tests/test_gpu_discretize.py
PERTURB_SEEDS = (1, 2, 3)
SUB32_STEPS = (11, 13)                       # of exo2, 1-based
FACTOR = 10.0
CAP = 2e-5                                   # the bound the suite uses on a minimiser against the independent oracle
OBJ_CAP = 1e-8
RHO_CLEARANCE = 0.05
# (run, step) -> why the oracle's rho is closer than RHO_CLEARANCE to a threshold.  At the last step of exo3 the oracle's interior-point
# method stalls (73 iterations) at a duality gap of 1.1e-7 whatever the tolerance, and ends "optimal" from 1.1e-9 up only by its
# numerical-floor rule (relgap < 100 tol): its point is 5.5e-8 above the twin's objective, and its rho = dJ / dL with dJ = 3.6e-4
# comes out as 0.9199 where the twin's is 1 - 1e-7 at 1e-8 and at 1e-9.  Both are on the same side of rh2 = 0.9; the generator
# asserts that, and that the twin's rho keeps the clearance.
NEAR_TIES = {("exo3", 6): "the oracle's solve ends on its numerical floor: rho 0.9199, the twin's 1.0000"}
STEP_KEYS = ("rk", "cost", "iter", "xr", "ur", "dsr", "nur", "pobj", "Jtr", "gap", "pres", "dres", "sub_tol", "jK", "lK", "rho", "dJ", "nu_norm", "tmin_nodes", "accepted",
             "next_rk", "run_rho", "run_nu_norm", "run_dJ", "ipm_iters", "rho_clearance", "TO", "R", "step_TO", "step_R", "twin_step", "twin_iters", "twin_status",
             "iterate_of")


def _aero_tables():
    z = np.load(os.path.join(GOLDEN, "lift_drag_tables.npz"))
    return z["drag"], z["lift"], z["torque"]


_EDITS = dict(mdry=0.55, nuTol=1e-6, delTol=1e-3, imax=40, tf_guess=8.0)


def oracle_problem(run):
    from oracle import model
    if RUNS[run]["model"] == "aero":
        return replace(model.base_prob_scaled(model.AeroData(*_aero_tables())), **_EDITS)
    return replace(model.base_prob_scaled(), **_EDITS)


def device_problem(run):
    from successiveconvexification_amd import sample_problems as sp
    from successiveconvexification_amd.defns import AtmosphericData
    if RUNS[run]["model"] == "aero":
        return replace(sp.base_prob_aero_scaled(AtmosphericData(*_aero_tables())), **_EDITS)
    return replace(sp.base_prob_scaled, **_EDITS)


def start(run):
    """ic [6] of a run"""
    from oracle import model
    return model.disperse_ics(oracle_problem(run), 4, 7)[RUNS[run]["traj"]]


def iterate(po, ic, x, u, sigma, rk, cost, it, deriv32=False):
    """oracle.scvx.Iterate of a recorded state, re-linearised by the oracle"""
    from oracle import dynamics as od, scvx
    par = od.Params(po)
    e, d = od.linearize(par, x[None], u[None], np.array([float(sigma)]), 1.0 / (po.K + 1), NSUB)
    p = replace(po, rIi=np.asarray(ic[:3], float), vIi=np.asarray(ic[3:], float))
    d = d.astype(np.float32).astype(np.float64) if deriv32 else d
    return scvx.Iterate(p, par, float(sigma), np.array(x, float), np.array(u, float), e[0], d[0], int(it), float(rk), float(cost), NSUB)


def objective(po, x, dx, du, ds, nu):
    """the subproblem's objective (rocketland.jl:84-86) of one trajectory's point"""
    return float(-x[po.K, 0] + po.wNu * np.linalg.norm(nu) + 0.5 * np.linalg.norm(np.concatenate([np.ravel(dx), np.ravel(du)])) + abs(ds))


def oracle_sub(it, tol):
    """the oracle's solve of the subproblem at `it`: (status, dict(xr, ur, dsr, nur [K][14], pobj, Jtr))"""
    from oracle import scvx
    sol, ix = scvx.solve_socp(it, tol)
    z = sol.x
    return sol.status, dict(xr=z[ix.xv].T.copy(), ur=z[ix.uv].T.copy(), dsr=float(z[ix.dsig]), nur=z[ix.nuv].T[1:].copy(), pobj=float(sol.pobj),
                            Jtr=float(z[ix.Jtr]), gap=float(sol.gap), pres=float(sol.pres), dres=float(sol.dres))


def step_figures(po, it, s):
    """jK, lK, rho, dJ, |nu| of a subproblem solution s at the iterate `it` (rocketland.jl:289-297); dJ = Inf where the step is rejected"""
    from oracle import dynamics as od
    K = po.K
    xn = od.propagate(it.par, s["xr"][None], s["ur"][None], np.array([it.sigma + s["dsr"]]), 1.0 / (K + 1), NSUB)[0]
    jK = float(-s["xr"][K, 0] + po.wNu * np.linalg.norm(s["xr"][1:] - xn))
    lK = float(-s["xr"][K, 0] + po.wNu * np.linalg.norm(s["nur"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        rho = float((it.cost - jK) / (it.cost - lK)) if np.isfinite(it.cost) else np.nan
    dJ = np.inf if rho < po.rh0 else float(it.cost - jK)
    return dict(jK=jK, lK=lK, rho=rho, dJ=dJ, nu_norm=float(np.linalg.norm(s["nur"])))


def twin_sub(po, ic, it, tol, lin32=False, e=None, d=None, **kw):
    """the parity twin on the linearisation of `it` (or on e, d [14..] of one trajectory): port.socp's dict, B = 1"""
    from oracle import port
    e = it.endpoint if e is None else e
    d = it.deriv if d is None else d
    return port.socp(po, it.x[None], it.u[None], e[None], d[None], np.array([it.rk]), np.asarray(ic, float)[None], tol=tol, lin32=lin32, **kw)


def twin_point(it, tw, t=0):
    """dict(xr, ur, dsr, nur) of trajectory t of a twin result"""
    return dict(xr=it.x + tw["dx"][t], ur=it.u + tw["du"][t], dsr=float(tw["ds"][t]), nur=tw["nu"][t].copy())


def distance(po, xbar, ubar, a, b):
    """per group of GROUPS between two points dict(xr, ur, dsr, nur[, pobj]): x, u, dsigma, nu absolute, objective relative (the
    objective of a point is its own pobj where it carries one -- the oracle's c'z -- and else computed from the point, as the device
    tests compute the device's)"""
    oa, ob = (s["pobj"] if "pobj" in s else objective(po, s["xr"], s["xr"] - xbar, s["ur"] - ubar, s["dsr"], s["nur"]) for s in (a, b))
    return np.array([np.abs(a["xr"] - b["xr"]).max(), np.abs(a["ur"] - b["ur"]).max(), abs(a["dsr"] - b["dsr"]), np.abs(a["nur"] - b["nur"]).max(),
                     abs(oa - ob) / max(abs(oa), abs(ob))])


def step_distance(a, b):
    """per group of STEP_GROUPS between two step_figures dicts, absolute; dJ: 0 where both are Inf (a rejected step), Inf where one is"""
    out = []
    for k in ("jK", "dJ", "rho", "nu_norm"):
        x, y = a[k], b[k]
        out.append(0.0 if (x == y or (np.isnan(x) and np.isnan(y))) else abs(x - y))
    return np.array(out)


def perturbed(e, d, seed):
    rng = np.random.default_rng(seed)
    return e * (1.0 + K1_BOUND * rng.uniform(-1.0, 1.0, e.shape)), d * (1.0 + K1_BOUND * rng.uniform(-1.0, 1.0, d.shape))


def measure_step(po, ic, it, ref, tol, lin32=False):
    """TO, R [5], step_TO, step_R [4], the twin's step figures [4], its iterations and status, at one recorded state: `it` the
    oracle's iterate, `ref` the oracle's subproblem solution at `tol`"""
    import oracle
    oracle.use_native(False)
    tw = twin_sub(po, ic, it, tol, lin32)
    pt = twin_point(it, tw)
    fo, ft = step_figures(po, it, ref), step_figures(po, it, pt)
    R, sR = np.zeros(len(GROUPS)), np.zeros(len(STEP_GROUPS))
    for s in PERTURB_SEEDS:
        e, d = perturbed(it.endpoint, it.deriv, s)
        q = twin_point(it, twin_sub(po, ic, it, tol, lin32, e=e, d=d))
        R, sR = np.maximum(R, distance(po, it.x, it.u, pt, q)), np.maximum(sR, step_distance(ft, step_figures(po, it, q)))
    return dict(TO=distance(po, it.x, it.u, pt, ref), R=R, step_TO=step_distance(ft, fo), step_R=sR,
                twin_step=np.array([ft["jK"], ft["dJ"], ft["rho"], ft["nu_norm"]]), twin_iters=int(tw["iters"][0]), twin_status=int(tw["status"][0]))


def tmin_nodes(po, ur):
    """nodes of a solution riding Tmin (within 1e-6)"""
    return int((np.linalg.norm(ur[:, :3], axis=1) < po.Tmin + 1e-6).sum())


# ---- reading the fixture -------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def load():
    """the fixture, unpacked once: a dict of its arrays"""
    with np.load(FIXTURE) as z:
        return {k: z[k] for k in z.files}


def steps_of(g, run):
    return int(g[run + "_rk"].shape[0])


def state(g, run, s):
    """the pre-step state of step s (0-based): (x, u, sigma, rk, cost, iter)"""
    i = int(g[run + "_iterate_of"][s])
    return (g[run + "_iterate_x"][i], g[run + "_iterate_u"][i], float(g[run + "_iterate_sigma"][i]), float(g[run + "_rk"][s]), float(g[run + "_cost"][s]),
            int(g[run + "_iter"][s]))


def reference(g, run, s, pre=""):
    """the oracle's subproblem solution of step s (0-based); pre = "sub32_" for the float-tile record (s indexes SUB32_STEPS then)"""
    return {k: (float(g["%s_%s%s" % (run, pre, k)][s]) if k in ("dsr", "pobj") else g["%s_%s%s" % (run, pre, k)][s]) for k in ("xr", "ur", "dsr", "nur", "pobj")}


def sub_bound(g, run, s, pre=""):
    """the device-vs-oracle bound per group of GROUPS: min(10 max(TO, R), cap), cap = 2e-5 on the minimiser and 1e-8 on the objective
    -- or the oracle's own duality gap relative to its objective where that is larger (its certificate of how well it knows its
    objective: above 1e-8 at the last step of exo3 only, 1.2e-7)"""
    b = FACTOR * np.maximum(g["%s_%sTO" % (run, pre)][s], g["%s_%sR" % (run, pre)][s])
    return np.minimum(b, np.array([CAP] * 4 + [obj_cap(g, run, s, pre)]))


def obj_cap(g, run, s, pre=""):
    """1e-8, but where the oracle's relative gap (gap / max(1, |pobj|), its own stopping measure) is above that: there gap / |pobj|"""
    gap, pobj = float(g["%s_%sgap" % (run, pre)][s]), abs(float(g["%s_%spobj" % (run, pre)][s]))
    return OBJ_CAP if gap / max(1.0, pobj) <= OBJ_CAP else gap / pobj


def step_bound(g, run, s):
    """the device-vs-oracle bound per group of STEP_GROUPS: 10 max(step_TO, step_R)"""
    return FACTOR * np.maximum(g[run + "_step_TO"][s], g[run + "_step_R"][s])


def subproblem_list(g, run):
    """the steps (0-based) whose subproblem the device test solves: every recorded step, except that a stretch of four or more rejected
    steps (one iterate, one subproblem but for the radius, which does not bind) counts as three: its first, its last and the one two
    before the last (rk 320, 20 and 5 on exo2)"""
    acc = g[run + "_accepted"]
    out, s, n = [], 0, len(acc)
    while s < n:
        if acc[s]:
            out.append(s)
            s += 1
            continue
        e = s
        while e + 1 < n and not acc[e + 1]:
            e += 1
        out += [s, e - 2, e] if e - s >= 3 else list(range(s, e + 1))
        s = e + 1
    return out
