"""Independent CPU reference for the aerodynamic body torque (SCVX_MODEL_AERO_TORQUE, include/scvx.h) -- a helper module, not a test file.

oracle/ is frozen and knows no torque, so the term is checked against this restatement instead: torch (CPU, float64) code of the
symbolic right-hand side (exo / aero / fins / torque, dynamics.jl:54-77 with the comment at :69 enabled, aerodynamics.jl:60-77), the cubic
B-spline of the tables evaluated from oracle.dynamics.prefilter_table coefficients with Flat() clamping, the first-order hold and the RK4
of the oracle with npts substeps.  Derivatives are torch.func.jacfwd of the WHOLE segment map inp[21 | 25] -> x+ (vmapped over segments):
automatic differentiation, independent of both the HIP analytic Jacobians and the C oracle's variational equations.

Params / linearize / propagate have the signatures of oracle.dynamics, so the oracle's SCvx loop (socp.build, ipm.solve, the trust-region
rules: oracle/scvx.py) runs on this discretisation unchanged:

    with unittest.mock.patch.object(oracle.scvx, "od", shim(torque=True)): ...
"""
import functools
import types

import numpy as np
import torch
from torch.func import jacfwd, vmap

from oracle.dynamics import prefilter_table

NX = 14
_T = dict(dtype=torch.float64, device="cpu")


class Params:
    """ProbInfo of an oracle.model.DescentProblem, plus the torque switch (valid only with aerodynamic data)."""

    def __init__(self, p, torque=False):
        if torque and p.aero is None:
            raise ValueError("the aerodynamic torque needs AtmosphericData")
        self.nu = 5 if getattr(p, "fins", False) else 3
        self.np = NX + 2 * self.nu + 1
        self.fins, self.torque = self.nu == 5, bool(torque)
        self.alpha, self.g0, self.sos = float(p.alpha), float(p.g), float(p.sos)
        J = np.asarray(p.jB, float)
        self.J = torch.tensor(J, **_T)
        self.Jinv = torch.tensor(np.linalg.inv(J), **_T)
        self.rTB = torch.tensor(np.asarray(p.rTB, float), **_T)
        self.rFB = torch.tensor(np.asarray(p.rFB, float), **_T)
        self.aero = p.aero is not None
        if self.aero:
            a = p.aero
            self.n_mach, self.n_aoa = a.drag.shape
            self.aoa0, self.daoa, self.mach0, self.dmach = float(a.aoa0), float(a.daoa), float(a.mach0), float(a.dmach)
            self.fs, self.ls = float(a.force_scalar), float(a.length_scalar)
            self.cdrag = torch.tensor(prefilter_table(a.drag), **_T)
            self.clift = torch.tensor(prefilter_table(a.lift), **_T)
            self.ctrq = torch.tensor(prefilter_table(a.trq), **_T)


def _weights(d):
    """uniform cubic B-spline basis at offset d in [0, 1]: weights of the coefficients i-1 .. i+2"""
    return torch.stack([(1 - d) ** 3 / 6, (4 - 6 * d**2 + 3 * d**3) / 6, (1 + 3 * d + 3 * d**2 - 3 * d**3) / 6, d**3 / 6])


def spline(par, coef, cos_aoa, mach):
    """Interpolations.jl extrapolate(scale(interpolate(A, BSpline(Cubic(Line(OnGrid())))), aoa, mach), Flat()) from the prefiltered
    coefficients [(n_mach+2)][(n_aoa+2)]: the arguments are clamped to the grid (zero slope outside)."""
    ta = torch.clamp((cos_aoa - par.aoa0) / par.daoa, 0.0, par.n_aoa - 1.0)
    tm = torch.clamp((mach - par.mach0) / par.dmach, 0.0, par.n_mach - 1.0)
    ia = torch.clamp(torch.floor(ta.detach()), 0, par.n_aoa - 2).long()
    im = torch.clamp(torch.floor(tm.detach()), 0, par.n_mach - 2).long()
    wa, wm = _weights(ta - ia), _weights(tm - im)
    off = torch.arange(4)
    block = coef[(im + off)[:, None], (ia + off)[None, :]]   # 4 x 4: mach rows, aoa columns
    return wm @ block @ wa


def dcm(q):
    q0, q1, q2, q3 = q[0], q[1], q[2], q[3]
    return torch.stack([
        torch.stack([1 - 2 * (q2 * q2 + q3 * q3), 2 * (q1 * q2 - q0 * q3), 2 * (q1 * q3 + q0 * q2)]),
        torch.stack([2 * (q1 * q2 + q0 * q3), 1 - 2 * (q1 * q1 + q3 * q3), 2 * (q2 * q3 - q0 * q1)]),
        torch.stack([2 * (q1 * q3 - q0 * q2), 2 * (q2 * q3 + q0 * q1), 1 - 2 * (q1 * q1 + q2 * q2)])])


def _safe_norm(a):
    """|a| with a zero (not NaN) derivative at a = 0"""
    n2 = (a * a).sum()
    ok = n2 > 0
    return torch.where(ok, torch.sqrt(torch.where(ok, n2, torch.ones_like(n2))), torch.zeros_like(n2)), ok


def aero_terms(par, q, v):
    """(force, torque) of the symbolic aero_force (aerodynamics.jl:60-77) at body attitude q and velocity v.  The torque is
    T(c, M) * length_scalar * force_scalar * (v x bv): ifnz(val, nz) = nz (dynamics.jl:205-207) leaves its direction un-normalised."""
    C = dcm(q)
    bv = C[:, 0]
    vn, on = _safe_norm(v)
    mach = vn / par.sos
    c = (bv * v).sum()
    # clamp_aoa (dynamics.jl:162-168): clamp(bv . v / (M sos), -1, 1), 0 when M <= 0
    cos_aoa = torch.where(on, torch.clamp(c / torch.where(on, mach * par.sos, torch.ones_like(mach)), -1.0, 1.0), torch.zeros_like(c))
    drag = spline(par, par.cdrag, cos_aoa, mach) * par.fs
    lift = spline(par, par.clift, cos_aoa, mach) * par.fs
    vhat = torch.where(on, v / torch.where(on, vn, torch.ones_like(vn)), torch.zeros_like(v))
    liftd = torch.linalg.cross(torch.linalg.cross(bv, v), v)
    ln, has_lift = _safe_norm(liftd)
    lhat = torch.where(has_lift, liftd / torch.where(has_lift, ln, torch.ones_like(ln)), torch.zeros_like(liftd))
    F = torch.where(on, drag * vhat + lift * lhat, torch.zeros_like(v))
    T = spline(par, par.ctrq, cos_aoa, mach) * (par.ls * par.fs)
    tau = T * torch.linalg.cross(v, bv)
    return F, tau


def rhs(par, x, u):
    """dx_static (dynamics.jl:54-77) with the build's extensions: fins (u[3:5], include/scvx.h) and the aerodynamic torque."""
    v, q, w = x[4:7], x[7:11], x[11:14]
    C = dcm(q)
    ut = u[:3]
    F = torch.zeros(3, **_T)
    torque = torch.linalg.cross(par.rTB, ut) - torch.linalg.cross(w, par.J @ w)
    if par.aero:
        Fa, tau = aero_terms(par, q, v)
        F = F + Fa
        if par.torque:
            torque = torque + tau
    if par.fins:
        n = torch.linalg.cross(C[:, 1], v)
        nn, ok = _safe_norm(n)
        fd1 = torch.where(ok, n / torch.where(ok, nn, torch.ones_like(nn)), torch.zeros_like(n))
        fd2 = torch.linalg.cross(fd1, v)
        ff = u[3] * fd1 + u[4] * fd2
        F = F + ff
        torque = torque + torch.linalg.cross(par.rFB, ff)
    mdot = -par.alpha * torch.sqrt((ut * ut).sum())
    vdot = (C @ ut + F) / x[0] - torch.tensor([par.g0, 0.0, 0.0], **_T)
    qdot = 0.5 * torch.stack([-w[0] * q[1] - w[1] * q[2] - w[2] * q[3],
                              w[0] * q[0] + w[2] * q[2] - w[1] * q[3],
                              w[1] * q[0] - w[2] * q[1] + w[0] * q[3],
                              w[2] * q[0] + w[1] * q[1] - w[0] * q[2]])
    wdot = par.Jinv @ torque
    return torch.cat([mdot[None], v, vdot, qdot, wdot])


def segment_map(par, inp, dt, nsub):
    """inp = [x; u_k; u_{k+1}; sigma] -> the state at the end of the segment: RK4 with nsub substeps, FOH control at substep start /
    middle / end (the oracle's integrator, without the reference rk4's stage bug)."""
    nu = par.nu
    x, uk, up, sig = inp[:NX], inp[NX:NX + nu], inp[NX + nu:NX + 2 * nu], inp[NX + 2 * nu]
    h = dt / nsub

    def f(xx, lam):
        return sig * rhs(par, xx, uk * (1.0 - lam) + up * lam)

    for s in range(nsub):
        l0, lm, l1 = s / nsub, (s + 0.5) / nsub, (s + 1.0) / nsub
        k1 = f(x, l0)
        k2 = f(x + 0.5 * h * k1, lm)
        k3 = f(x + 0.5 * h * k2, lm)
        k4 = f(x + h * k3, l1)
        x = x + h / 6.0 * k1 + h / 3.0 * k2 + h / 3.0 * k3 + h / 6.0 * k4
    return x


def _inputs(par, x, u, sigma):
    x, u, sigma = np.asarray(x, float), np.asarray(u, float), np.asarray(sigma, float)
    B, K1, _ = x.shape
    K = K1 - 1
    assert u.shape == (B, K1, par.nu), (u.shape, par.nu)
    inp = np.concatenate([x[:, :-1], u[:, :-1], u[:, 1:], np.broadcast_to(sigma[:, None, None], (B, K, 1))], axis=-1)
    return torch.tensor(inp.reshape(B * K, par.np), **_T), B, K


def linearize(par, x, u, sigma, dt, nsub=10):
    """x [B][K+1][14], u [B][K+1][nu], sigma [B] -> endpoint [B][K][14], deriv [B][K][np][14] (the layout of oracle.dynamics)."""
    inp, B, K = _inputs(par, x, u, sigma)
    fmap = functools.partial(segment_map, par, dt=float(dt), nsub=int(nsub))
    with torch.no_grad():
        e = vmap(fmap)(inp)
    d = vmap(jacfwd(fmap))(inp)        # [B K][14][np]
    return e.numpy().reshape(B, K, NX), d.detach().transpose(1, 2).numpy().reshape(B, K, par.np, NX)


def propagate(par, x, u, sigma, dt, nsub=10):
    inp, B, K = _inputs(par, x, u, sigma)
    with torch.no_grad():
        e = vmap(functools.partial(segment_map, par, dt=float(dt), nsub=int(nsub)))(inp)
    return e.numpy().reshape(B, K, NX)


def shim(torque=True):
    """A stand-in for the oracle.dynamics module as oracle/scvx.py uses it (od.Params / od.linearize / od.propagate)."""
    return types.SimpleNamespace(Params=functools.partial(Params, torque=torque), linearize=linearize, propagate=propagate)
