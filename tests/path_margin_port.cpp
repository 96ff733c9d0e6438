// path_margin_port.cpp -- the CPU twin of the conic solve under path-constraint back-offs (TEST INFRASTRUCTURE, built by
// tests/test_path_margins_cpu.py with the flags of oracle/Makefile; the product never loads it).
//
// oracle/scvx_port.cpp compiles the interior-point core of the HIP kernel (successiveconvexification_amd/csrc/scvx_ipm_core.hpp)
// with a one-lane host executor, and must stay as it is; this file includes it for that executor and adds one entry point with a
// loop of its own that also calls Solver::set_path_margins.  With -DPATH_MARGIN_PORT_MAIN it is a stand-alone program (the form
// in which a sanitizer may check it): a solve of a synthetic hover subproblem with and without back-offs.
#include "../oracle/scvx_port.cpp"

namespace {
// B subproblems, one after the other.  Layouts as port_socp of scvx_port.cpp; marg [B][K+1][2] = (lo, hi) or null; pmarg
// [B][K+1][4] = (mass, glide, tilt, rate) or null -- what socp_body hands to the solver on the device.
template <class DStor, int NU>
int pm_socp(const scvx::ipm::Consts* C, int B, const double* xbar, const double* ubar, const double* endpoint, const double* deriv,
            const double* rk, const double* ic, double* sol, double* nu, double* info, const double* marg, const double* pmarg) {
    const int K = C->K;
    scvx::ipm::Layout L;
    L.init(K, C->vmax > 0.0, NU);
    constexpr int DSZ = 14 * (14 + 2 * NU + 1);
    std::vector<double> work(L.work_doubles());
    std::vector<DStor> D((size_t)K * DSZ);
    HostEx ex;
    for (int b = 0; b < B; b++) {
        for (size_t i = 0; i < D.size(); i++) D[i] = (DStor)deriv[(size_t)b * K * DSZ + i];
        scvx::ipm::Solver<HostEx, double, DStor, NU, SCVX_FACTOR_T> S(ex, *C);
        S.set_margins(marg ? marg + (size_t)b * (K + 1) * 2 : nullptr);
        S.set_path_margins(pmarg ? pmarg + (size_t)b * (K + 1) * 4 : nullptr);
        const scvx::ipm::Result r = S.solve(xbar + (size_t)b * (K + 1) * 14, ubar + (size_t)b * (K + 1) * NU, endpoint + (size_t)b * K * 14,
                                            D.data(), rk[b], ic + (size_t)b * 6, work.data(), false);
        double* so = sol + (size_t)b * ((K + 1) * (14 + NU) + 1);
        for (int i = 0; i < L.nx + L.nu_; i++) so[i] = S.V[i];
        so[L.nx + L.nu_] = S.V[L.iS];
        for (int i = 0; i < L.ny; i++) nu[(size_t)b * K * 14 + i] = S.V[L.nx + L.nu_ + i];
        info[4 * b + 0] = r.status; info[4 * b + 1] = r.iters; info[4 * b + 2] = r.merit; info[4 * b + 3] = r.pobj;
    }
    return 0;
}
}  // namespace

extern "C" {
// control_dim 3 (tiles: 0 double, 1 rounded to float) or 5 (double tiles); -1 for anything else
int path_margin_port_socp(const scvx::ipm::Consts* C, int B, const double* xbar, const double* ubar, const double* endpoint,
                          const double* deriv, const double* rk, const double* ic, double* sol, double* nu, double* info,
                          const double* marg, const double* pmarg, int control_dim, int lin32) {
    if (control_dim == 5 && !lin32) return pm_socp<double, 5>(C, B, xbar, ubar, endpoint, deriv, rk, ic, sol, nu, info, marg, pmarg);
    if (control_dim != 3) return -1;
    return lin32 ? pm_socp<float, 3>(C, B, xbar, ubar, endpoint, deriv, rk, ic, sol, nu, info, marg, pmarg)
                 : pm_socp<double, 3>(C, B, xbar, ubar, endpoint, deriv, rk, ic, sol, nu, info, marg, pmarg);
}
size_t path_margin_port_work_doubles(int K, int nu) {
    scvx::ipm::Layout L;
    L.init(K, false, nu);
    return L.work_doubles();
}
}

#if defined(PATH_MARGIN_PORT_MAIN)
// A synthetic subproblem: K = 6, the vehicle at rest above the pad with hover thrust, identity tiles (x_{k+1} = x_k).  The numbers
// mean nothing; the point is that every array the solver carves, the four path arrays among them, is written and read inside its slab.
int main() {
    const int K = 6, NU = 3, DSZ = 14 * (14 + 2 * NU + 1);
    scvx::ipm::Consts C{};
    C.K = K; C.max_iter = 30; C.refine = 2; C.retries = 1; C.tol = 1e-6; C.accept = 1e-6;
    C.itan = 2.0; C.sqcm = 0.7; C.icos = 1.1; C.Tmax = 2.0; C.Tmin = 0.5; C.omMax = 1.0; C.mdry = 0.5; C.wNu = 1e3; C.mwet = 1.0;
    C.qBIf[0] = 1.0;
    std::vector<double> x((K + 1) * 14, 0.0), u((K + 1) * NU, 0.0), e(K * 14, 0.0), d((size_t)K * DSZ, 0.0), pm((K + 1) * 4, 0.0);
    for (int k = 0; k <= K; k++) { x[14 * k] = 1.0; x[14 * k + 1] = 1.0 - (double)k / K; x[14 * k + 7] = 1.0; u[NU * k] = 1.0; }
    for (int k = 0; k < K; k++) {
        for (int i = 0; i < 14; i++) { e[14 * k + i] = x[14 * k + i]; d[(size_t)k * DSZ + 14 * i + i] = 1.0; }
    }
    for (int k = 1; k < K; k++) { pm[4 * k] = 0.01; pm[4 * k + 1] = 0.01; pm[4 * k + 2] = 0.05; pm[4 * k + 3] = 0.1; }
    pm[4 * K] = 0.01; pm[2] = 0.05;
    const double rk = 10.0, ic[6] = {1.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    std::vector<double> sol((K + 1) * (14 + NU) + 1), nu(K * 14), info(4);
    for (int with = 0; with < 2; with++) {
        path_margin_port_socp(&C, 1, x.data(), u.data(), e.data(), d.data(), &rk, ic, sol.data(), nu.data(), info.data(), nullptr,
                              with ? pm.data() : nullptr, 3, 0);
        printf("back-offs %d: status %g after %g iterations, merit %.3e\n", with, info[0], info[1], info[2]);
    }
    return 0;
}
#endif
