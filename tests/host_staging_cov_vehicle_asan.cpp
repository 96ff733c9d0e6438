// Stand-alone sanitizer program for the HOST-side staging of the vehicle errors in the first-order analyses (scvx_vehicle_tiles_f64_host,
// scvx_cov_vehicle_f64_host, scvx_nav_cov_vehicle_f64_host).  The HIP runtime, the traffic counters, CALL, Plan and the error sweep are
// those of tests/host_staging_asan.cpp, which is included with its main renamed (its own scenarios run in its own program); vtile and
// sens are allocated with exactly the size include/scvx.h documents, so a staging buffer that is too small or a copy that is too long
// is an AddressSanitizer report.
//
// Beyond the sanitizers, per scenario: without vtile, sens and the dense outputs the covariance form stages exactly what
// scvx_cov_path_sigma_f64_host stages and the navigation form what scvx_nav_path_sigma_f64_host stages; vtile costs one upload of
// B K 2 14 doubles, sens one download of B (K + 1) n 6 doubles, every dense output one download of its documented size, psig = NULL one
// download less; the launches are the same in number.  The tile call stages three uploads and one download.  A refusal allocates
// nothing.  The error sweep covers the three forms.  cov_refusals(true) pins what the _vehicle forms refuse, in which words, and which
// of two faults wins (tests/golden/cov_refusals.txt).  tests/test_host_staging_cov_vehicle_sanitizers.py holds the build recipe.
#define main host_staging_main
#include "host_staging_asan.cpp"
#undef main

// a = b plus nup uploads of `up` bytes and ndown downloads of `down` bytes in all, each in a buffer of its own
static bool adds(const Traffic& a, const Traffic& b, size_t nup, size_t up, size_t ndown, size_t down) {
    const size_t n = nup + ndown;
    return a.allocs == b.allocs + n && a.alloc_bytes == b.alloc_bytes + up + down && a.frees == b.frees + n && a.h2d == b.h2d + nup &&
           a.h2d_bytes == b.h2d_bytes + up && a.d2h == b.d2h + ndown && a.d2h_bytes == b.d2h_bytes + down && a.memsets == b.memsets &&
           a.launches == b.launches && a.syncs == b.syncs;
}

static int run_veh(int nu, int B, int K, int m) {
    g_nu = nu;
    tag("covveh", nu, B, K, 0, m, 0, 0, 0);
    Plan p(nu, B, K, 1, m);
    const int n = 14 + nu;
    V vtile((size_t)B * K * SCVX_VTILE_N * 14), sens((size_t)B * (K + 1) * n * SCVX_VEH_N);
    double sp[SCVX_VEH_N] = {1e-3, 1e-3, 0.0, 1e-3, 0.0, 0.0}, spc[SCVX_VEH_N] = {1e-3, 0.0, 1e-3, 0.0, 0.0, 0.0};
    if (nu == 5) sp[SCVX_VEH_FIN] = 1e-2;
    double* const none = nullptr;
    double *Hm = m ? p.H.data() : nullptr, *rmm = m ? p.rm.data() : nullptr;
    const size_t vb = vtile.size() * 8, sb = sens.size() * 8, pb = p.psig.size() * 8;
    scvx_ctx ctx;
    ctx.prob.K = K;
    ctx.dyn.fin = nu == 5;
    // the tiles: x, u, sigma up, vtile down, one launch
    CALL(scvx_vehicle_tiles_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.sg.data(), vtile.data());
    REQUIRE(g_t.allocs == 4 && g_t.h2d == 3 && g_t.d2h == 1 && g_t.d2h_bytes == vb && g_t.launches == 1 && g_t.frees == 4);
    // the covariance form
#define ARGS &ctx, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.w.data(), p.crep.data()
    CALL(scvx_cov_path_sigma_f64_host, ARGS, p.psig.data());
    const Traffic tc = g_t;
    CALL(scvx_cov_vehicle_f64_host, ARGS, p.psig.data(), none, none, none, none, spc, none);
    REQUIRE(adds(g_t, tc, 0, 0, 0, 0));
    CALL(scvx_cov_vehicle_f64_host, ARGS, p.psig.data(), none, none, none, vtile.data(), sp, sens.data());
    REQUIRE(adds(g_t, tc, 1, vb, 1, sb));
    CALL(scvx_cov_vehicle_f64_host, ARGS, p.psig.data(), p.sig.data(), p.covK.data(), p.cov.data(), vtile.data(), sp, none);
    REQUIRE(adds(g_t, tc, 1, vb, 3, (p.sig.size() + p.covK.size() + p.cov.size()) * 8));
    CALL(scvx_cov_vehicle_f64_host, ARGS, none, p.sig.data(), none, none, vtile.data(), sp, sens.data());
    REQUIRE(adds(g_t, tc, 1, vb, 1, sb + p.sig.size() * 8 - pb));
    // refusals before any staging: nothing is allocated
    const size_t a0 = g_allocs;
    double bad[SCVX_VEH_N] = {-1e-3, 0.0, 0.0, 0.0, 0.0, 0.0}, aero[SCVX_VEH_N] = {0.0, 0.0, 0.0, 0.0, 1e-3, 0.0};
    REQUIRE(scvx_cov_vehicle_f64_host(ARGS, p.psig.data(), none, none, none, vtile.data(), bad, none) == SCVX_ERR_ARG);
    REQUIRE(scvx_cov_vehicle_f64_host(ARGS, p.psig.data(), none, none, none, vtile.data(), aero, none) == SCVX_ERR_ARG);
    REQUIRE(scvx_cov_vehicle_f64_host(ARGS, p.psig.data(), none, none, none, none, sp, none) == SCVX_ERR_ARG);       // ISP without the tiles
    REQUIRE(scvx_cov_vehicle_f64_host(ARGS, p.psig.data(), none, none, none, vtile.data(), nullptr, none) == SCVX_ERR_ARG);
    REQUIRE(scvx_vehicle_tiles_f64_host(&ctx, B, K, p.x.data(), p.u.data(), none, vtile.data()) == SCVX_ERR_ARG);
    REQUIRE(g_allocs == a0);
#undef ARGS
    // the navigation form
#define ARGS &ctx, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.N0.data(), m, Hm, rmm, p.w.data(), p.crep.data(), \
             p.nrep.data()
    CALL(scvx_nav_path_sigma_f64_host, ARGS, p.psig.data());
    const Traffic tn = g_t;
    CALL(scvx_nav_cov_vehicle_f64_host, ARGS, p.psig.data(), none, none, none, none, none, spc, none);
    REQUIRE(adds(g_t, tn, 0, 0, 0, 0));
    CALL(scvx_nav_cov_vehicle_f64_host, ARGS, p.psig.data(), none, none, none, none, vtile.data(), sp, sens.data());
    REQUIRE(adds(g_t, tn, 1, vb, 1, sb));
    CALL(scvx_nav_cov_vehicle_f64_host, ARGS, p.psig.data(), p.sig.data(), p.navsig.data(), p.kf.data(), p.joint.data(), vtile.data(), sp,
         sens.data());
    REQUIRE(adds(g_t, tn, 1, vb, m ? 5 : 4, sb + (p.sig.size() + p.navsig.size() + (m ? p.kf.size() : 0) + p.joint.size()) * 8));
    const size_t a1 = g_allocs;
    REQUIRE(scvx_nav_cov_vehicle_f64_host(ARGS, p.psig.data(), none, none, none, none, vtile.data(), bad, none) == SCVX_ERR_ARG);
    REQUIRE(scvx_nav_cov_vehicle_f64_host(ARGS, p.psig.data(), none, none, none, none, none, sp, none) == SCVX_ERR_ARG);
    REQUIRE(g_allocs == a1);
#undef ARGS
    return 0;
}

static int veh_error_paths() {
    const int nu = 3, B = 2, K = 2, m = 2;
    Plan p(nu, B, K, 1, m);
    V vtile((size_t)B * K * SCVX_VTILE_N * 14), sens((size_t)B * (K + 1) * (14 + nu) * SCVX_VEH_N);
    double sp[SCVX_VEH_N] = {1e-3, 0.0, 0.0, 1e-3, 0.0, 0.0};
#define SWEEP(name, ...) \
    if (sweep(#name, K, nu, [&](scvx_ctx* c) { return name(c, __VA_ARGS__); })) return 1
    SWEEP(scvx_vehicle_tiles_f64_host, B, K, p.x.data(), p.u.data(), p.sg.data(), vtile.data());
    SWEEP(scvx_cov_vehicle_f64_host, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.w.data(), p.crep.data(),
          p.psig.data(), p.sig.data(), p.covK.data(), p.cov.data(), vtile.data(), sp, sens.data());
    SWEEP(scvx_nav_cov_vehicle_f64_host, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.N0.data(), m, p.H.data(),
          p.rm.data(), p.w.data(), p.crep.data(), p.nrep.data(), p.psig.data(), p.sig.data(), p.navsig.data(), p.kf.data(), p.joint.data(),
          vtile.data(), sp, sens.data());
#undef SWEEP
    return 0;
}

int main() {
    if (cov_refusals(true)) return 1;   // the _vehicle forms of the table of tests/host_staging_asan.cpp
    for (int nu : {3, 5})
        for (int m : {0, 6})
            if (run_veh(nu, 3, 4, m)) return 1;
    if (run_veh(3, 1, 1, 0)) return 1;
    fflush(stdout);
    if (veh_error_paths()) return 1;
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers on\n");
#endif
#endif
    printf("host staging (vehicle errors, first-order analyses): %zu allocations, %zu frees, %zu launches\n", g_allocs, g_frees, g_launches);
    return g_allocs == g_frees ? 0 : 1;
}
