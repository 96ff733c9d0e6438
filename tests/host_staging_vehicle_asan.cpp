// Stand-alone sanitizer program for the HOST-side staging of the _veh forms of the sampled calls (scvx_track_mc_veh_f64_host,
// scvx_track_mc_nav_veh_f64_host): what they add to the staging of the _q / _rng forms is one upload (zeta [S][6]) and one download
// (theta [B][S][6]).  The HIP runtime, the traffic counters, CALL, Plan and the error sweep are those of tests/host_staging_asan.cpp,
// which is included with its main renamed (its own scenarios run in its own program); zeta and theta are allocated with exactly the
// size include/scvx.h documents, so a staging buffer that is too small or a copy that is too long is an AddressSanitizer report.
//
// Beyond the sanitizers, per scenario: veh = NULL stages exactly what the _q (uploaded draws) or the _rng (device draws) call stages;
// with veh and uploaded draws the call allocates two more buffers, of S 6 and B S 6 doubles, uploads the first and downloads the
// second; with device draws only theta is added; the launches are the same in number.  The error sweep covers both forms.
// tests/test_host_staging_vehicle_sanitizers.py holds the build recipe and runs the program.
#define main host_staging_main
#include "host_staging_asan.cpp"
#undef main

// a = b plus `up` bytes in one more upload and `down` bytes in one more download (0: none), each in a buffer of its own
static bool adds(const Traffic& a, const Traffic& b, size_t up, size_t down) {
    const size_t n = (up ? 1 : 0) + (down ? 1 : 0);
    return a.allocs == b.allocs + n && a.alloc_bytes == b.alloc_bytes + up + down && a.frees == b.frees + n &&
           a.h2d == b.h2d + (up ? 1 : 0) && a.h2d_bytes == b.h2d_bytes + up && a.d2h == b.d2h + (down ? 1 : 0) &&
           a.d2h_bytes == b.d2h_bytes + down && a.memsets == b.memsets && a.launches == b.launches && a.syncs == b.syncs;
}

static int run_veh(int nu, int B, int K, int S, int m, int nq, bool dense, bool noise) {
    g_nu = nu;
    tag("veh", nu, B, K, S, m, nq, dense, noise);
    const int n = 14 + nu;
    V x((size_t)B * (K + 1) * 14, 1.0), u((size_t)B * (K + 1) * nu, 1.0), sg(B, 1.0), gain((size_t)B * K * nu * n), C0((size_t)B * 196),
        xi0((size_t)S * 14), eta((size_t)S * K * 14), sw(14, 1e-3), rep((size_t)B * SCVX_MC_NREP), xm((size_t)B * 14), xc((size_t)B * 196),
        fl((size_t)B * S * SCVX_FLIGHT_NREP), xl((size_t)B * S * 14), d0((size_t)B * S * 14), fq((size_t)B * 16 * nq),
        pq((size_t)B * (K + 1) * 5 * nq), pv((size_t)B * (K + 1) * 5 * S), zeta((size_t)S * SCVX_VEH_N), theta((size_t)B * S * SCVX_VEH_N);
    V deriv((size_t)B * K * 14 * (14 + 2 * nu + 1)), kf((size_t)B * K * 14 * (m ? m : 1)), CN((size_t)B * 196), xin((size_t)S * 14),
        nud((size_t)S * K * (m ? m : 1)), H((size_t)(m ? m : 1) * 14, 0.0), rm(m ? m : 1, 1e-6), jm((size_t)B * 28), jc((size_t)B * 784),
        nv((size_t)B * SCVX_NAV_NREP), fed((size_t)B * S * K * 14), nk((size_t)B * S * 14);
    std::vector<int> ranks(nq);
    for (int i = 0; i < nq; i++) ranks[i] = (i * 7) % S;
    double* const none = nullptr;
    const scvx_mc_rng rng{20261020u, 0u, 0u, 0, 0};
    scvx_mc_vehicle veh{};
    veh.sp[SCVX_VEH_THRUST] = veh.sp[SCVX_VEH_MIS_Z] = veh.sp[SCVX_VEH_ISP] = 1e-3;
    veh.mu[SCVX_VEH_MIS_Y] = 1e-3;
    if (nu == 5) veh.sp[SCVX_VEH_FIN] = 1e-2;
    const size_t zb = zeta.size() * 8, tb = theta.size() * 8;
    const int *rk = nq ? ranks.data() : nullptr;
    double *e = noise ? eta.data() : none, *s = noise ? sw.data() : none, *f = dense ? fl.data() : none, *l = dense ? xl.data() : none,
           *d = dense ? d0.data() : none, *q = nq ? fq.data() : none, *p = nq ? pq.data() : none, *v = dense ? pv.data() : none;
    {   // truth-fed
        scvx_ctx ctx;
        ctx.prob.K = K;
        ctx.dyn.fin = nu == 5;
#define ARGS(xi, et) &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi, et, s, nullptr, 10, 0, 0.0, rep.data(), \
                     xm.data(), xc.data(), f, l, d, nq, rk, q, p, v
        CALL(scvx_track_mc_q_f64_host, ARGS(xi0.data(), e));   // grows the context's workspaces: the calls compared below find them grown
        CALL(scvx_track_mc_q_f64_host, ARGS(xi0.data(), e));
        const Traffic tq = g_t;
        CALL(scvx_track_mc_veh_f64_host, ARGS(xi0.data(), e), nullptr, 0, nullptr, none, none);
        REQUIRE(adds(g_t, tq, 0, 0));
        CALL(scvx_track_mc_veh_f64_host, ARGS(xi0.data(), e), nullptr, 0, &veh, zeta.data(), theta.data());
        REQUIRE(adds(g_t, tq, zb, tb));
        CALL(scvx_track_mc_veh_f64_host, ARGS(xi0.data(), e), nullptr, 0, &veh, zeta.data(), none);
        REQUIRE(adds(g_t, tq, zb, 0));
        CALL(scvx_track_mc_rng_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), &rng, noise ? 1 : 0, s, nullptr,
             10, 0, 0.0, rep.data(), xm.data(), xc.data(), f, l, d, nq, rk, q, p, v);
        const Traffic tr = g_t;
        CALL(scvx_track_mc_veh_f64_host, ARGS(none, none), &rng, noise ? 1 : 0, nullptr, none, none);
        REQUIRE(adds(g_t, tr, 0, 0));
        CALL(scvx_track_mc_veh_f64_host, ARGS(none, none), &rng, noise ? 1 : 0, &veh, none, theta.data());
        REQUIRE(adds(g_t, tr, 0, tb));
#undef ARGS
        // refusals before any staging: nothing is allocated
        const size_t a0 = g_allocs;
        veh.reserved[1] = 1;
        REQUIRE(scvx_track_mc_veh_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), none, none, nullptr,
                                           10, 0, 0.0, rep.data(), xm.data(), xc.data(), none, none, none, 0, nullptr, none, none, none, nullptr,
                                           0, &veh, zeta.data(), theta.data()) == SCVX_ERR_ARG);
        veh.reserved[1] = 0;
        REQUIRE(scvx_track_mc_veh_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), none, none, nullptr,
                                           10, 0, 0.0, rep.data(), xm.data(), xc.data(), none, none, none, 0, nullptr, none, none, none, &rng, 0,
                                           &veh, none, theta.data()) == SCVX_ERR_ARG);   // rng with an uploaded xi0
        REQUIRE(g_allocs == a0);
        scvx::mc_workspace_free(&ctx);
    }
    {   // flown on an estimate
        scvx_ctx ctx;
        ctx.prob.K = K;
        ctx.dyn.fin = nu == 5;
        double *kk = m ? kf.data() : none, *nn = m ? nud.data() : none, *hh = m ? H.data() : none, *rr = m ? rm.data() : none,
               *fe = dense ? fed.data() : none, *k2 = dense ? nk.data() : none;
#define ARGS(xi, et, xn, nd) &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi, et, s, deriv.data(), kk, CN.data(), xn, nd, \
                             m, hh, rr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), jm.data(), jc.data(), nv.data(), f, l, d, fe, k2, nq, rk, q, \
                             p, v
        CALL(scvx_track_mc_nav_q_f64_host, ARGS(xi0.data(), e, xin.data(), nn));   // grows the workspaces
        CALL(scvx_track_mc_nav_q_f64_host, ARGS(xi0.data(), e, xin.data(), nn));
        const Traffic tq = g_t;
        CALL(scvx_track_mc_nav_veh_f64_host, ARGS(xi0.data(), e, xin.data(), nn), nullptr, 0, nullptr, none, none);
        REQUIRE(adds(g_t, tq, 0, 0));
        CALL(scvx_track_mc_nav_veh_f64_host, ARGS(xi0.data(), e, xin.data(), nn), nullptr, 0, &veh, zeta.data(), theta.data());
        REQUIRE(adds(g_t, tq, zb, tb));
        CALL(scvx_track_mc_nav_rng_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), &rng, noise ? 1 : 0, s,
             deriv.data(), kk, CN.data(), m, hh, rr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), jm.data(), jc.data(), nv.data(), f, l, d, fe,
             k2, nq, rk, q, p, v);
        const Traffic tr = g_t;
        CALL(scvx_track_mc_nav_veh_f64_host, ARGS(none, none, none, none), &rng, noise ? 1 : 0, nullptr, none, none);
        REQUIRE(adds(g_t, tr, 0, 0));
        CALL(scvx_track_mc_nav_veh_f64_host, ARGS(none, none, none, none), &rng, noise ? 1 : 0, &veh, none, theta.data());
        REQUIRE(adds(g_t, tr, 0, tb));
#undef ARGS
        scvx::mc_workspace_free(&ctx);
    }
    return 0;
}

static int veh_error_paths() {
    const int nu = 3, B = 2, K = 2, S = 3, m = 2, nq = 2;
    Plan p(nu, B, K, S, m);
    V C0((size_t)B * 196), xi0((size_t)S * 14), eta((size_t)S * K * 14), xin((size_t)S * 14), nud((size_t)S * K * m), rep((size_t)B * SCVX_MC_NREP),
        xm((size_t)B * 14), xc((size_t)B * 196), fl((size_t)B * S * SCVX_FLIGHT_NREP), xl((size_t)B * S * 14), d0((size_t)B * S * 14),
        fq((size_t)B * 16 * nq), pq((size_t)B * (K + 1) * 5 * nq), pv((size_t)B * (K + 1) * 5 * S), jm((size_t)B * 28), jc((size_t)B * 784),
        fed((size_t)B * S * K * 14), nk((size_t)B * S * 14), zeta((size_t)S * SCVX_VEH_N), theta((size_t)B * S * SCVX_VEH_N);
    std::vector<int> ranks = {0, 2};
    scvx_mc_vehicle veh{};
    veh.sp[SCVX_VEH_THRUST] = 1e-3;
#define SWEEP(name, ...) \
    if (sweep(#name, K, nu, [&](scvx_ctx* c) { return name(c, __VA_ARGS__); })) return 1
    SWEEP(scvx_track_mc_veh_f64_host, B, K, S, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), C0.data(), xi0.data(), eta.data(),
          p.w.data(), nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), fl.data(), xl.data(), d0.data(), nq, ranks.data(), fq.data(),
          pq.data(), pv.data(), nullptr, 0, &veh, zeta.data(), theta.data());
    SWEEP(scvx_track_mc_nav_veh_f64_host, B, K, S, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), C0.data(), xi0.data(), eta.data(),
          p.w.data(), p.deriv.data(), p.kf.data(), p.N0.data(), xin.data(), nud.data(), m, p.H.data(), p.rm.data(), 10, 0, 0.0, rep.data(),
          xm.data(), xc.data(), jm.data(), jc.data(), p.nrep.data(), fl.data(), xl.data(), d0.data(), fed.data(), nk.data(), nq, ranks.data(),
          fq.data(), pq.data(), pv.data(), nullptr, 0, &veh, zeta.data(), theta.data());
#undef SWEEP
    return 0;
}

int main() {
    if (refusals(true)) return 1;   // the _veh forms of the table of tests/host_staging_asan.cpp
    for (int nu : {3, 5})
        for (int m : {0, 6})
            for (int nq : {0, 16})
                for (int dense = 0; dense < 2; dense++)
                    if (run_veh(nu, 3, 4, 70, m, nq, dense != 0, m != 0)) return 1;
    if (run_veh(3, 1, 1, 1, 0, 1, true, false)) return 1;
    fflush(stdout);
    if (veh_error_paths()) return 1;
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers on\n");
#endif
#endif
    printf("host staging (vehicle errors): %zu allocations, %zu frees, %zu launches\n", g_allocs, g_frees, g_launches);
    return g_allocs == g_frees ? 0 : 1;
}
