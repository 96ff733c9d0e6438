// Stand-alone sanitizer program for the HOST-side staging of the _host forms: the sampled calls and the order statistics
// (scvx_track_mc[_nav]_q_f64_host, their _rng forms and the old forms through them, scvx_mc_draws_f64_host, scvx_order_stats_f64_host),
// the covariance and navigation analyses (scvx_cov_*_f64_host, scvx_nav_*_f64_host) and plan tracking (scvx_track_*_f64_host).
//
// Built WITHOUT a GPU runtime: the translation units are compiled for the host only (hipcc --cuda-host-only), every sanitizer option
// passed to the host compilation alone (-Xarch_host), and linked against the small HIP runtime below, in which "device" memory is host
// memory from malloc, sized exactly as the call asked, a copy is a memcpy and a kernel launch does nothing.  Every array this program
// hands in is allocated with exactly the size include/scvx.h documents, so a staging buffer that is too small, a copy that is too long on
// either side, a leak or a use after free in the staging code is an AddressSanitizer report.  No kernel runs: the outputs are whatever
// the "device" buffers held (zeroed here), and nothing about them is checked.
//
// The runtime also counts.  Every successful call prints one "traffic" line: allocations and their bytes, frees, uploads and downloads
// and their bytes, memsets, launches, synchronises.  tests/golden/host_staging_traffic.txt holds the lines this program printed when it
// was linked against the staging code as it stood BEFORE csrc/scvx_stage.hpp existed; the test requires the same lines, so the staging
// helper allocates, copies, launches and synchronises exactly what the hand-written sequences did.  And the runtime can make the n-th
// hipMalloc, hipMemcpyAsync or launch of a call fail: sweep() does that at every position of one small call of every form and checks the
// error contract of scvx::Staging.  tests/test_host_staging_sanitizers.py holds the build recipe and runs the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>
#include "scvx_mc.hpp"

// ---- the HIP runtime of this program -------------------------------------------------------------------------------------------------
struct Traffic {
    size_t allocs, alloc_bytes, frees, h2d, h2d_bytes, d2h, d2h_bytes, memsets, launches, syncs;
};
static Traffic g_t{};
static size_t g_allocs = 0, g_frees = 0, g_launches = 0;   // of the whole run
static std::string g_log;           // one letter per runtime call since the last reset: Alloc, Free, Copy, Memset, Launch, Sync
static char g_fail_kind = 0;        // 'A', 'C' or 'L': that kind's g_fail_at-th call since the last reset fails; 0: nothing fails
static size_t g_fail_at = 0, g_failed_pos = std::string::npos;   // g_failed_pos: the failing call's place in g_log
static hipError_t g_last = hipSuccess;

static void reset_traffic() {
    g_t = Traffic{};
    g_log.clear();
    g_failed_pos = std::string::npos;
    g_last = hipSuccess;
}
static size_t count(char kind) {
    size_t n = 0;
    for (char c : g_log) n += c == kind;
    return n;
}
// logs the call; true when it is the one that has to fail
static bool event(char kind) {
    g_log.push_back(kind);
    if (kind != g_fail_kind || count(kind) != g_fail_at) return false;
    g_failed_pos = g_log.size() - 1;
    return true;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    *p = nullptr;
    if (event('A')) return hipErrorOutOfMemory;
    *p = calloc(n ? n : 1, 1);
    g_allocs++, g_t.allocs++, g_t.alloc_bytes += n;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    event('F');
    free(p);
    g_frees++, g_t.frees++;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind kind, hipStream_t) {
    if (event('C')) return hipErrorInvalidValue;
    memcpy(d, s, n);
    if (kind == hipMemcpyHostToDevice) g_t.h2d++, g_t.h2d_bytes += n;
    else g_t.d2h++, g_t.d2h_bytes += n;
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
    event('M');
    memset(d, v, n);
    g_t.memsets++;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    event('S');
    g_t.syncs++;
    return hipSuccess;
}
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) {
    const hipError_t e = g_last;
    g_last = hipSuccess;
    return e;
}
const char* hipGetErrorString(hipError_t) { return "shim"; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) {
    if (event('L')) return g_last = hipErrorLaunchFailure;
    g_launches++, g_t.launches++;
    return hipSuccess;
}
static dim3 g_grid, g_block;
static size_t g_shmem;
static hipStream_t g_stream;
hipError_t __hipPushCallConfiguration(dim3 g, dim3 b, size_t s, hipStream_t st) {
    g_grid = g, g_block = b, g_shmem = s, g_stream = st;
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* g, dim3* b, size_t* s, hipStream_t* st) {
    *g = g_grid, *b = g_block, *s = g_shmem, *st = g_stream;
    return hipSuccess;
}
void** __hipRegisterFatBinary(const void*) {
    static void* h;
    return &h;
}
void __hipRegisterFunction(void**, const void*, char*, const char*, unsigned, void*, void*, void*, void*, int*) {}
void __hipRegisterVar(void**, void*, char*, char*, int, size_t, int, int) {}
void __hipUnregisterFatBinary(void**) {}
}

// ---- what the translation units take from the rest of the library ---------------------------------------------------------------------
static int g_nu = 3;
extern "C" int scvx_control_dim(const scvx_ctx*) { return g_nu; }
namespace scvx {
PathK path_constants(const scvx_problem&) { return PathK{}; }
// the two closed-loop flights of scvx_flight.hip: one kernel launch each
hipError_t launch_track_fly(const scvx_ctx*, int, int, const double*, const double*, const double*, const double*, const double*, int, int,
                            double*, double*, double*, hipStream_t st) {
    (void)hipLaunchKernel(nullptr, dim3(1), dim3(64), nullptr, 0, st);
    return hipGetLastError();
}
hipError_t launch_track_fly_nav(const scvx_ctx*, int, int, const double*, const double*, const double*, const double*, const double*,
                                const double*, int, int, double*, double*, double*, hipStream_t st) {
    (void)hipLaunchKernel(nullptr, dim3(1), dim3(64), nullptr, 0, st);
    return hipGetLastError();
}
}  // namespace scvx

typedef std::vector<double> V;
#define REQUIRE(c)                                                  \
    do {                                                            \
        if (!(c)) {                                                 \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
            return 1;                                               \
        }                                                           \
    } while (0)

static std::string g_tag;   // the scenario, in front of every traffic line
// one call that must succeed, and its traffic line
#define CALL(name, ...)                                                                                                                   \
    do {                                                                                                                                  \
        reset_traffic();                                                                                                                  \
        REQUIRE(name(__VA_ARGS__) == SCVX_OK);                                                                                            \
        printf("traffic %s %s: alloc %zu / %zu B, free %zu, h2d %zu / %zu B, d2h %zu / %zu B, memset %zu, launch %zu, sync %zu\n",         \
               g_tag.c_str(), #name, g_t.allocs, g_t.alloc_bytes, g_t.frees, g_t.h2d, g_t.h2d_bytes, g_t.d2h, g_t.d2h_bytes, g_t.memsets, \
               g_t.launches, g_t.syncs);                                                                                                  \
    } while (0)

static void tag(const char* what, int nu, int B, int K, int S, int m, int nq, int opt, int noise) {
    char buf[160];
    snprintf(buf, sizeof buf, "%s nu=%d B=%d K=%d S=%d m=%d nq=%d opt=%d noise=%d", what, nu, B, K, S, m, nq, opt, noise);
    g_tag = buf;
}

// the sampled calls; a fresh context every time, so the workspace the launches grow is part of every line
static int run(int nu, int B, int K, int S, int m, int nq, bool dense, bool noise) {
    g_nu = nu;
    tag("mc", nu, B, K, S, m, nq, dense, noise);
    const int n = 14 + nu;
    V x((size_t)B * (K + 1) * 14, 1.0), u((size_t)B * (K + 1) * nu, 1.0), sg(B, 1.0), gain((size_t)B * K * nu * n), C0((size_t)B * 196),
        xi0((size_t)S * 14), eta((size_t)S * K * 14), sw(14, 1e-3), rep((size_t)B * SCVX_MC_NREP), xm((size_t)B * 14), xc((size_t)B * 196),
        fl((size_t)B * S * SCVX_FLIGHT_NREP), xl((size_t)B * S * 14), d0((size_t)B * S * 14), fq((size_t)B * 16 * nq),
        pq((size_t)B * (K + 1) * 5 * nq), pv((size_t)B * (K + 1) * 5 * S);
    std::vector<int> ranks(nq);
    for (int i = 0; i < nq; i++) ranks[i] = (i * 7) % S;
    double* const none = nullptr;
    const scvx_mc_rng rng{20261020u, 0u, 0u, 0, 0};
    V deriv((size_t)B * K * 14 * (14 + 2 * nu + 1)), kf((size_t)B * K * 14 * (m ? m : 1)), CN((size_t)B * 196), xin((size_t)S * 14),
        nud((size_t)S * K * (m ? m : 1)), H((size_t)(m ? m : 1) * 14, 0.0), rm(m ? m : 1, 1e-6), jm((size_t)B * 28), jc((size_t)B * 784),
        nv((size_t)B * SCVX_NAV_NREP), fed((size_t)B * S * K * 14), nk((size_t)B * S * 14);
    {   // truth-fed
        scvx_ctx ctx;
        ctx.prob.K = K;
        CALL(scvx_track_mc_q_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(),
             noise ? eta.data() : none, noise ? sw.data() : none, nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(),
             dense ? fl.data() : none, dense ? xl.data() : none, dense ? d0.data() : none, nq, nq ? ranks.data() : nullptr,
             nq ? fq.data() : none, nq ? pq.data() : none, dense ? pv.data() : none);
        CALL(scvx_track_mc_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(),
             noise ? eta.data() : none, noise ? sw.data() : none, nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(),
             dense ? fl.data() : none, none, none);
        CALL(scvx_track_mc_rng_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), &rng, noise ? 1 : 0,
             noise ? sw.data() : none, nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), dense ? fl.data() : none,
             dense ? xl.data() : none, dense ? d0.data() : none, nq, nq ? ranks.data() : nullptr, nq ? fq.data() : none,
             nq ? pq.data() : none, dense ? pv.data() : none);
        // a refusal after the old checks and before any staging: nothing is allocated
        if (nq) {
            const size_t a0 = g_allocs;
            const int r0 = ranks[0];
            ranks[0] = S;
            int rc = scvx_track_mc_q_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), none, none,
                                              nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), none, none, none, nq, ranks.data(),
                                              fq.data(), none, none);
            REQUIRE(rc == SCVX_ERR_ARG && g_allocs == a0);
            ranks[0] = r0;
        }
        scvx::mc_workspace_free(&ctx);
    }
    {   // flown on an estimate
        scvx_ctx ctx;
        ctx.prob.K = K;
        CALL(scvx_track_mc_nav_q_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(),
             noise ? eta.data() : none, noise ? sw.data() : none, deriv.data(), m ? kf.data() : none, CN.data(), xin.data(),
             m ? nud.data() : none, m, m ? H.data() : none, m ? rm.data() : none, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), jm.data(),
             jc.data(), nv.data(), dense ? fl.data() : none, dense ? xl.data() : none, dense ? d0.data() : none, dense ? fed.data() : none,
             dense ? nk.data() : none, nq, nq ? ranks.data() : nullptr, nq ? fq.data() : none, nq ? pq.data() : none,
             dense ? pv.data() : none);
        CALL(scvx_track_mc_nav_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), none, none,
             deriv.data(), m ? kf.data() : none, CN.data(), xin.data(), m ? nud.data() : none, m, m ? H.data() : none, m ? rm.data() : none,
             10, 0, 0.0, rep.data(), xm.data(), xc.data(), jm.data(), jc.data(), nv.data(), none, none, none, none, none);
        CALL(scvx_track_mc_nav_rng_f64_host, &ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), &rng, noise ? 1 : 0,
             noise ? sw.data() : none, deriv.data(), m ? kf.data() : none, CN.data(), m, m ? H.data() : none, m ? rm.data() : none, 10, 0,
             0.0, rep.data(), xm.data(), xc.data(), jm.data(), jc.data(), nv.data(), dense ? fl.data() : none, dense ? xl.data() : none,
             dense ? d0.data() : none, dense ? fed.data() : none, dense ? nk.data() : none, nq, nq ? ranks.data() : nullptr,
             nq ? fq.data() : none, nq ? pq.data() : none, dense ? pv.data() : none);
        scvx::mc_workspace_free(&ctx);
    }
    return 0;
}

// the arrays of the analyses and of plan tracking, each of exactly its documented size
struct Plan {
    int nu, B, K, S, m, n, N;
    V x, u, sg, deriv, gain, p0, S0, N0, H, rm, w, q, r, qf, dx0, nav, frep, xfly, ufly, crep, nrep, sig, covK, cov, psig, navsig, kf, joint,
        xi0, eta, xin, nud;
    scvx_mc_rng rng{20261020u, 0u, 0u, 1, 0};
    Plan(int nu_, int B_, int K_, int S_, int m_)
        : nu(nu_), B(B_), K(K_), S(S_), m(m_), n(14 + nu_), N(28 + nu_), x((size_t)B * (K + 1) * 14, 1.0), u((size_t)B * (K + 1) * nu, 1.0),
          sg(B, 1.0), deriv((size_t)B * K * 14 * (14 + 2 * nu + 1)), gain((size_t)B * K * nu * n), p0((size_t)B * n * n), S0((size_t)B * 196),
          N0((size_t)B * 196), H((size_t)(m ? m : 1) * 14, 0.0), rm(m ? m : 1, 1e-6), w(14, 1e-6), q(14, 1.0), r(nu, 1.0), qf(14, 1.0),
          dx0((size_t)B * 14), nav((size_t)B * K * 14), frep((size_t)B * SCVX_FLIGHT_NREP), xfly((size_t)B * (K + 1) * 14),
          ufly((size_t)B * (K + 1) * nu), crep((size_t)B * SCVX_COV_NREP), nrep((size_t)B * SCVX_NAV_NREP), sig((size_t)B * (K + 1) * n),
          covK((size_t)B * n * n), cov((size_t)B * (K + 1) * n * n), psig((size_t)B * (K + 1) * SCVX_PSIG_N), navsig((size_t)B * (K + 1) * 14),
          kf((size_t)B * K * 14 * (m ? m : 1)), joint((size_t)B * (K + 1) * N * N), xi0((size_t)B * S * 14), eta((size_t)B * S * K * 14),
          xin((size_t)B * S * 14), nud((size_t)B * S * K * 14) {}
};

// the forms of scvx_cov.hip, scvx_nav.hip and scvx_track.hip and the draws; opt: every optional array present (1) or absent (0)
static int analyses(int nu, int B, int K, int S, int m, bool opt) {
    g_nu = nu;
    tag("plan", nu, B, K, S, m, 0, opt, 0);
    Plan p(nu, B, K, S, m);
    scvx_ctx ctx;
    ctx.prob.K = K;
    ctx.dyn.fin = nu == 5;
    auto o = [&](V& v) { return opt ? v.data() : nullptr; };
    double *Hm = m ? p.H.data() : nullptr, *rmm = m ? p.rm.data() : nullptr;
    CALL(scvx_track_gains_f64_host, &ctx, B, K, p.deriv.data(), p.q.data(), p.r.data(), p.qf.data(), p.gain.data(), o(p.p0));
    CALL(scvx_track_fly_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), o(p.dx0), 10, 0, p.frep.data(), o(p.xfly),
         o(p.ufly));
    CALL(scvx_track_fly_nav_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), o(p.dx0), p.nav.data(), 10, 0,
         p.frep.data(), o(p.xfly), o(p.ufly));
    CALL(scvx_cov_propagate_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), o(p.w), p.crep.data(),
         o(p.sig), o(p.covK), o(p.cov));
    CALL(scvx_cov_path_sigma_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), o(p.w), p.crep.data(),
         p.psig.data());
    CALL(scvx_nav_cov_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.N0.data(), m, Hm, rmm, o(p.w),
         p.crep.data(), p.nrep.data(), o(p.sig), o(p.navsig), o(p.kf), o(p.joint));
    CALL(scvx_nav_path_sigma_f64_host, &ctx, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.N0.data(), m, Hm,
         rmm, o(p.w), p.crep.data(), p.nrep.data(), p.psig.data());
    CALL(scvx_mc_draws_f64_host, &ctx, &p.rng, B, S, K, o(p.xi0), o(p.eta), o(p.xin), o(p.nud));
    return 0;
}

static int order_stats(int R, int S, size_t inc, int nq) {
    scvx_ctx ctx;
    tag("order", 0, R, (int)inc, S, 0, nq, 0, 0);
    const size_t ld = (size_t)(S - 1) * inc + 3;
    V v((size_t)(R - 1) * ld + (size_t)(S - 1) * inc + 1, 0.5), out((size_t)R * nq);   // the last row is NOT padded
    std::vector<int> ranks(nq, S - 1);
    CALL(scvx_order_stats_f64_host, &ctx, R, S, v.data(), ld, inc, nq, ranks.data(), out.data());
    REQUIRE(scvx_order_stats_f64_host(&ctx, R, S, v.data(), ld, inc, SCVX_Q_MAX + 1, ranks.data(), out.data()) == SCVX_ERR_ARG);
    return 0;
}

// ---- the error path --------------------------------------------------------------------------------------------------------------------
// One call of one form, with every hipMalloc, hipMemcpyAsync and launch in turn made to fail.  Required of each: SCVX_ERR_HIP; nothing
// allocated, copied, set or launched after the failing call; exactly one synchronise after it, before the first free; every allocation
// freed (the context's workspace by mc_workspace_free); the message begins with the exported name.
static int sweep(const char* entry, int K, int nu, const std::function<int(scvx_ctx*)>& call) {
    g_nu = nu;
    size_t total[3] = {0, 0, 0};
    const char kinds[3] = {'A', 'C', 'L'};
    for (int pass = 0; pass < 4; pass++)                                            // pass 0: nothing fails, the calls are counted
        for (size_t at = 1; at <= (pass == 0 ? 1 : total[pass - 1]); at++) {
            scvx_ctx ctx;
            ctx.prob.K = K;
            ctx.dyn.fin = nu == 5;
            g_fail_kind = pass == 0 ? 0 : kinds[pass - 1], g_fail_at = at;
            const size_t a0 = g_allocs, f0 = g_frees;
            reset_traffic();
            const int rc = call(&ctx);
            g_fail_kind = 0;
            const std::string log = g_log;
            const size_t pos = g_failed_pos;
            scvx::mc_workspace_free(&ctx);
            REQUIRE(g_allocs - a0 == g_frees - f0);
            if (pass == 0) {
                REQUIRE(rc == SCVX_OK && total[0] + total[1] + total[2] == 0);
                for (int k = 0; k < 3; k++)
                    for (char c : log) total[k] += c == kinds[k];
                REQUIRE(total[0] > 0 && total[1] > 0 && total[2] > 0);
                continue;
            }
            if (rc != SCVX_ERR_HIP || pos == std::string::npos || ctx.err.rfind(std::string(entry) + ": ", 0) != 0) {
                fprintf(stderr, "%s: %c %zu: rc %d, message '%s', calls %s\n", entry, kinds[pass - 1], at, rc, ctx.err.c_str(), log.c_str());
                return 1;
            }
            const std::string after = log.substr(pos + 1);
            const size_t sync = after.find('S'), fr = after.find('F');
            if (after.find_first_of("ACML") != std::string::npos || sync == std::string::npos || after.find('S', sync + 1) != std::string::npos ||
                (fr != std::string::npos && fr < sync)) {
                fprintf(stderr, "%s: %c %zu: calls %s, after the failure %s\n", entry, kinds[pass - 1], at, log.c_str(), after.c_str());
                return 1;
            }
        }
    printf("error path %s: %zu allocations, %zu copies, %zu launches made to fail\n", entry, total[0], total[1], total[2]);
    return 0;
}

static int error_paths() {
    const int nu = 3, B = 2, K = 2, S = 3, m = 2, nq = 2;
    Plan p(nu, B, K, S, m);
    V C0((size_t)B * 196), xi0((size_t)S * 14), eta((size_t)S * K * 14), xin((size_t)S * 14), nud((size_t)S * K * m), rep((size_t)B * SCVX_MC_NREP),
        xm((size_t)B * 14), xc((size_t)B * 196), fl((size_t)B * S * SCVX_FLIGHT_NREP), xl((size_t)B * S * 14), d0((size_t)B * S * 14),
        fq((size_t)B * 16 * nq), pq((size_t)B * (K + 1) * 5 * nq), pv((size_t)B * (K + 1) * 5 * S), jm((size_t)B * 28), jc((size_t)B * 784),
        fed((size_t)B * S * K * 14), nk((size_t)B * S * 14), ov((size_t)B * nq);
    std::vector<int> ranks = {0, 2};
#define SWEEP(name, ...) \
    if (sweep(#name, K, nu, [&](scvx_ctx* c) { return name(c, __VA_ARGS__); })) return 1
    SWEEP(scvx_track_gains_f64_host, B, K, p.deriv.data(), p.q.data(), p.r.data(), p.qf.data(), p.gain.data(), p.p0.data());
    SWEEP(scvx_track_fly_f64_host, B, K, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), p.dx0.data(), 10, 0, p.frep.data(),
          p.xfly.data(), p.ufly.data());
    SWEEP(scvx_track_fly_nav_f64_host, B, K, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), p.dx0.data(), p.nav.data(), 10, 0,
          p.frep.data(), p.xfly.data(), p.ufly.data());
    SWEEP(scvx_cov_propagate_f64_host, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.w.data(), p.crep.data(),
          p.sig.data(), p.covK.data(), p.cov.data());
    SWEEP(scvx_cov_path_sigma_f64_host, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.w.data(), p.crep.data(),
          p.psig.data());
    SWEEP(scvx_nav_cov_f64_host, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.N0.data(), m, p.H.data(),
          p.rm.data(), p.w.data(), p.crep.data(), p.nrep.data(), p.sig.data(), p.navsig.data(), p.kf.data(), p.joint.data());
    SWEEP(scvx_nav_path_sigma_f64_host, B, K, p.x.data(), p.u.data(), p.deriv.data(), p.gain.data(), p.S0.data(), p.N0.data(), m, p.H.data(),
          p.rm.data(), p.w.data(), p.crep.data(), p.nrep.data(), p.psig.data());
    SWEEP(scvx_mc_draws_f64_host, &p.rng, B, S, K, p.xi0.data(), p.eta.data(), p.xin.data(), p.nud.data());
    SWEEP(scvx_track_mc_q_f64_host, B, K, S, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), C0.data(), xi0.data(), eta.data(), p.w.data(),
          nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), fl.data(), xl.data(), d0.data(), nq, ranks.data(), fq.data(), pq.data(),
          pv.data());
    SWEEP(scvx_track_mc_nav_q_f64_host, B, K, S, p.x.data(), p.u.data(), p.sg.data(), p.gain.data(), C0.data(), xi0.data(), eta.data(),
          p.w.data(), p.deriv.data(), p.kf.data(), p.N0.data(), xin.data(), nud.data(), m, p.H.data(), p.rm.data(), 10, 0, 0.0, rep.data(),
          xm.data(), xc.data(), jm.data(), jc.data(), p.nrep.data(), fl.data(), xl.data(), d0.data(), fed.data(), nk.data(), nq, ranks.data(),
          fq.data(), pq.data(), pv.data());
    SWEEP(scvx_order_stats_f64_host, B, S, fl.data(), (size_t)S, (size_t)1, nq, ranks.data(), ov.data());
#undef SWEEP
    return 0;
}

int main() {
    for (int nu : {3, 5})
        for (int m : {0, 6})
            for (int nq : {0, 1, 16})
                for (int dense = 0; dense < 2; dense++)
                    if (run(nu, 3, 4, 70, m, nq, dense != 0, m != 0)) return 1;
    if (run(3, 1, 1, 1, 0, 1, true, false)) return 1;
    for (int nu : {3, 5})
        for (int m : {0, 6})
            for (int opt = 0; opt < 2; opt++)
                if (analyses(nu, 3, 4, 70, m, opt != 0)) return 1;
    if (analyses(3, 1, 1, 1, 0, true)) return 1;
    if (order_stats(1, 1, 1, 1) || order_stats(5, 65, 16, 3) || order_stats(2, 5000, 1, SCVX_Q_MAX)) return 1;
    fflush(stdout);
    if (error_paths()) return 1;
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers on\n");
#endif
#endif
    printf("host staging: %zu allocations, %zu frees, %zu launches\n", g_allocs, g_frees, g_launches);
    return g_allocs == g_frees ? 0 : 1;
}
