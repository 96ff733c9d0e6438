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
// error contract of scvx::Staging.  refusals() and cov_refusals() pin what the sampled calls and the first-order analyses refuse, in which
// words, and which of two faults wins (tests/golden/mc_refusals.txt, cov_refusals.txt).  tests/test_host_staging_sanitizers.py holds the
// build recipe and runs the program.
#include <cmath>
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

// ---- the refusals ----------------------------------------------------------------------------------------------------------------------
// Every argument of the sixteen scvx_track_mc* forms, valid for B = 2, K = 3, S = 2, NU = 3 and m rows, each array of its documented
// size.  refusals() starts every form from this call, makes one argument (or two) bad and prints "refusal <entry> <case> <rc> <message>";
// a refused call allocates nothing.  tests/golden/mc_refusals.txt holds the lines as the six hand-written bodies gave them, before
// check_mc_call replaced their checks: which message a bad call gets, and which fault wins when two are present.
enum { F_NAV = 1, F_Q = 2, F_UP = 4, F_RNG = 8, F_VEH = 16, F_TRUTH = 32, F_M = 64 };
struct McArgs {
    int B = 2, K = 3, S = 2, m, nsub = 10, flags = 0, nq = 1, noise = 0;
    double tol = 0.0;
    V vx, vu, vsg, vgain, vC0, vxi0, veta, vw, vderiv, vkf, vCN, vxin, vnud, vH, vrm, vzeta, vrep, vxm, vxc, vjm, vjc, vnv, vfl, vxl, vd0, vfed,
        vnk, vfq, vpq, vpv, vth;
    std::vector<int> vranks{1};
    const double *x, *u, *sigma, *gain, *C0, *xi0, *eta, *w, *deriv, *kf, *CN, *xin, *nud, *H, *rm, *zeta = nullptr;
    const void* reserved = nullptr;
    double *mcrep, *xmean, *xcov, *jmean, *jcov, *mcnav, *flights, *xland, *dx0, *navfed, *navK, *flightq, *pathq, *pathv, *theta = nullptr;
    const int* ranks;
    scvx_mc_rng rngv{20261020u, 0u, 0u, 0, 0};
    const scvx_mc_rng* rng = nullptr;
    scvx_mc_vehicle vehv{};
    const scvx_mc_vehicle* veh = nullptr;
    scvx_ctx ctx;
    McArgs(int traits, int m_)
        : m(m_), vx(2 * 4 * 14, 1.0), vu(2 * 4 * 3, 1.0), vsg(2, 1.0), vgain(2 * 3 * 3 * 17), vC0(2 * 196), vxi0(2 * 14), veta(2 * 3 * 14),
          vw(14, 1e-3), vderiv(2 * 3 * 14 * 21), vkf(2 * 3 * 14 * (m_ ? m_ : 1)), vCN(2 * 196), vxin(2 * 14), vnud(2 * 3 * (m_ ? m_ : 1)),
          vH((m_ ? m_ : 1) * 14, 0.0), vrm(m_ ? m_ : 1, 1e-6), vzeta(2 * SCVX_VEH_N), vrep(2 * SCVX_MC_NREP), vxm(2 * 14), vxc(2 * 196),
          vjm(2 * 28), vjc(2 * 784), vnv(2 * SCVX_NAV_NREP), vfl(2 * 2 * SCVX_FLIGHT_NREP), vxl(2 * 2 * 14), vd0(2 * 2 * 14),
          vfed(2 * 2 * 3 * 14), vnk(2 * 2 * 14), vfq(2 * 16), vpq(2 * 4 * 5), vpv(2 * 4 * 5 * 2), vth(2 * 2 * SCVX_VEH_N) {
        x = vx.data(), u = vu.data(), sigma = vsg.data(), gain = vgain.data(), C0 = vC0.data(), w = vw.data(), deriv = vderiv.data();
        CN = vCN.data(), kf = m ? vkf.data() : nullptr, H = m ? vH.data() : nullptr, rm = m ? vrm.data() : nullptr;
        const bool up = traits & F_UP;
        xi0 = up ? vxi0.data() : nullptr, eta = up ? veta.data() : nullptr, xin = up ? vxin.data() : nullptr;
        nud = up && m ? vnud.data() : nullptr;
        mcrep = vrep.data(), xmean = vxm.data(), xcov = vxc.data(), jmean = vjm.data(), jcov = vjc.data(), mcnav = vnv.data();
        flights = vfl.data(), xland = vxl.data(), dx0 = vd0.data(), navfed = vfed.data(), navK = vnk.data();
        flightq = vfq.data(), pathq = vpq.data(), pathv = vpv.data(), ranks = vranks.data();
        if (traits & F_RNG) rng = &rngv, noise = 1;
        if (traits & F_VEH) {
            vehv.sp[SCVX_VEH_THRUST] = 1e-3;
            veh = &vehv, theta = vth.data(), zeta = up ? vzeta.data() : nullptr;
        }
        ctx.prob.K = K;
    }
    McArgs(const McArgs&) = delete;
};

struct McForm {
    const char* entry;
    int traits;
    int (*call)(McArgs&);
};
#define MC_A &a.ctx, a.B, a.K, a.S, a.x, a.u, a.sigma, a.gain, a.C0
#define MC_T a.w, a.reserved, a.nsub, a.flags, a.tol, a.mcrep, a.xmean, a.xcov, a.flights, a.xland, a.dx0
#define MC_N1 a.w, a.deriv, a.kf, a.CN
#define MC_N2 \
    a.m, a.H, a.rm, a.nsub, a.flags, a.tol, a.mcrep, a.xmean, a.xcov, a.jmean, a.jcov, a.mcnav, a.flights, a.xland, a.dx0, a.navfed, a.navK
#define MC_Q a.nq, a.ranks, a.flightq, a.pathq, a.pathv
#define MC_V a.rng, a.noise, a.veh, a.zeta, a.theta
#define MC_FORM(name, traits, ...) {#name, traits, [](McArgs& a) { return name(__VA_ARGS__); }}
#define MC_BOTH(name, traits, ...) MC_FORM(name, traits, __VA_ARGS__), MC_FORM(name##_host, traits, __VA_ARGS__)
static const McForm g_forms[] = {
    MC_BOTH(scvx_track_mc_f64, F_TRUTH | F_UP, MC_A, a.xi0, a.eta, MC_T),
    MC_BOTH(scvx_track_mc_q_f64, F_TRUTH | F_UP | F_Q, MC_A, a.xi0, a.eta, MC_T, MC_Q),
    MC_BOTH(scvx_track_mc_rng_f64, F_TRUTH | F_RNG | F_Q, MC_A, a.rng, a.noise, MC_T, MC_Q),
    MC_BOTH(scvx_track_mc_nav_f64, F_NAV | F_UP, MC_A, a.xi0, a.eta, MC_N1, a.xin, a.nud, MC_N2),
    MC_BOTH(scvx_track_mc_nav_q_f64, F_NAV | F_UP | F_Q, MC_A, a.xi0, a.eta, MC_N1, a.xin, a.nud, MC_N2, MC_Q),
    MC_BOTH(scvx_track_mc_nav_rng_f64, F_NAV | F_RNG | F_Q, MC_A, a.rng, a.noise, MC_N1, MC_N2, MC_Q),
    // the _veh forms, on uploaded draws and with rng: tests/host_staging_vehicle_asan.cpp
    MC_BOTH(scvx_track_mc_veh_f64, F_TRUTH | F_UP | F_Q | F_VEH, MC_A, a.xi0, a.eta, MC_T, MC_Q, MC_V),
    MC_BOTH(scvx_track_mc_veh_f64, F_TRUTH | F_RNG | F_Q | F_VEH, MC_A, a.xi0, a.eta, MC_T, MC_Q, MC_V),
    MC_BOTH(scvx_track_mc_nav_veh_f64, F_NAV | F_UP | F_Q | F_VEH, MC_A, a.xi0, a.eta, MC_N1, a.xin, a.nud, MC_N2, MC_Q, MC_V),
    MC_BOTH(scvx_track_mc_nav_veh_f64, F_NAV | F_RNG | F_Q | F_VEH, MC_A, a.xi0, a.eta, MC_N1, a.xin, a.nud, MC_N2, MC_Q, MC_V),
};

// one bad argument: applies to the forms that have every trait of `need` and none of `not_`
struct McFault {
    const char* name;
    int need, not_;
    std::function<void(McArgs&)> make;
};
static const double g_nan = std::nan(""), g_wneg[14] = {1e-3, 1e-3, -1e-3}, g_wnan[14] = {1e-3, g_nan};
static const int g_rank_lo[1] = {-1}, g_rank_hi[1] = {2};
#define BAD(name, need, not_, ...) {name, need, not_, [](McArgs& a) { __VA_ARGS__; }}
static const McFault g_faults[] = {
    BAD("x=NULL", 0, 0, a.x = nullptr), BAD("u=NULL", 0, 0, a.u = nullptr), BAD("sigma=NULL", 0, 0, a.sigma = nullptr),
    BAD("gain=NULL", 0, 0, a.gain = nullptr), BAD("C0=NULL", 0, 0, a.C0 = nullptr), BAD("xi0=NULL", F_UP, 0, a.xi0 = nullptr),
    BAD("mcrep=NULL", 0, 0, a.mcrep = nullptr), BAD("xmean=NULL", 0, 0, a.xmean = nullptr), BAD("xcov=NULL", 0, 0, a.xcov = nullptr),
    BAD("deriv=NULL", F_NAV, 0, a.deriv = nullptr), BAD("CN=NULL", F_NAV, 0, a.CN = nullptr), BAD("xin=NULL", F_NAV | F_UP, 0, a.xin = nullptr),
    BAD("jmean=NULL", F_NAV, 0, a.jmean = nullptr), BAD("jcov=NULL", F_NAV, 0, a.jcov = nullptr), BAD("mcnav=NULL", F_NAV, 0, a.mcnav = nullptr),
    BAD("B=0", 0, 0, a.B = 0), BAD("B=65536", 0, 0, a.B = 65536), BAD("S=0", 0, 0, a.S = 0), BAD("K=4", 0, 0, a.K = 4),
    BAD("nsub=0", 0, 0, a.nsub = 0), BAD("nsub=1001", 0, 0, a.nsub = 1001), BAD("flags=2", 0, 0, a.flags = 2),
    BAD("tol=-1", 0, 0, a.tol = -1.0), BAD("tol=NaN", 0, 0, a.tol = g_nan), BAD("w<0", 0, 0, a.w = g_wneg), BAD("w=NaN", 0, 0, a.w = g_wnan),
    BAD("eta-without-w", 0, 0, a.w = nullptr), BAD("reserved", F_TRUTH, 0, a.reserved = &a),
    BAD("rng=NULL", F_RNG, F_VEH, a.rng = nullptr), BAD("rng.reserved=1", F_RNG, 0, a.rngv.reserved = 1),
    BAD("rng.independent=2", F_RNG, 0, a.rngv.independent = 2),
    BAD("nq=0", F_Q, 0, a.nq = 0), BAD("nq=17", F_Q, 0, a.nq = SCVX_Q_MAX + 1), BAD("ranks=NULL", F_Q, 0, a.ranks = nullptr),
    BAD("rank=-1", F_Q, 0, a.ranks = g_rank_lo), BAD("rank=S", F_Q, 0, a.ranks = g_rank_hi),
    BAD("zeta-without-veh", F_VEH | F_UP, 0, a.veh = nullptr, a.theta = nullptr), BAD("theta-without-veh", F_VEH, 0, a.veh = nullptr, a.zeta = nullptr),
    BAD("veh.reserved=1", F_VEH, 0, a.vehv.reserved[1] = 1), BAD("veh.mu=NaN", F_VEH, 0, a.vehv.mu[SCVX_VEH_ISP] = g_nan),
    BAD("veh.sp<0", F_VEH, 0, a.vehv.sp[SCVX_VEH_ISP] = -1.0), BAD("veh.sp=NaN", F_VEH, 0, a.vehv.sp[SCVX_VEH_ISP] = g_nan),
    BAD("veh.aero", F_VEH, 0, a.vehv.mu[SCVX_VEH_AERO] = 1e-3), BAD("veh.fin", F_VEH, 0, a.vehv.sp[SCVX_VEH_FIN] = 1e-3),
    BAD("veh.sp-without-zeta", F_VEH | F_UP, 0, a.zeta = nullptr),
    BAD("rng+xi0", F_VEH | F_RNG, 0, a.xi0 = a.vxi0.data()), BAD("rng+zeta", F_VEH | F_RNG, 0, a.zeta = a.vzeta.data()),
    BAD("noise-without-rng", F_VEH | F_UP, 0, a.noise = 1),
    BAD("m=-1", F_NAV, 0, a.m = -1), BAD("m=15", F_NAV, 0, a.m = 15), BAD("H=NULL", F_NAV | F_M, 0, a.H = nullptr),
    BAD("rm=NULL", F_NAV | F_M, 0, a.rm = nullptr), BAD("kf=NULL", F_NAV | F_M, 0, a.kf = nullptr),
    BAD("nud=NULL", F_NAV | F_M | F_UP, 0, a.nud = nullptr),
    BAD("aero-without-table", 0, 0, a.ctx.prob.aero_kind = 1),
};
// two faults at once: the first named is of the part every form shares, or of an earlier check than the second
static const char* const g_pairs[][2] = {
    {"B=0", "rng.reserved=1"}, {"x=NULL", "rng=NULL"}, {"B=0", "nq=17"}, {"xcov=NULL", "rank=S"}, {"B=0", "veh.reserved=1"},
    {"x=NULL", "theta-without-veh"}, {"x=NULL", "w<0"}, {"aero-without-table", "w=NaN"}, {"B=0", "m=15"}, {"C0=NULL", "H=NULL"},
    {"tol=NaN", "CN=NULL"}, {"mcrep=NULL", "kf=NULL"}, {"B=0", "noise-without-rng"}, {"S=0", "rng+xi0"}, {"w<0", "reserved"},
    {"rng.reserved=1", "nq=0"}, {"rank=-1", "veh.mu=NaN"}, {"rng.independent=2", "veh.fin"}, {"m=-1", "jcov=NULL"}, {"w=NaN", "m=15"},
    {"CN=NULL", "kf=NULL"}, {"nud=NULL", "nq=17"},
};

static const McFault* fault(const char* name, int traits) {
    for (const McFault& f : g_faults)
        if (!strcmp(f.name, name)) return (traits & f.need) == f.need && !(traits & f.not_) ? &f : nullptr;
    fprintf(stderr, "no fault named %s\n", name);
    abort();
}

static int refuse(const McForm& fm, int traits, int m, const McFault* f1, const McFault* f2) {
    McArgs a(traits, m);
    if (f1) f1->make(a);
    if (f2) f2->make(a);
    const size_t a0 = g_allocs;
    const int rc = fm.call(a);
    printf("refusal %s%s m=%d/%s%s%s %d %s\n", fm.entry, (traits & (F_VEH | F_RNG)) == (F_VEH | F_RNG) ? "+rng" : "", m,
           f1 ? f1->name : "valid", f2 ? "+" : "", f2 ? f2->name : "", rc, a.ctx.err.empty() ? "-" : a.ctx.err.c_str());
    if (f1) REQUIRE(rc != SCVX_OK && g_allocs == a0);
    else REQUIRE(rc == SCVX_OK);
    scvx::mc_workspace_free(&a.ctx);
    return 0;
}

// veh: the _veh forms (their checks live in scvx_mc_veh.hip, which only the vehicle program links) or all the others
static int refusals(bool veh) {
    g_nu = 3;
    for (const McForm& fm : g_forms) {
        if (veh != ((fm.traits & F_VEH) != 0)) continue;
        for (int m : {0, 2}) {
            if (m && !(fm.traits & F_NAV)) continue;
            const int traits = fm.traits | (m ? F_M : 0);
            if (refuse(fm, traits, m, nullptr, nullptr)) return 1;
            for (const McFault& f : g_faults)
                if (fault(f.name, traits) && refuse(fm, traits, m, &f, nullptr)) return 1;
            for (const auto& p : g_pairs) {
                const McFault *f1 = fault(p[0], traits), *f2 = fault(p[1], traits);
                if (f1 && f2 && refuse(fm, traits, m, f1, f2)) return 1;
            }
        }
    }
    if (veh) return 0;
    // scvx_mc_draws_f64[_host]
    V d0(2 * 2 * 14), dk(2 * 2 * 3 * 14);
    struct {
        const char* name;
        int rng, reserved, independent, P, S, K;
    } const draws[] = {{"rng=NULL", 0, 0, 0, 2, 2, 3},     {"rng.reserved=1", 1, 1, 0, 2, 2, 3}, {"rng.independent=2", 1, 0, 2, 2, 2, 3},
                       {"P=0", 1, 0, 0, 0, 2, 3},          {"P=65536", 1, 0, 0, 65536, 2, 3},    {"S=0", 1, 0, 0, 2, 0, 3},
                       {"K=0", 1, 0, 0, 2, 2, 0},          {"rng=NULL+P=0", 0, 0, 0, 0, 2, 3},   {"rng.reserved=1+S=0", 1, 1, 0, 2, 0, 3}};
    for (int host = 0; host < 2; host++)
        for (const auto& c : draws) {
            scvx_ctx ctx;
            const scvx_mc_rng rg{1u, 0u, 0u, c.independent, c.reserved};
            const size_t a0 = g_allocs;
            const int rc = (host ? scvx_mc_draws_f64_host : scvx_mc_draws_f64)(&ctx, c.rng ? &rg : nullptr, c.P, c.S, c.K, d0.data(), dk.data(),
                                                                               d0.data(), dk.data());
            printf("refusal %s %s %d %s\n", host ? "scvx_mc_draws_f64_host" : "scvx_mc_draws_f64", c.name, rc, ctx.err.c_str());
            REQUIRE(rc != SCVX_OK && g_allocs == a0);
        }
    return 0;
}

// ---- the refusals of the first-order analyses ---------------------------------------------------------------------------------------------
// Every argument of the twelve scvx_cov_* / scvx_nav_* forms, valid for B = 2, K = 3, NU = 3 and m rows, each array of its documented
// size.  cov_refusals() starts every form from this call, makes one argument (or two) bad and prints
// "cov-refusal <entry> <case> <rc> <message>"; a refused call allocates nothing.  tests/golden/cov_refusals.txt holds the lines as the
// twelve hand-written bodies gave them: which message a bad call gets, and which fault wins when two are present.
enum { C_NAV = 1, C_PS = 2, C_VEH = 4, C_M = 8 };
struct CovArgs {
    int B = 2, K = 3, m;
    V vx, vu, vderiv, vgain, vS0, vN0, vH, vrm, vw, vvtile, vsp, vrep, vnrep, vpsig, vsig, vcovK, vcov, vnavsig, vkf, vjoint, vsens;
    const double *x, *u, *deriv, *gain, *S0, *N0, *H, *rm, *w, *vtile, *sp6;
    double *report, *navrep, *psig, *sig, *covK, *cov, *navsig, *kf, *joint, *sens;
    scvx_ctx ctx;
    explicit CovArgs(int m_)
        : m(m_), vx(2 * 4 * 14, 1.0), vu(2 * 4 * 3, 1.0), vderiv(2 * 3 * 14 * 21), vgain(2 * 3 * 3 * 17), vS0(2 * 196), vN0(2 * 196),
          vH((m_ ? m_ : 1) * 14, 0.0), vrm(m_ ? m_ : 1, 1e-6), vw(14, 1e-6), vvtile(2 * 3 * SCVX_VTILE_N * 14), vsp(SCVX_VEH_N, 0.0),
          vrep(2 * SCVX_COV_NREP), vnrep(2 * SCVX_NAV_NREP), vpsig(2 * 4 * SCVX_PSIG_N), vsig(2 * 4 * 17), vcovK(2 * 17 * 17),
          vcov(2 * 4 * 17 * 17), vnavsig(2 * 4 * 14), vkf(2 * 3 * 14 * (m_ ? m_ : 1)), vjoint(2 * 4 * 31 * 31), vsens(2 * 4 * 17 * SCVX_VEH_N) {
        vsp[SCVX_VEH_THRUST] = 1e-3;
        x = vx.data(), u = vu.data(), deriv = vderiv.data(), gain = vgain.data(), S0 = vS0.data(), N0 = vN0.data(), w = vw.data();
        H = m ? vH.data() : nullptr, rm = m ? vrm.data() : nullptr, vtile = vvtile.data(), sp6 = vsp.data();
        report = vrep.data(), navrep = vnrep.data(), psig = vpsig.data(), sig = vsig.data(), covK = vcovK.data(), cov = vcov.data();
        navsig = vnavsig.data(), kf = m ? vkf.data() : nullptr, joint = vjoint.data(), sens = vsens.data();
        ctx.prob.K = K;
    }
    CovArgs(const CovArgs&) = delete;
};

struct CovForm {
    const char* entry;
    int traits;
    int (*call)(CovArgs&);
};
#define COV_A &a.ctx, a.B, a.K, a.x, a.u, a.deriv, a.gain, a.S0
#define COV_N a.N0, a.m, a.H, a.rm
#define COV_V a.vtile, a.sp6, a.sens
#define COV_FORM(name, traits, ...) {#name, traits, [](CovArgs& a) { return name(__VA_ARGS__); }}
#define COV_BOTH(name, traits, ...) COV_FORM(name, traits, __VA_ARGS__), COV_FORM(name##_host, traits, __VA_ARGS__)
static const CovForm g_cov_forms[] = {
    COV_BOTH(scvx_cov_propagate_f64, 0, COV_A, a.w, a.report, a.sig, a.covK, a.cov),
    COV_BOTH(scvx_cov_path_sigma_f64, C_PS, COV_A, a.w, a.report, a.psig),
    COV_BOTH(scvx_cov_vehicle_f64, C_VEH, COV_A, a.w, a.report, a.psig, a.sig, a.covK, a.cov, COV_V),
    COV_BOTH(scvx_nav_cov_f64, C_NAV, COV_A, COV_N, a.w, a.report, a.navrep, a.sig, a.navsig, a.kf, a.joint),
    COV_BOTH(scvx_nav_path_sigma_f64, C_NAV | C_PS, COV_A, COV_N, a.w, a.report, a.navrep, a.psig),
    COV_BOTH(scvx_nav_cov_vehicle_f64, C_NAV | C_VEH, COV_A, COV_N, a.w, a.report, a.navrep, a.psig, a.sig, a.navsig, a.kf, a.joint, COV_V),
};

// one bad argument: applies to the forms that have every trait of `need`
struct CovFault {
    const char* name;
    int need;
    void (*make)(CovArgs&);
};
static const double g_cwneg[14] = {1e-6, 1e-6, -1e-6}, g_cwnan[14] = {1e-6, g_nan};
#define CBAD(name, need, ...) {name, need, [](CovArgs& a) { __VA_ARGS__; }}
static const CovFault g_cov_faults[] = {
    CBAD("x=NULL", 0, a.x = nullptr), CBAD("u=NULL", 0, a.u = nullptr), CBAD("deriv=NULL", 0, a.deriv = nullptr),
    CBAD("gain=NULL", 0, a.gain = nullptr), CBAD("S0=NULL", 0, a.S0 = nullptr), CBAD("report=NULL", 0, a.report = nullptr),
    CBAD("N0=NULL", C_NAV, a.N0 = nullptr), CBAD("navrep=NULL", C_NAV, a.navrep = nullptr), CBAD("psig=NULL", C_PS, a.psig = nullptr),
    CBAD("B=0", 0, a.B = 0), CBAD("K=4", 0, a.K = 4), CBAD("w<0", 0, a.w = g_cwneg), CBAD("w=NaN", 0, a.w = g_cwnan),
    CBAD("m=-1", C_NAV, a.m = -1), CBAD("m=15", C_NAV, a.m = 15), CBAD("H=NULL", C_NAV | C_M, a.H = nullptr),
    CBAD("rm=NULL", C_NAV | C_M, a.rm = nullptr), CBAD("rm=0", C_NAV | C_M, a.vrm[1] = 0.0), CBAD("rm=NaN", C_NAV | C_M, a.vrm[0] = g_nan),
    CBAD("H=NaN", C_NAV | C_M, a.vH[15] = g_nan),
    CBAD("sp6=NULL", C_VEH, a.sp6 = nullptr), CBAD("sp<0", C_VEH, a.vsp[SCVX_VEH_MIS_Y] = -1e-3), CBAD("sp=NaN", C_VEH, a.vsp[SCVX_VEH_MIS_Z] = g_nan),
    CBAD("sp.aero", C_VEH, a.vsp[SCVX_VEH_AERO] = 1e-3), CBAD("sp.fin", C_VEH, a.vsp[SCVX_VEH_FIN] = 1e-3),
    CBAD("sp.isp-without-vtile", C_VEH, a.vsp[SCVX_VEH_ISP] = 1e-3, a.vtile = nullptr),
};
// two faults at once, one from each of two groups of checks (shape, null buffers, w, the navigation model, psig, the vehicle) and a few
// within a group; whichever check comes first in a form decides the line
static const char* const g_cov_pairs[][2] = {
    {"B=0", "K=4"},          {"B=0", "x=NULL"},           {"K=4", "w<0"},          {"B=0", "m=15"},        {"K=4", "N0=NULL"},
    {"B=0", "psig=NULL"},    {"K=4", "sp6=NULL"},         {"gain=NULL", "w=NaN"},  {"report=NULL", "H=NULL"}, {"S0=NULL", "N0=NULL"},
    {"u=NULL", "m=-1"},      {"N0=NULL", "m=-1"},         {"navrep=NULL", "rm=0"}, {"S0=NULL", "psig=NULL"}, {"navrep=NULL", "psig=NULL"},
    {"u=NULL", "sp<0"},      {"N0=NULL", "sp.fin"},       {"w<0", "m=15"},         {"w=NaN", "N0=NULL"},   {"w<0", "psig=NULL"},
    {"w=NaN", "sp=NaN"},     {"m=15", "H=NULL"},          {"rm=NULL", "H=NaN"},    {"rm=NaN", "H=NaN"},    {"rm=0", "psig=NULL"},
    {"m=15", "psig=NULL"},   {"H=NaN", "sp.aero"},        {"m=-1", "sp6=NULL"},    {"sp<0", "sp.fin"},     {"sp.aero", "sp.isp-without-vtile"},
};

static const CovFault* cov_fault(const char* name, int traits) {
    for (const CovFault& f : g_cov_faults)
        if (!strcmp(f.name, name)) return (traits & f.need) == f.need ? &f : nullptr;
    fprintf(stderr, "no fault named %s\n", name);
    abort();
}

static int cov_refuse(const CovForm& fm, int m, const CovFault* f1, const CovFault* f2) {
    CovArgs a(m);
    if (f1) f1->make(a);
    if (f2) f2->make(a);
    const size_t a0 = g_allocs, f0 = g_frees;
    const int rc = fm.call(a);
    printf("cov-refusal %s m=%d/%s%s%s %d %s\n", fm.entry, m, f1 ? f1->name : "valid", f2 ? "+" : "", f2 ? f2->name : "", rc,
           a.ctx.err.empty() ? "-" : a.ctx.err.c_str());
    if (f1) REQUIRE(rc != SCVX_OK && g_allocs == a0);
    else REQUIRE(rc == SCVX_OK && g_allocs - a0 == g_frees - f0);
    return 0;
}

// veh: the _vehicle forms (tests/host_staging_cov_vehicle_asan.cpp runs them) or all the others
static int cov_refusals(bool veh) {
    g_nu = 3;
    for (const CovForm& fm : g_cov_forms) {
        if (veh != ((fm.traits & C_VEH) != 0)) continue;
        for (int m : {0, 2}) {
            if (m && !(fm.traits & C_NAV)) continue;
            const int traits = fm.traits | (m ? C_M : 0);
            if (cov_refuse(fm, m, nullptr, nullptr)) return 1;
            for (const CovFault& f : g_cov_faults)
                if (cov_fault(f.name, traits) && cov_refuse(fm, m, &f, nullptr)) return 1;
            for (const auto& p : g_cov_pairs) {
                const CovFault *f1 = cov_fault(p[0], traits), *f2 = cov_fault(p[1], traits);
                if (f1 && f2 && cov_refuse(fm, m, f1, f2)) return 1;
            }
        }
    }
    return 0;
}

int main() {
    if (refusals(false) || cov_refusals(false)) return 1;
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
