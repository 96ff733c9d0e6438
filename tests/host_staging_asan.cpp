// Stand-alone sanitizer program for the HOST-side staging of the _host forms of the sampled calls and of the order statistics
// (scvx_track_mc_q_f64_host, scvx_track_mc_nav_q_f64_host, scvx_order_stats_f64_host and, through them, the old _host forms).
//
// Built WITHOUT a GPU runtime: the three translation units are compiled for the host only (hipcc --cuda-host-only), every sanitizer
// option passed to the host compilation alone (-Xarch_host), and linked against the small HIP runtime below, in which "device" memory is
// host memory from malloc, sized exactly as the call asked, a copy is a memcpy and a kernel launch does nothing.  Every array this
// program hands in is allocated with exactly the size include/scvx.h documents, so a staging buffer that is too small, a copy that is
// too long on either side, a leak or a use after free in the staging code is an AddressSanitizer report.  No kernel runs: the outputs
// are whatever the "device" buffers held (zeroed here), and nothing about them is checked.  tests/test_host_staging_sanitizers.py holds
// the build recipe and runs the program.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "scvx_mc.hpp"

// ---- the HIP runtime of this program -------------------------------------------------------------------------------------------------
static size_t g_allocs = 0, g_frees = 0, g_launches = 0;
extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    *p = calloc(n ? n : 1, 1);
    g_allocs++;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    free(p);
    g_frees++;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind, hipStream_t) {
    memcpy(d, s, n);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t) {
    memset(d, v, n);
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipSetDevice(int) { return hipSuccess; }
hipError_t hipGetLastError(void) { return hipSuccess; }
const char* hipGetErrorString(hipError_t) { return "shim"; }
hipError_t hipLaunchKernel(const void*, dim3, dim3, void**, size_t, hipStream_t) {
    g_launches++;
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

// ---- what the three translation units take from the rest of the library ---------------------------------------------------------------
static int g_nu = 3;
extern "C" int scvx_control_dim(const scvx_ctx*) { return g_nu; }
namespace scvx {
PathK path_constants(const scvx_problem&) { return PathK{}; }
int check_nav_model(scvx_ctx* ctx, int m, const double* H, const double* rm) {
    if (m < 0 || m > 14 || (m > 0 && (!H || !rm))) return fail(ctx, SCVX_ERR_ARG, "nav model");
    return SCVX_OK;
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

static int run(int nu, int B, int K, int S, int m, int nq, bool dense, bool noise) {
    g_nu = nu;
    scvx_ctx ctx;
    ctx.prob.K = K;
    const int n = 14 + nu;
    V x((size_t)B * (K + 1) * 14, 1.0), u((size_t)B * (K + 1) * nu, 1.0), sg(B, 1.0), gain((size_t)B * K * nu * n), C0((size_t)B * 196),
        xi0((size_t)S * 14), eta((size_t)S * K * 14), sw(14, 1e-3), rep((size_t)B * SCVX_MC_NREP), xm((size_t)B * 14), xc((size_t)B * 196),
        fl((size_t)B * S * SCVX_FLIGHT_NREP), xl((size_t)B * S * 14), d0((size_t)B * S * 14), fq((size_t)B * 16 * nq),
        pq((size_t)B * (K + 1) * 5 * nq), pv((size_t)B * (K + 1) * 5 * S);
    std::vector<int> ranks(nq);
    for (int i = 0; i < nq; i++) ranks[i] = (i * 7) % S;
    double* const none = nullptr;
    // truth-fed
    int rc = scvx_track_mc_q_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(),
                                      noise ? eta.data() : none, noise ? sw.data() : none, nullptr, 10, 0, 0.0, rep.data(), xm.data(),
                                      xc.data(), dense ? fl.data() : none, dense ? xl.data() : none, dense ? d0.data() : none, nq,
                                      nq ? ranks.data() : nullptr, nq ? fq.data() : none, nq ? pq.data() : none, dense ? pv.data() : none);
    REQUIRE(rc == SCVX_OK);
    rc = scvx_track_mc_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), noise ? eta.data() : none,
                                noise ? sw.data() : none, nullptr, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), dense ? fl.data() : none,
                                none, none);
    REQUIRE(rc == SCVX_OK);
    // flown on an estimate
    V deriv((size_t)B * K * 14 * (14 + 2 * nu + 1)), kf((size_t)B * K * 14 * (m ? m : 1)), CN((size_t)B * 196), xin((size_t)S * 14),
        nud((size_t)S * K * (m ? m : 1)), H((size_t)(m ? m : 1) * 14, 0.0), rm(m ? m : 1, 1e-6), jm((size_t)B * 28), jc((size_t)B * 784),
        nv((size_t)B * SCVX_NAV_NREP), fed((size_t)B * S * K * 14), nk((size_t)B * S * 14);
    rc = scvx_track_mc_nav_q_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(),
                                      noise ? eta.data() : none, noise ? sw.data() : none, deriv.data(), m ? kf.data() : none, CN.data(),
                                      xin.data(), m ? nud.data() : none, m, m ? H.data() : none, m ? rm.data() : none, 10, 0, 0.0, rep.data(),
                                      xm.data(), xc.data(), jm.data(), jc.data(), nv.data(), dense ? fl.data() : none, dense ? xl.data() : none,
                                      dense ? d0.data() : none, dense ? fed.data() : none, dense ? nk.data() : none, nq,
                                      nq ? ranks.data() : nullptr, nq ? fq.data() : none, nq ? pq.data() : none, dense ? pv.data() : none);
    REQUIRE(rc == SCVX_OK);
    rc = scvx_track_mc_nav_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), none, none, deriv.data(),
                                    m ? kf.data() : none, CN.data(), xin.data(), m ? nud.data() : none, m, m ? H.data() : none,
                                    m ? rm.data() : none, 10, 0, 0.0, rep.data(), xm.data(), xc.data(), jm.data(), jc.data(), nv.data(), none,
                                    none, none, none, none);
    REQUIRE(rc == SCVX_OK);
    // a refusal after the old checks and before any staging: nothing is allocated
    if (nq) {
        const size_t a0 = g_allocs;
        ranks[0] = S;
        rc = scvx_track_mc_q_f64_host(&ctx, B, K, S, x.data(), u.data(), sg.data(), gain.data(), C0.data(), xi0.data(), none, none, nullptr, 10,
                                      0, 0.0, rep.data(), xm.data(), xc.data(), none, none, none, nq, ranks.data(), fq.data(), none, none);
        REQUIRE(rc == SCVX_ERR_ARG && g_allocs == a0);
    }
    scvx::mc_workspace_free(&ctx);
    return 0;
}

static int order_stats(int R, int S, size_t inc, int nq) {
    scvx_ctx ctx;
    const size_t ld = (size_t)(S - 1) * inc + 3;
    V v((size_t)(R - 1) * ld + (size_t)(S - 1) * inc + 1, 0.5), out((size_t)R * nq);   // the last row is NOT padded
    std::vector<int> ranks(nq, S - 1);
    REQUIRE(scvx_order_stats_f64_host(&ctx, R, S, v.data(), ld, inc, nq, ranks.data(), out.data()) == SCVX_OK);
    REQUIRE(scvx_order_stats_f64_host(&ctx, R, S, v.data(), ld, inc, SCVX_Q_MAX + 1, ranks.data(), out.data()) == SCVX_ERR_ARG);
    return 0;
}

int main() {
    for (int nu : {3, 5})
        for (int m : {0, 6})
            for (int nq : {0, 1, 16})
                for (int dense = 0; dense < 2; dense++)
                    if (run(nu, 3, 4, 70, m, nq, dense != 0, m != 0)) return 1;
    if (run(3, 1, 1, 1, 0, 1, true, false)) return 1;
    if (order_stats(1, 1, 1, 1) || order_stats(5, 65, 16, 3) || order_stats(2, 5000, 1, SCVX_Q_MAX)) return 1;
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers on\n");
#endif
#endif
    printf("host staging: %zu allocations, %zu frees, %zu launches\n", g_allocs, g_frees, g_launches);
    return g_allocs == g_frees ? 0 : 1;
}
