// Stand-alone sanitizer program for the HOST-side staging of scvx_segment_audit_f64_host, on the pattern of tests/host_staging_asan.cpp.
//
// Built WITHOUT a GPU runtime: csrc/scvx_audit.hip is compiled for the host only (hipcc --cuda-host-only), every sanitizer option passed
// to the host compilation alone (-Xarch_host), and linked against the small HIP runtime below, in which "device" memory is host memory
// from malloc, sized exactly as the call asked, a copy is a memcpy and a kernel launch does nothing.  Every array this program hands in
// has exactly the size include/scvx.h documents, so a staging buffer that is too small, a copy that is too long on either side, a leak
// or a use after free is an AddressSanitizer report.  No kernel runs and nothing about the outputs is checked.  The runtime counts what a
// call allocates, copies, launches and synchronises ("traffic" lines), and makes every allocation, copy and launch of one call fail in
// turn: the call then answers SCVX_ERR_HIP with the entry point's name, has synchronised, and has freed what it allocated.
// tests/test_segment_audit_sanitizers.py holds the build recipe and runs the program.  Nothing here is loaded into python.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "scvx_internal.hpp"

struct Traffic {
    size_t allocs, alloc_bytes, frees, h2d, h2d_bytes, d2h, d2h_bytes, launches, syncs;
};
static Traffic g_t{};
static std::string g_log;      // one letter per runtime call since the last reset: Alloc, Free, Copy, Launch, Sync
static char g_fail_kind = 0;   // 'A', 'C' or 'L': that kind's g_fail_at-th call since the last reset fails; 0: nothing fails
static size_t g_fail_at = 0;
static hipError_t g_last = hipSuccess;

static void reset_traffic() {
    g_t = Traffic{};
    g_log.clear();
    g_last = hipSuccess;
}
static size_t count(char kind) {
    size_t n = 0;
    for (char c : g_log) n += c == kind;
    return n;
}
static bool event(char kind) {
    g_log.push_back(kind);
    return kind == g_fail_kind && count(kind) == g_fail_at;
}

extern "C" {
hipError_t hipMalloc(void** p, size_t n) {
    *p = nullptr;
    if (event('A')) return hipErrorOutOfMemory;
    *p = calloc(n ? n : 1, 1);
    g_t.allocs++, g_t.alloc_bytes += n;
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void* p) {
    event('F');
    free(p);
    g_t.frees++;
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind kind, hipStream_t) {
    if (event('C')) return hipErrorInvalidValue;
    memcpy(d, s, n);
    if (kind == hipMemcpyHostToDevice) g_t.h2d++, g_t.h2d_bytes += n;
    else g_t.d2h++, g_t.d2h_bytes += n;
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
    g_t.launches++;
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

// ---- what the translation unit takes from the rest of the library ----
static int g_nu = 3;
extern "C" int scvx_control_dim(const scvx_ctx*) { return g_nu; }
namespace scvx {
PathK path_constants(const scvx_problem&) { return PathK{}; }
}

static int g_bad = 0;
#define REQUIRE(c)                                                    \
    do {                                                              \
        if (!(c)) {                                                   \
            printf("FAILED line %d: %s\n", __LINE__, #c);             \
            g_bad++;                                                  \
        }                                                             \
    } while (0)

// one call on arrays of exactly the documented sizes; with_report: the optional output
static int audit(scvx_ctx* ctx, int B, int K, int nsub, bool with_report) {
    const size_t nu = (size_t)g_nu;
    std::vector<double> x((size_t)B * (K + 1) * 14, 0.5), u((size_t)B * (K + 1) * nu, 0.25), sigma((size_t)B, 1.0);
    std::vector<double> seg((size_t)B * K * SCVX_SEG_N), report((size_t)B * SCVX_FLIGHT_NREP);
    return scvx_segment_audit_f64_host(ctx, B, K, x.data(), u.data(), sigma.data(), nsub, seg.data(), with_report ? report.data() : nullptr);
}

int main() {
#if defined(__has_feature)
#if __has_feature(address_sanitizer)
    printf("sanitizers on\n");
#endif
#endif
    const int shapes[][2] = {{1, 1}, {3, 7}, {65, 3}, {2, 50}};
    for (int nu : {3, 5}) {
        g_nu = nu;
        for (auto& s : shapes) {
            const int B = s[0], K = s[1];
            scvx_ctx ctx;
            ctx.prob.K = K;
            ctx.dyn.fin = nu == 5;
            for (int rep = 1; rep >= 0; rep--) {
                reset_traffic();
                const int rc = audit(&ctx, B, K, rep ? 0 : 40, rep != 0);   // nsub = 0: the context's
                REQUIRE(rc == SCVX_OK);
                REQUIRE(g_t.allocs == g_t.frees && g_t.syncs == 1 && g_t.h2d == 3);
                REQUIRE(g_t.launches == (rep ? 2u : 1u) && g_t.d2h == (rep ? 2u : 1u));
                REQUIRE(g_t.d2h_bytes == 8 * ((size_t)B * K * SCVX_SEG_N + (rep ? (size_t)B * SCVX_FLIGHT_NREP : 0)));
                REQUIRE(g_t.h2d_bytes == 8 * ((size_t)B * (K + 1) * (14 + nu) + B));
                printf("traffic NU %d B %d K %d report %d: allocs %zu (%zu B) frees %zu h2d %zu (%zu B) d2h %zu (%zu B) launches %zu syncs %zu\n", nu, B,
                       K, rep, g_t.allocs, g_t.alloc_bytes, g_t.frees, g_t.h2d, g_t.h2d_bytes, g_t.d2h, g_t.d2h_bytes, g_t.launches, g_t.syncs);
            }
            // every allocation, copy and launch of the call with the report fails in turn
            for (char kind : {'A', 'C', 'L'}) {
                reset_traffic();
                REQUIRE(audit(&ctx, B, K, 10, true) == SCVX_OK);
                const size_t n = count(kind);
                REQUIRE(n == (kind == 'A' ? 5u : kind == 'C' ? 5u : 2u));
                for (size_t at = 1; at <= n; at++) {
                    reset_traffic();
                    g_fail_kind = kind, g_fail_at = at;
                    const int rc = audit(&ctx, B, K, 10, true);
                    g_fail_kind = 0;
                    REQUIRE(rc == SCVX_ERR_HIP);
                    REQUIRE(ctx.err.find("scvx_segment_audit_f64_host") == 0);
                    REQUIRE(g_t.allocs == g_t.frees && g_t.syncs == 1);
                    REQUIRE(g_log.rfind('S') > g_log.rfind('C') || g_log.rfind('C') == std::string::npos);   // synchronised after the last copy
                    REQUIRE(g_log.find('F') == std::string::npos || g_log.find('F') > g_log.rfind('S'));     // and before the first free
                }
            }
            // refusals come before anything is allocated
            reset_traffic();
            REQUIRE(audit(&ctx, B, K, -1, true) == SCVX_ERR_ARG && ctx.err.find("nsub") != std::string::npos);
            REQUIRE(audit(&ctx, B, K, 1001, true) == SCVX_ERR_ARG);
            REQUIRE(audit(&ctx, 0, K, 10, true) == SCVX_ERR_ARG && ctx.err.find("B >= 1") != std::string::npos);
            REQUIRE(audit(&ctx, B, K + 1, 10, true) == SCVX_ERR_ARG && ctx.err.find("K must equal") != std::string::npos);
            std::vector<double> a(64);
            REQUIRE(scvx_segment_audit_f64_host(&ctx, B, K, a.data(), a.data(), a.data(), 10, nullptr, a.data()) == SCVX_ERR_ARG);
            REQUIRE(scvx_segment_audit_f64_host(&ctx, B, K, nullptr, a.data(), a.data(), 10, a.data(), nullptr) == SCVX_ERR_ARG);
            REQUIRE(scvx_segment_audit_f64_host(nullptr, B, K, a.data(), a.data(), a.data(), 10, a.data(), nullptr) == SCVX_ERR_ARG);
            REQUIRE(g_log.empty());
        }
    }
    printf("segment audit staging: %s\n", g_bad ? "FAILED" : "clean");
    return g_bad ? 1 : 0;
}
