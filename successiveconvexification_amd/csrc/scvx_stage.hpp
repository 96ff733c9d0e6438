// The device staging of a one-shot call (the _host forms and the batch-level analyses): the one way to write "allocate temporaries, copy
// the inputs up, launch, copy the wanted outputs down, synchronise, free".  Not part of the ABI.
//
//     Staging s(ctx);
//     const double* dx = s.in(x, d.x);        // nullptr in, nullptr out: an optional array costs nothing
//     double* dr = s.out(report, d.frep);
//     s.launch([&] { return launch_flight(ctx, ..., dx, ..., dr, s.st); });
//     return s.finish("scvx_flight_check_f64_host");
//
// Declare every buffer before the first launch: the uploads are enqueued in front of it, behind all the allocations, the order the
// hand-written sequences had (profiles/host_staging.md).  The first HIP error sticks: nothing more is allocated, copied or launched
// after it.  finish() ALWAYS synchronises the stream before the buffers are freed, on the error path too, so nothing that was enqueued
// can still touch them or the caller's arrays when the call returns.
#pragma once
#include <string>
#include <vector>
#include "scvx_internal.hpp"

namespace scvx {

class Staging {
    struct Buf {
        void* dev;
        const void* src;   // what launch() uploads first, or nullptr
        void* dst;         // where finish() downloads it to, or nullptr
        size_t bytes;
    };
    scvx_ctx* ctx_;
    hipError_t e_;
    std::vector<Buf> bufs_;
    size_t uploaded_ = 0;   // the buffers before this one have had their upload enqueued

    void* alloc(size_t bytes, const void* src, void* dst) {
        void* p = nullptr;
        if (e_ != hipSuccess || (e_ = hipMalloc(&p, bytes)) != hipSuccess) return nullptr;
        bufs_.push_back({p, src, dst, bytes});
        return p;
    }
    void release() {
        for (const Buf& b : bufs_) (void)hipFree(b.dev);
        bufs_.clear();
    }

public:
    const hipStream_t st;

    explicit Staging(scvx_ctx* ctx) : ctx_(ctx), e_(hipSetDevice(ctx->device)), st(ctx->stream) {}
    Staging(const Staging&) = delete;
    ~Staging() { release(); }

    // a device-only buffer of n elements
    template <typename T = double>
    T* tmp(size_t n) {
        return (T*)alloc(n * sizeof(T), nullptr, nullptr);
    }
    // host[n], uploaded in front of the next launch
    template <typename T>
    T* in(const T* host, size_t n) {
        return host ? (T*)alloc(n * sizeof(T), host, nullptr) : nullptr;
    }
    // n elements that finish() downloads to host; out_always: allocated, for a kernel that writes them anyway, also without a host
    template <typename T>
    T* out(T* host, size_t n) {
        return host ? out_always(host, n) : nullptr;
    }
    template <typename T>
    T* out_always(T* host, size_t n) {
        return (T*)alloc(n * sizeof(T), nullptr, host);
    }
    // the uploads declared so far, then f(), which enqueues on st and returns a hipError_t; nothing of it after a failure
    template <typename F>
    void launch(F&& f) {
        for (; uploaded_ < bufs_.size() && e_ == hipSuccess; uploaded_++)
            if (const Buf& b = bufs_[uploaded_]; b.src) e_ = hipMemcpyAsync(b.dev, b.src, b.bytes, hipMemcpyHostToDevice, st);
        if (e_ == hipSuccess) e_ = f();
    }
    // the downloads in the order of their out() calls, the synchronise, the frees; entry: the exported name, for the message
    int finish(const char* entry) {
        for (size_t i = 0; i < bufs_.size() && e_ == hipSuccess; i++)
            if (const Buf& b = bufs_[i]; b.dst) e_ = hipMemcpyAsync(b.dst, b.dev, b.bytes, hipMemcpyDeviceToHost, st);
        const hipError_t es = hipStreamSynchronize(st);
        if (e_ == hipSuccess) e_ = es;
        release();
        return e_ == hipSuccess ? (int)SCVX_OK : fail(ctx_, SCVX_ERR_HIP, std::string(entry) + ": " + hipGetErrorString(e_));
    }
};

// element counts of the arrays of include/scvx.h for a call's shape; S, m, nq: 0 where the call has none
struct Dims {
    size_t x, u, b, seg, deriv, gain, p0, c14, b14, frep, crep, nrep, mcrep, sig, covK, cov, psig, navsig, kf, joint;   // per plan
    size_t xi, eta, nud, flights, s14, fed, jmean, jcov, flightq, pathq, pathv, zeta, theta;                           // sampled
    size_t vtile, sens;                                                                                                // vehicle errors
    size_t srep, satk;                                                                                                 // clamp-aware covariance
    size_t aud;                                                                                                        // segment audit
    Dims(int B_, int K_, int NU, int S_ = 0, int m_ = 0, int nq_ = 0) {
        const size_t B = (size_t)B_, K = (size_t)K_, S = (size_t)S_, m = (size_t)m_, nq = (size_t)nq_, n = 14 + (size_t)NU, N = n + 14;
        x = B * (K + 1) * 14, u = B * (K + 1) * NU, b = B, seg = B * K * 14, deriv = B * K * 14 * (14 + 2 * NU + 1);
        gain = B * K * NU * n, p0 = covK = B * n * n, c14 = B * 196, b14 = B * 14;
        frep = B * SCVX_FLIGHT_NREP, crep = B * SCVX_COV_NREP, nrep = B * SCVX_NAV_NREP, mcrep = B * SCVX_MC_NREP;
        sig = B * (K + 1) * n, cov = B * (K + 1) * n * n, psig = B * (K + 1) * SCVX_PSIG_N, navsig = B * (K + 1) * 14;
        kf = B * K * 14 * m, joint = B * (K + 1) * N * N;
        xi = S * 14, eta = S * K * 14, nud = S * K * m, flights = B * S * SCVX_FLIGHT_NREP, s14 = B * S * 14, fed = B * S * K * 14;
        jmean = B * 28, jcov = B * 784, flightq = B * SCVX_FLIGHT_NREP * nq, pathq = psig * nq, pathv = psig * S;
        zeta = S * SCVX_VEH_N, theta = B * S * SCVX_VEH_N;
        vtile = B * K * SCVX_VTILE_N * 14, sens = B * (K + 1) * n * SCVX_VEH_N;
        srep = B * SCVX_SAT_NREP, satk = B * K * 4;
        aud = B * K * SCVX_SEG_N;
    }
};

}  // namespace scvx
