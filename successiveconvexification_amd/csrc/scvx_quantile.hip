// Exact batched order statistics (scvx_order_stats_f64, include/scvx.h): out[r][i] = the element of rank ranks[i] of row r in ascending
// order, -inf < .. < -0 <= +0 < .. < +inf < every NaN.  A SELECTION: the output is one of the inputs bit for bit (a NaN comes back as
// the quiet NaN 0x7ff..f).  No counterpart in the reference.
//
// order_stats_kernel: ONE WORKGROUP PER ROW over monotone 64-bit keys.  A double maps to a key by flipping all bits of a negative, the
// sign bit of a non-negative, and sending every NaN to the top key; unsigned order of the keys is then the order above.
//   * S > QSMALL = 256: a most-significant-digit radix select, 256 lanes.  Eight passes of eight bits, most significant first: every
//     pass histograms (integer LDS atomics: the counts do not depend on the order of arrival, so two launches agree bitwise) the digit
//     of the keys that still share the prefix found so far, for all nq ranks at once -- a key is read once per pass; ranks whose prefixes
//     still coincide (all of them in the first passes) share ONE histogram, so the leading digits, where a flight's values crowd into a
//     few bins, cost one contended atomic per key and not nq --, then one wavefront per rank scans the 256 counts (four per lane, a
//     shuffle prefix sum) for the digit that holds the rank.  After the eighth pass the prefix IS the key.  The passes run over the
//     row's keys in LDS when the row fits QLDS = 4,096 keys (32 KB; with the 16 KB of histograms at nq = 16 inside the 64 KB a workgroup
//     gets without opting into more), else over the row in global memory, converted on the fly -- the row is then read eight times.
//     This path serves every S >= 1.
//   * S <= QSMALL: the rank of every key by counting, 64 lanes -- rank_i = #{j : key_j < key_i, or key_j = key_i and j < i}, the keys
//     read from LDS at one address per step (a broadcast); the ranks are a permutation of 0 .. S - 1, so exactly one lane owns each
//     wanted rank and writes it.  S (S / 64) steps per lane and one barrier, against eight passes of three barriers: the rows of the
//     sampled dispersion at S = 64 (tens of thousands of them) are what this second path is kept for; profiles/mc_quantiles.md has the
//     measurement of both paths on those rows.
// The LDS is dynamic, sized by min(S, QLDS) and nq, so that the small rows do not reserve what an 8,192-row needs.
#include "scvx_mc.hpp"
#include "scvx_stage.hpp"

namespace scvx {

constexpr int QLDS = 4096, QSMALL = 256;

struct QRanks { int r[SCVX_Q_MAX]; };

__device__ __forceinline__ unsigned long long q_key(double v) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(v);
    if ((u & 0x7fffffffffffffffull) > 0x7ff0000000000000ull) return ~0ull;   // every NaN, either sign
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ double q_value(unsigned long long k) {
    const unsigned long long u = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;   // the top key gives 0x7ff..f, a quiet NaN
    return __longlong_as_double((long long)u);
}

// rows: row r starts at v[(r / inner) * ld_outer + (r % inner) * ld_inner], its S values inc apart
__global__ __launch_bounds__(256) void order_stats_kernel(int S, const double* __restrict__ v, size_t ld_outer, int inner, size_t ld_inner,
                                                          size_t inc, int nq, QRanks rk, double* __restrict__ out) {
    extern __shared__ unsigned long long q_lds[];
    const int r = blockIdx.x, t = threadIdx.x, nt = blockDim.x;
    const bool staged = S <= QLDS, counting = S <= QSMALL;
    unsigned long long* keys = q_lds;                                             // [staged ? S : 0]
    unsigned* hist = reinterpret_cast<unsigned*>(q_lds + (staged ? S : 0));       // [nq][256]
    __shared__ unsigned long long prefix[SCVX_Q_MAX];
    __shared__ unsigned rem[SCVX_Q_MAX];
    __shared__ int owner[SCVX_Q_MAX];   // the first rank with the same prefix: its histogram serves both
    const double* row = v + (size_t)(r / inner) * ld_outer + (size_t)(r % inner) * ld_inner;
    if (staged)
        for (int i = t; i < S; i += nt) keys[i] = q_key(row[(size_t)i * inc]);
    if (t < nq) {
        prefix[t] = 0ull;
        rem[t] = (unsigned)rk.r[t];
        owner[t] = 0;
    }
    if (counting) {
        __syncthreads();
        for (int i = t; i < S; i += nt) {
            const unsigned long long k = keys[i];
            unsigned rnk = 0;
            for (int j = 0; j < S; j++) {
                const unsigned long long kj = keys[j];
                rnk += (kj < k || (kj == k && j < i)) ? 1u : 0u;
            }
            for (int q = 0; q < nq; q++)
                if (rnk == rem[q]) out[(size_t)r * nq + q] = q_value(k);
        }
        return;
    }
    for (int pass = 7; pass >= 0; pass--) {
        const int shift = pass * 8;
        const unsigned long long himask = pass == 7 ? 0ull : (~0ull << (shift + 8));   // the digits already fixed
        for (int i = t; i < nq * 256; i += nt) hist[i] = 0u;
        __syncthreads();   // the histograms are clear, and prefix / rem of the previous pass (or the start) are written
        for (int i = t; i < S; i += nt) {
            const unsigned long long k = staged ? keys[i] : q_key(row[(size_t)i * inc]);
            const unsigned d = (unsigned)(k >> shift) & 255u;
            for (int q = 0; q < nq; q++)
                if (owner[q] == q && ((k ^ prefix[q]) & himask) == 0ull) atomicAdd(&hist[q * 256 + d], 1u);
        }
        __syncthreads();
        // one wavefront per rank: lane l holds the counts of digits 4 l .. 4 l + 3
        const int lane = t & 63;
        for (int q = t >> 6; q < nq; q += nt >> 6) {
            const unsigned* h = hist + owner[q] * 256 + lane * 4;
            const unsigned c0 = h[0], c1 = h[1], c2 = h[2], c3 = h[3];
            const unsigned sum = c0 + c1 + c2 + c3;
            unsigned incl = sum;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const unsigned up = __shfl_up(incl, o);
                if (lane >= o) incl += up;
            }
            const unsigned excl = incl - sum, want = rem[q];
            if (want >= excl && want < incl) {   // exactly one lane: the counts of the keys sharing the prefix sum to more than rem
                unsigned d = 0, a = excl;
                if (want >= a + c0) { a += c0; d = 1;
                    if (want >= a + c1) { a += c1; d = 2;
                        if (want >= a + c2) { a += c2; d = 3; } } }
                prefix[q] |= (unsigned long long)(lane * 4 + d) << shift;
                rem[q] = want - a;
            }
        }
        __syncthreads();   // every wavefront has read the histograms before the next pass clears them, and the prefixes are final
        if (t < nq) {
            int o = t;
            for (int q = t - 1; q >= 0; q--)
                if (prefix[q] == prefix[t]) o = q;
            owner[t] = o;   // read behind the barrier that follows the next pass's clearing
        }
    }
    if (t < nq) out[(size_t)r * nq + t] = q_value(prefix[t]);
}

hipError_t launch_order_stats(int R, int S, const double* v, size_t ld_outer, int inner, size_t ld_inner, size_t inc, int nq,
                              const int* ranks, double* out, hipStream_t st) {
    QRanks rk{};
    for (int i = 0; i < nq; i++) rk.r[i] = ranks[i];
    const size_t lds = (size_t)(S <= QLDS ? S : 0) * 8 + (S <= QSMALL ? 0 : (size_t)nq * 256 * 4);   // the counting path has no histogram
    hipLaunchKernelGGL(order_stats_kernel, dim3((unsigned)R), dim3(S <= QSMALL ? 64 : 256), lds, st, S, v, ld_outer, inner, ld_inner, inc,
                       nq, rk, out);
    return hipGetLastError();
}

int check_ranks(scvx_ctx* ctx, int S, int nq, const int* ranks) {
    if (nq < 1 || nq > SCVX_Q_MAX) return fail(ctx, SCVX_ERR_ARG, "order stats: 1 <= nq <= SCVX_Q_MAX required");
    if (!ranks) return fail(ctx, SCVX_ERR_ARG, "order stats: null ranks");
    for (int i = 0; i < nq; i++)
        if (ranks[i] < 0 || ranks[i] >= S) return fail(ctx, SCVX_ERR_ARG, "order stats: 0 <= rank < S required");
    return SCVX_OK;
}

static int check_order_stats(scvx_ctx* ctx, int R, int S, const void* v, size_t ld, size_t inc, int nq, const int* ranks, const void* out) {
    if (!ctx) return SCVX_ERR_ARG;
    if (R < 1 || S < 1) return fail(ctx, SCVX_ERR_ARG, "order stats: R >= 1 and S >= 1 required");
    int rc = check_ranks(ctx, S, nq, ranks);
    if (rc) return rc;
    if (inc < 1) return fail(ctx, SCVX_ERR_ARG, "order stats: inc >= 1 required");
    if (R > 1 && ld < (size_t)(S - 1) * inc + 1) return fail(ctx, SCVX_ERR_ARG, "order stats: ld must be at least (S - 1) inc + 1");
    if (!v || !out) return fail(ctx, SCVX_ERR_ARG, "order stats: null buffer");
    return SCVX_OK;
}

}  // namespace scvx

extern "C" {

int scvx_order_stats_f64(scvx_ctx* ctx, int R, int S, const double* v_dev, size_t ld, size_t inc, int nq, const int* ranks,
                         double* out_dev) {
    int rc = scvx::check_order_stats(ctx, R, S, v_dev, ld, inc, nq, ranks, out_dev);
    if (rc) return rc;
    SCVX_HIP(ctx, hipSetDevice(ctx->device));
    SCVX_HIP(ctx, scvx::launch_order_stats(R, S, v_dev, ld, 1, 0, inc, nq, ranks, out_dev, ctx->stream));
    return SCVX_OK;
}

int scvx_order_stats_f64_host(scvx_ctx* ctx, int R, int S, const double* v, size_t ld, size_t inc, int nq, const int* ranks, double* out) {
    int rc = scvx::check_order_stats(ctx, R, S, v, ld, inc, nq, ranks, out);
    if (rc) return rc;
    scvx::Staging s(ctx);
    const double* dv = s.in(v, (size_t)(R - 1) * ld + (size_t)(S - 1) * inc + 1);   // the last row need not be padded
    double* dout = s.out(out, (size_t)R * nq);
    s.launch([&] { return scvx::launch_order_stats(R, S, dv, ld, 1, 0, inc, nq, ranks, dout, s.st); });
    return s.finish("scvx_order_stats_f64_host");
}

}  // extern "C"
