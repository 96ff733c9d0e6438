// The executor primitives of the conic kernel (K4) in isolation, against long-double arithmetic on the host: when the path test
// (tests/test_gpu_k4_path.py) fails, this program says which brick is wrong.  WaveExT<3>, WaveExT<5>, BlockEx<2, 3 / 5> and
// BlockEx<4, 3 / 5> on random tiles:
//   * tile_gemm, acc_zero / acc_mac / acc_store (one and two acc_mac on one accumulator), acc_store_init: Kd in {1, 3, 4, 5, 13, 14, 20, 24}
//     (the tails of the 4-wide k-slots, the widest fin operand), nb in {1, 4, 14}, row-major / transposed / padded (TS = 22 / 26) strides
//     for A, B and C, alpha in {1, -1, 0.37}, acc / add both ways; C outside 14 x nb holds a sentinel and must come back untouched;
//   * sum, min, all over the executor's 64 / 128 / 256 lanes with one lane different from the rest, for every lane position;
//   * chain, chain_n (NR = 1, 2, 4) forward and reverse at K in {1, 2, 3, 9, 50}, chain_range_n over parts of a 50-node chain (BlockEx: both
//     halves side by side, as the two-ended solve runs them); coupling tiles of spectral radius about 0.9.
// Bounds are derived, not measured (u = 2^-53):
//   * a product of depth n: |fl - exact| <= (n + 2) u sum |a_k| |b_k| (alpha and the add included; any order of summation, with or without FMA);
//   * chains: the same bound (n = 15: fourteen columns and z) applied along the recursion, the error bound carried beside the values;
//   * sum within (lanes) u sum |x|; min and all exact.
// One line per executor and primitive with the worst ratio of error to bound; exit status 1 if any ratio exceeds 1, a sentinel moved, a
// launch failed or a result differs between lanes.  All inputs are finite, every launch is bounded.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Isuccessiveconvexification_amd/csrc -o k4_executor_ab tools/micro/k4_executor_ab.hip
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "scvx_socp.hpp"

namespace {

constexpr int IMG = 640;                 // doubles per LDS image: the largest index a 14 x 24 tile with stride 26 reaches is 611
constexpr double SENT = -12345.678;      // sentinel outside the 14 x nb block of C and in chain outputs never stored
constexpr long double U = 1.0L / 9007199254740992.0L;   // 2^-53

struct ProdJob {
    int mode;       // 0 tile_gemm, 1 acc_zero + acc_mac + acc_store, 2 two acc_mac on one accumulator, 3 acc_mac + acc_store_init
    int Kd, Kd2, nb, sai, sak, sbk, sbj, sci, scj, add;
    double alpha, alpha2, diag;
};

template <class Ex>
__global__ __launch_bounds__(256) void prod_kernel(const ProdJob* jobs, const double* img, double* out) {
    __shared__ double A[IMG], B[IMG], A2[IMG], B2[IMG], Cm[IMG], H[IMG];
    const ProdJob j = jobs[blockIdx.x];
    const double* src = img + (size_t)blockIdx.x * 6 * IMG;
    for (int e = threadIdx.x; e < IMG; e += blockDim.x) {
        A[e] = src[e]; B[e] = src[IMG + e]; A2[e] = src[2 * IMG + e]; B2[e] = src[3 * IMG + e]; Cm[e] = src[4 * IMG + e]; H[e] = src[5 * IMG + e];
    }
    __syncthreads();
    Ex ex;
    if (j.mode == 0) {
        ex.tile_gemm(Cm, j.sci, j.scj, A, j.sai, j.sak, B, j.sbk, j.sbj, j.Kd, j.alpha, j.add != 0, j.nb);
    } else {
        typename Ex::Acc c;
        ex.acc_zero(c);
        ex.acc_mac(c, A, j.sai, j.sak, B, j.sbk, j.sbj, j.Kd, j.alpha, j.nb);
        if (j.mode == 2) ex.acc_mac(c, A2, j.sai, j.sak, B2, j.sbk, j.sbj, j.Kd2, j.alpha2, j.nb);
        if (j.mode == 3) ex.acc_store_init(c, Cm, H, j.diag);
        else ex.acc_store(c, Cm, j.sci, j.scj, j.add != 0, j.nb);
    }
    __syncthreads();
    for (int e = threadIdx.x; e < IMG; e += blockDim.x) out[(size_t)blockIdx.x * IMG + e] = Cm[e];
}

// one lane different from the rest, for every lane position p: every lane keeps what the reduction handed it
template <class Ex>
__global__ __launch_bounds__(256) void reduce_kernel(double v0, double v1, const double* rnd, double* osum, double* omin, int* oall) {
    Ex ex;
    const int nl = ex.nlanes(), l = ex.lane();
    for (int p = 0; p <= nl; p++) {      // p == nl: no lane differs (sum: the random values of rnd)
        const double xs = p < nl ? (l == p ? v1 : v0) : rnd[l];
        osum[(size_t)p * nl + l] = ex.sum(xs);
        omin[(size_t)p * nl + l] = ex.min(p < nl ? (l == p ? -1.5 : 2.5 + l) : rnd[l]);
        oall[(size_t)p * nl + l] = ex.all(l != p) ? 1 : 0;
    }
}

struct ChainJob {
    int kind;       // 0 chain, 1 chain_n, 2 chain_range_n (one range), 3 chain_range_n of a BlockEx: both halves side by side
    int K, NR, reverse, k0, ns, store_first, k0b, nsb;   // the second range (kind 3): reverse from k0b over nsb nodes
    size_t zoff, noff;   // offsets of this job's z / out ([NR][K][14]) and N ([K][196])
};

template <class Ex, int NR>
__device__ __forceinline__ void chain_job(Ex& ex, const ChainJob& j, const double* z, const double* N, double* out) {
    scvx::ipm::cgptr zs[NR];
    scvx::ipm::gptr os[NR];
    for (int q = 0; q < NR; q++) {
        zs[q] = (scvx::ipm::cgptr)(z + j.zoff + (size_t)q * 14 * j.K);
        os[q] = (scvx::ipm::gptr)(out + j.zoff + (size_t)q * 14 * j.K);
    }
    const scvx::ipm::cgptr Np = (scvx::ipm::cgptr)(N + j.noff);
    if (j.kind == 0) {
        if constexpr (NR == 1) ex.chain(j.K, zs[0], Np, os[0], j.reverse != 0);
    } else if (j.kind == 1) {
        ex.template chain_n<NR>(j.K, zs, Np, os, j.reverse != 0);
    } else if constexpr (Ex::kLanes == 64) {
        ex.template chain_range_n<NR>(j.K, zs, Np, os, j.reverse != 0, j.k0, j.ns, j.store_first != 0);
    } else {
        ex.template chain_range_n<NR>(0, j.K, zs, Np, os, j.reverse != 0, j.k0, j.ns, j.store_first != 0);
        if (j.kind == 3) ex.template chain_range_n<NR>(2, j.K, zs, Np, os, true, j.k0b, j.nsb, j.store_first != 0);
    }
}

template <class Ex>
__global__ __launch_bounds__(256) void chain_kernel(const ChainJob* jobs, const double* z, const double* N, double* out) {
    const ChainJob j = jobs[blockIdx.x];
    Ex ex;
    if (j.NR == 1) chain_job<Ex, 1>(ex, j, z, N, out);
    else if (j.NR == 2) chain_job<Ex, 2>(ex, j, z, N, out);
    else chain_job<Ex, 4>(ex, j, z, N, out);
}

unsigned long long g_rng = 88172645463325252ull;
double rnd() {   // xorshift64: uniform in (-1, 1)
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return (double)(g_rng >> 11) / 4503599627370496.0 - 1.0;
}
int rndi(int n) { g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17; return (int)((g_rng >> 33) % (unsigned)n); }

bool g_fail = false;
void report(const char* exname, const char* prim, double ratio, long checked, long bad) {
    printf("%-12s %-16s worst error / bound %.3f  (%ld values, %ld outside the contract)\n", exname, prim, ratio, checked, bad);
    if (!(ratio <= 1.0) || bad) g_fail = true;
}
#define HIPOK(x) do { if ((x) != hipSuccess) { printf("HIP call failed: %s\n", #x); return false; } } while (0)

template <class Ex>
bool run_products(const char* exname, int TS) {
    const int Kds[8] = {1, 3, 4, 5, 13, 14, 20, 24}, nbs[3] = {1, 4, 14};
    const double alphas[3] = {1.0, -1.0, 0.37};
    const int sA[3][2] = {{TS, 1}, {1, 14}, {1, TS}}, sB[3][2] = {{14, 1}, {1, TS}, {TS, 1}}, sC[3][2] = {{14, 1}, {TS, 1}, {1, TS}};
    std::vector<ProdJob> jobs;
    int seen[4][3][2] = {};
    for (int mode = 0; mode < 4; mode++)
        for (int a = 0; a < 8; a++) for (int b = 0; b < 3; b++) for (int ia = 0; ia < 3; ia++) for (int ib = 0; ib < 3; ib++) for (int ic = 0; ic < 3; ic++) {
            if (mode == 3 && (nbs[b] != 14 || ic != 0)) continue;   // acc_store_init writes a packed 14 x 14 tile
            ProdJob j;
            const int al = rndi(3);
            j.mode = mode; j.Kd = Kds[a]; j.Kd2 = Kds[rndi(8)]; j.nb = nbs[b];
            j.sai = sA[ia][0]; j.sak = sA[ia][1]; j.sbk = sB[ib][0]; j.sbj = sB[ib][1]; j.sci = sC[ic][0]; j.scj = sC[ic][1];
            j.add = rndi(2); j.alpha = alphas[al]; j.alpha2 = alphas[rndi(3)]; j.diag = 0.5 + rnd();
            seen[mode][al][j.add]++;
            jobs.push_back(j);
        }
    for (int m = 0; m < 4; m++) for (int al = 0; al < 3; al++) for (int ad = 0; ad < 2; ad++)
        if (!seen[m][al][ad] && m != 3) { printf("%s: mode %d never drew alpha %g with add %d\n", exname, m, alphas[al], ad); return false; }
    const size_t nj = jobs.size();
    std::vector<double> img(nj * 6 * IMG), out(nj * IMG);
    for (size_t q = 0; q < nj; q++) {
        double* s = &img[q * 6 * IMG];
        for (int e = 0; e < 6 * IMG; e++) s[e] = rnd();
        double* c = s + 4 * IMG;
        std::vector<double> init(14 * 14);
        for (auto& v : init) v = rnd();
        for (int e = 0; e < IMG; e++) c[e] = SENT;
        const ProdJob& j = jobs[q];
        for (int i = 0; i < 14; i++) for (int jj = 0; jj < j.nb; jj++) c[i * j.sci + jj * j.scj] = init[14 * i + jj];
    }
    ProdJob* dj; double *dimg, *dout;
    HIPOK(hipMalloc((void**)&dj, nj * sizeof(ProdJob))); HIPOK(hipMalloc((void**)&dimg, img.size() * 8)); HIPOK(hipMalloc((void**)&dout, out.size() * 8));
    HIPOK(hipMemcpy(dj, jobs.data(), nj * sizeof(ProdJob), hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(dimg, img.data(), img.size() * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemset(dout, 0, out.size() * 8));
    hipLaunchKernelGGL(prod_kernel<Ex>, dim3((unsigned)nj), dim3(Ex::kLanes), 0, 0, dj, dimg, dout);
    HIPOK(hipGetLastError());
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemcpy(out.data(), dout, out.size() * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dj); (void)hipFree(dimg); (void)hipFree(dout);
    const char* names[4] = {"tile_gemm", "acc_mac_store", "acc_mac_twice", "acc_store_init"};
    double worst[4] = {0, 0, 0, 0}; long checked[4] = {0, 0, 0, 0}, bad[4] = {0, 0, 0, 0};
    for (size_t q = 0; q < nj; q++) {
        const ProdJob& j = jobs[q];
        const double *A = &img[q * 6 * IMG], *B = A + IMG, *A2 = A + 2 * IMG, *B2 = A + 3 * IMG, *C0 = A + 4 * IMG, *H = A + 5 * IMG;
        const double* got = &out[q * IMG];
        std::vector<char> inblock(IMG, 0);
        for (int i = 0; i < 14; i++) for (int jj = 0; jj < j.nb; jj++) {
            const int at = i * j.sci + jj * j.scj;
            inblock[at] = 1;
            long double v = 0, S = 0;
            int n = j.Kd + 2;
            for (int k = 0; k < j.Kd; k++) {
                const long double t = (long double)j.alpha * A[i * j.sai + k * j.sak] * B[k * j.sbk + jj * j.sbj];
                v += t; S += fabsl(t);
            }
            if (j.mode == 2) {
                n += j.Kd2;
                for (int k = 0; k < j.Kd2; k++) {
                    const long double t = (long double)j.alpha2 * A2[i * j.sai + k * j.sak] * B2[k * j.sbk + jj * j.sbj];
                    v += t; S += fabsl(t);
                }
            }
            if (j.mode == 3) {
                const long double h = (long double)H[14 * i + jj] + (i == jj ? (long double)j.diag : 0.0L);
                v += h; S += fabsl((long double)H[14 * i + jj]) + (i == jj ? fabsl((long double)j.diag) : 0.0L); n += 1;
            } else if (j.add) {
                v += C0[at]; S += fabsl((long double)C0[at]);
            }
            const long double err = fabsl((long double)got[at] - v), bound = n * U * S;
            const double r = bound > 0 ? (double)(err / bound) : (err == 0 ? 0.0 : 1e300);
            if (!(r <= 1.0)) bad[j.mode]++;
            if (!(r <= worst[j.mode])) worst[j.mode] = r;
            checked[j.mode]++;
        }
        for (int e = 0; e < IMG; e++)
            if (!inblock[e] && memcmp(&got[e], &SENT, 8) != 0) bad[j.mode]++;   // outside 14 x nb: untouched
    }
    for (int m = 0; m < 4; m++) report(exname, names[m], worst[m], checked[m], bad[m]);
    return true;
}

template <class Ex>
bool run_reductions(const char* exname) {
    const int nl = Ex::kLanes;
    const double v0 = 0.1, v1 = -7.3;
    std::vector<double> r(nl), osum((size_t)(nl + 1) * nl), omin((size_t)(nl + 1) * nl);
    std::vector<int> oall((size_t)(nl + 1) * nl);
    for (auto& v : r) v = rnd();
    double *dr, *ds, *dm; int* da;
    HIPOK(hipMalloc((void**)&dr, nl * 8)); HIPOK(hipMalloc((void**)&ds, osum.size() * 8)); HIPOK(hipMalloc((void**)&dm, omin.size() * 8));
    HIPOK(hipMalloc((void**)&da, oall.size() * 4));
    HIPOK(hipMemcpy(dr, r.data(), nl * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemset(ds, 0, osum.size() * 8)); HIPOK(hipMemset(dm, 0, omin.size() * 8)); HIPOK(hipMemset(da, 0xff, oall.size() * 4));
    hipLaunchKernelGGL(reduce_kernel<Ex>, dim3(1), dim3(nl), 0, 0, v0, v1, dr, ds, dm, da);
    HIPOK(hipGetLastError());
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemcpy(osum.data(), ds, osum.size() * 8, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(omin.data(), dm, omin.size() * 8, hipMemcpyDeviceToHost));
    HIPOK(hipMemcpy(oall.data(), da, oall.size() * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dr); (void)hipFree(ds); (void)hipFree(dm); (void)hipFree(da);
    double wsum = 0; long bsum = 0, bmin = 0, ball = 0;
    long double rs = 0, ra = 0; double rmin = r[0];
    for (int l = 0; l < nl; l++) { rs += r[l]; ra += fabsl((long double)r[l]); rmin = r[l] < rmin ? r[l] : rmin; }
    for (int p = 0; p <= nl; p++) {
        const long double ex_ = p < nl ? (long double)v0 * (nl - 1) + (long double)v1 : rs;
        const long double S = p < nl ? fabsl((long double)v0) * (nl - 1) + fabsl((long double)v1) : ra;
        const double mn = p < nl ? -1.5 : rmin;
        const int al = p < nl ? 0 : 1;
        for (int l = 0; l < nl; l++) {
            const size_t at = (size_t)p * nl + l;
            const double rr = (double)(fabsl((long double)osum[at] - ex_) / (nl * U * S));
            if (!(rr <= 1.0) || memcmp(&osum[at], &osum[(size_t)p * nl], 8) != 0) bsum++;   // and every lane holds the same bits
            if (!(rr <= wsum)) wsum = rr;
            if (omin[at] != mn) bmin++;
            if (oall[at] != al) ball++;
        }
    }
    const long n = (long)(nl + 1) * nl;
    report(exname, "sum", wsum, n, bsum);
    report(exname, "min", bmin ? 1e300 : 0.0, n, bmin);
    report(exname, "all", ball ? 1e300 : 0.0, n, ball);
    return true;
}

// the recursion of one range in long double with the running error bound; writes want / bound where the device stores
void chain_ref(const ChainJob& j, int q, const double* z, const double* N, int reverse, int k0, int ns, bool store_first,
               std::vector<long double>& want, std::vector<long double>& bnd, std::vector<char>& stored) {
    const double* zq = z + j.zoff + (size_t)q * 14 * j.K;
    const double* Nt = N + j.noff;
    long double run[14] = {0}, err[14] = {0};
    for (int s = 0; s < ns; s++) {
        const int k = k0 + (reverse ? -s : s);
        long double nxt[14], ne[14];
        for (int i = 0; i < 14; i++) {
            long double a = zq[14 * k + i], S = fabsl(a), e = 0;
            if (s > 0)
                for (int c = 0; c < 14; c++) {
                    const long double m = reverse ? Nt[(size_t)(k + 1) * 196 + 14 * i + c] : Nt[(size_t)k * 196 + 14 * c + i];
                    a += m * run[c];
                    S += fabsl(m) * (fabsl(run[c]) + err[c]);
                    e += fabsl(m) * err[c];
                }
            nxt[i] = a; ne[i] = e + 17 * U * S;
        }
        for (int i = 0; i < 14; i++) {
            run[i] = nxt[i]; err[i] = ne[i];
            if (s > 0 || store_first) { const size_t at = (size_t)q * 14 * j.K + 14 * k + i; want[at] = run[i]; bnd[at] = err[i]; stored[at] = 1; }
        }
    }
}

template <class Ex>
bool run_chains(const char* exname) {
    const int Ks[5] = {1, 2, 3, 9, 50}, NRs[3] = {1, 2, 4};
    std::vector<ChainJob> jobs;
    std::vector<int> prim;   // 0 chain, 1..3 chain_n<1,2,4>, 4 chain_range_n
    size_t zt = 0, nt = 0;
    auto add = [&](ChainJob j, int p) { j.zoff = zt; j.noff = nt; zt += (size_t)j.NR * 14 * j.K; nt += (size_t)196 * j.K; jobs.push_back(j); prim.push_back(p); };
    for (int rep = 0; rep < 4; rep++)
        for (int ki = 0; ki < 5; ki++) for (int rev = 0; rev < 2; rev++) {
            const int K = Ks[ki];
            add(ChainJob{0, K, 1, rev, rev ? K - 1 : 0, K, 1, 0, 0, 0, 0}, 0);
            for (int r = 0; r < 3; r++) add(ChainJob{1, K, NRs[r], rev, rev ? K - 1 : 0, K, 1, 0, 0, 0, 0}, 1 + r);
        }
    for (int rep = 0; rep < 4; rep++)
        for (int r = 0; r < 3; r++) {
            const int K = 50, NR = NRs[r];
            if (Ex::kLanes == 64) {
                add(ChainJob{2, K, NR, 0, 0, K / 2 + 1, 1, 0, 0, 0, 0}, 4);       // the top half, downwards
                add(ChainJob{2, K, NR, 1, K - 1, K - K / 2, 1, 0, 0, 0, 0}, 4);   // the bottom half, upwards
                add(ChainJob{2, K, NR, 0, 7, 20, 0, 0, 0, 0, 0}, 4);              // the first node is not stored
                add(ChainJob{2, K, NR, 1, 40, 15, 0, 0, 0, 0, 0}, 4);
                add(ChainJob{2, 9, NR, 0, 4, 5, 1, 0, 0, 0, 0}, 4);
                add(ChainJob{2, 9, NR, 1, 4, 5, 0, 0, 0, 0, 0}, 4);
            } else {
                add(ChainJob{3, K, NR, 0, 0, K / 2, 1, K - 1, K - K / 2, 0, 0}, 4);   // both halves side by side: nodes 0..24 | 49..25
                add(ChainJob{3, K, NR, 0, 3, 20, 0, 45, 18, 0, 0}, 4);                // nodes 3..22 | 45..28, the first of each not stored
                add(ChainJob{3, 9, NR, 0, 0, 4, 1, 8, 5, 0, 0}, 4);                   // an odd horizon: one more node in the bottom half
                add(ChainJob{2, K, NR, 1, 40, 15, 1, 0, 0, 0, 0}, 4);                 // wavefront 0 alone, upwards
            }
        }
    std::vector<double> z(zt), N(nt), out(zt, SENT);
    const double scale = 0.9 / sqrt(14.0 / 3.0);   // entries U(-1, 1) scale: spectral radius about 0.9
    for (auto& v : z) v = rnd();
    for (auto& v : N) v = scale * rnd();
    ChainJob* dj; double *dz, *dN, *dout;
    HIPOK(hipMalloc((void**)&dj, jobs.size() * sizeof(ChainJob))); HIPOK(hipMalloc((void**)&dz, zt * 8)); HIPOK(hipMalloc((void**)&dN, nt * 8));
    HIPOK(hipMalloc((void**)&dout, zt * 8));
    HIPOK(hipMemcpy(dj, jobs.data(), jobs.size() * sizeof(ChainJob), hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(dz, z.data(), zt * 8, hipMemcpyHostToDevice)); HIPOK(hipMemcpy(dN, N.data(), nt * 8, hipMemcpyHostToDevice));
    HIPOK(hipMemcpy(dout, out.data(), zt * 8, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(chain_kernel<Ex>, dim3((unsigned)jobs.size()), dim3(Ex::kLanes), 0, 0, dj, dz, dN, dout);
    HIPOK(hipGetLastError());
    HIPOK(hipDeviceSynchronize());
    HIPOK(hipMemcpy(out.data(), dout, zt * 8, hipMemcpyDeviceToHost));
    (void)hipFree(dj); (void)hipFree(dz); (void)hipFree(dN); (void)hipFree(dout);
    const char* names[5] = {"chain", "chain_n1", "chain_n2", "chain_n4", "chain_range_n"};
    double worst[5] = {0, 0, 0, 0, 0}; long checked[5] = {0, 0, 0, 0, 0}, bad[5] = {0, 0, 0, 0, 0};
    for (size_t q = 0; q < jobs.size(); q++) {
        const ChainJob& j = jobs[q];
        const size_t n = (size_t)j.NR * 14 * j.K;
        std::vector<long double> want(n, 0), bnd(n, 0);
        std::vector<char> stored(n, 0);
        for (int r = 0; r < j.NR; r++) {
            chain_ref(j, r, z.data(), N.data(), j.reverse, j.k0, j.ns, j.store_first != 0, want, bnd, stored);
            if (j.kind == 3) chain_ref(j, r, z.data(), N.data(), 1, j.k0b, j.nsb, j.store_first != 0, want, bnd, stored);
        }
        const int p = prim[q];
        for (size_t e = 0; e < n; e++) {
            const double g = out[j.zoff + e];
            if (!stored[e]) { if (memcmp(&g, &SENT, 8) != 0) bad[p]++; continue; }
            const double r = (double)(fabsl((long double)g - want[e]) / bnd[e]);
            if (!(r <= 1.0)) bad[p]++;
            if (!(r <= worst[p])) worst[p] = r;
            checked[p]++;
        }
    }
    for (int p = 0; p < 5; p++) report(exname, names[p], worst[p], checked[p], bad[p]);
    return true;
}

template <class Ex>
bool run_all(const char* exname, int TS) {
    return run_products<Ex>(exname, TS) && run_reductions<Ex>(exname) && run_chains<Ex>(exname);
}

}  // namespace

int main() {
    bool ok = run_all<scvx::WaveExT<3>>("WaveExT<3>", 22) && run_all<scvx::WaveExT<5>>("WaveExT<5>", 26)
              && run_all<scvx::BlockEx<2, 3>>("BlockEx<2,3>", 22) && run_all<scvx::BlockEx<2, 5>>("BlockEx<2,5>", 26)
              && run_all<scvx::BlockEx<4, 3>>("BlockEx<4,3>", 22) && run_all<scvx::BlockEx<4, 5>>("BlockEx<4,5>", 26);
    if (!ok) { printf("a launch or a copy failed\n"); return 2; }
    printf(g_fail ? "FAILED\n" : "all primitives within their bounds\n");
    return g_fail ? 1 : 0;
}
