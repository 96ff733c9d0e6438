// The draws of the sampled closed-loop dispersion made ON THE DEVICE (scvx_track_mc_rng_f64, scvx_track_mc_nav_rng_f64,
// scvx_mc_draws_f64; include/scvx.h spells out the stream): defined here once and used by both flying kernels (scvx_mc.hip,
// scvx_mc_nav.hip) and by the dump kernel, so dumped and consumed draws are the same bits.  Not part of the ABI.
//
// Generator: Philox4x64-10 exactly as numpy's np.random.Philox -- key [seed, 0]; block j of the stream with base counter
// [0, c1, c2, c3] is the block of counter [1 + j, c1, c2, c3] (numpy increments before its first block).  c1 = 6 for the truth (xi0,
// eta), 7 for the navigation error (xin, nud), beside the host helpers' 4 and 5; c3 = s_lo + s; c2 = 0 with shared draws, 1 + b_lo + b
// with independent ones.  A group of 14 draws occupies 4 blocks = 16 normals, draw i is normal i & 3 of block i >> 2 (two are unused);
// group 0 is the start, group 1 + k belongs to node k: any (s, k, i) is random access and nothing depends on m, on K or on the noise.
// Normals: Box-Muller per block, u_j = ((w_j >> 11) + 0.5) 2^-53 in double arithmetic (never 0; the sum rounds to even above 2^52, so
// u is a multiple of 2^-53 in (0, 1]), (z0, z1) = sqrt(-2 log u0) (cospi(2 u1), sinpi(2 u1)) and (z2, z3) likewise from u2, u3.  The
// two products are __dmul_rn: nothing here can be contracted into a consumer's sum, in whichever kernel it is inlined.
#pragma once
#include <cstdint>
#include <hip/hip_runtime.h>

namespace scvx {

constexpr uint64_t PHILOX_M0 = 0xD2E7470EE14C6C93ull, PHILOX_M1 = 0xCA5A826395121157ull;
constexpr uint64_t PHILOX_W0 = 0x9E3779B97F4A7C15ull, PHILOX_W1 = 0xBB67AE8584CAA73Bull;
constexpr uint64_t MC_STREAM_TRUTH = 6, MC_STREAM_NAV = 7, MC_STREAM_VEH = 8;   // VEH: the vehicle errors, the first six normals of group 0

// scvx_mc_rng as the kernels take it, and whether the truth receives impulses
struct McRngK {
    uint64_t seed, s_lo, b_lo;
    int independent, noise;
};

__device__ __forceinline__ void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1, uint64_t w[4]) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t h0 = __umul64hi(PHILOX_M0, c0), l0 = PHILOX_M0 * c0;
        const uint64_t h1 = __umul64hi(PHILOX_M1, c2), l1 = PHILOX_M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

__device__ __forceinline__ double mc_unit(uint64_t w) { return (double(w >> 11) + 0.5) * 0x1p-53; }

__device__ __forceinline__ void mc_box_muller(uint64_t wa, uint64_t wb, double& z0, double& z1) {
    const double r = sqrt(-2.0 * log(mc_unit(wa)));
    double s, c;
    sincospi(2.0 * mc_unit(wb), &s, &c);
    z0 = __dmul_rn(r, c);
    z1 = __dmul_rn(r, s);
}

// c2 and c3 of flight (b, s)
__device__ __forceinline__ uint64_t mc_rng_c2(const McRngK& g, int b) { return g.independent ? 1 + g.b_lo + uint64_t(b) : 0; }
__device__ __forceinline__ uint64_t mc_rng_c3(const McRngK& g, int s) { return g.s_lo + uint64_t(s); }

// the first cnt (<= 14) draws of group grp of stream c1 into z; only the blocks that hold them are formed
__device__ __forceinline__ void mc_draw_group(uint64_t seed, uint64_t c1, uint64_t c2, uint64_t c3, int grp, int cnt, double z[16]) {
#pragma unroll
    for (int blk = 0; blk < 4; blk++) {
        if (4 * blk < cnt) {
            uint64_t w[4];
            philox4x64_10(uint64_t(1) + 4 * uint64_t(grp) + blk, c1, c2, c3, seed, 0, w);
            mc_box_muller(w[0], w[1], z[4 * blk], z[4 * blk + 1]);
            mc_box_muller(w[2], w[3], z[4 * blk + 2], z[4 * blk + 3]);
        }
    }
}

}  // namespace scvx
