// What the two random-Fourier-feature kernels share (gp_rff.hip: the four functionals of a prior draw; gp_rff_grad.hip: its gradient): the tile
// shape, the quad hand-over, the generation of one 64 x 32 stage of omega for the theta product, and the check of the draw indices.  Both kernels
// draw feature f of draw r as normal4(quad, site = f, root = r, stream = SCASML_STREAM_GP_RFF, key = seed) and form omega = sqrt(a) * (double)v, so
// draw r of the one is the same function as draw r of the other.
#pragma once
#include "common.hpp"
#include "f64_mfma_tile.hpp"
#include "philox_normal.hpp"

namespace scasml {

constexpr int kRffTile = 64, kRffThreads = 256;

// lane `src` (0..3) of every quad of lanes hands its value to all four; src is a constant once the caller's loop is unrolled
template <int SRC>
__device__ __forceinline__ float quad_lane(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), SRC * 0x55, 0xf, 0xf, false));
}
__device__ __forceinline__ float quad_broadcast(float v, int src) {
    return src == 0 ? quad_lane<0>(v) : src == 1 ? quad_lane<1>(v) : src == 2 ? quad_lane<2>(v) : quad_lane<3>(v);
}

// This thread's elements of the two operand chunks of columns [kk, kk + NB) of the theta product (mfma_tile_k_loop's fetch): ra from the points
// p0 .. p0 + 63 (float32 widened, zeros past n and past column d), rb from the GENERATED stage of omega, features f0 .. f0 + 63 (zeros past F and
// past column d).  The four threads that park one 4-column group of the stage (columns 4 q .. 4 q + 3 of rows r, r + 8, .. r + 56) draw two of its
// eight Philox blocks each and hand the components round inside the quad of lanes.  visit(h, fr, k, c, om) sees every normal this thread drew:
// its block h (0, 1), the feature's row fr in the tile, the column k < d + 3, the float32 normal c and om = sqrt_a * (double)c.
template <class Visit>
__device__ __forceinline__ void rff_stage_fetch(int d, double sqrt_a, const float *__restrict__ x, int64_t n, int64_t ld_x, int F, uint32_t k0, uint32_t k1,
                                                uint32_t root, int64_t p0, int f0, int64_t kk, double (&ra)[8], double (&rb)[8], Visit visit) {
    constexpr int PER = kRffTile * NB / kRffThreads;
    static_assert(PER == 8, "the quad hand-over is written for eight elements per thread");
    const int tid = threadIdx.x;
    const int m4 = tid & 3, qs = (tid >> 2) & 7, rbase = tid >> 5;       // this thread parks column 4 qs + m4 of rows rbase + 8 e
    const int kdim = d + 1, kend = d + 3;
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int idx = tid + e * kRffThreads, rr = idx / NB, cc = idx % NB;
        const int64_t p = p0 + rr;
        ra[e] = (p < n && kk + cc < kdim) ? (double)x[p * ld_x + kk + cc] : 0.0;
    }
    // blocks e = 2 m4 and 2 m4 + 1 of this quad of lanes: features f0 + rbase + 8 e, columns kk + 4 qs .. + 3
    float4 blk[2];
    const int col0 = (int)kk + 4 * qs;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int fr = rbase + 8 * (2 * m4 + h), f = f0 + fr;
        blk[h] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col0 < kend) {                            // features past F: zeros, so that P = Q = 0
            const float4 v = f < F ? normal4((uint32_t)(col0 >> 2), (uint32_t)f, root, SCASML_STREAM_GP_RFF, k0, k1) : blk[h];
            const float c[4] = {v.x, v.y, v.z, v.w};
            float b[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int k = col0 + j;
                visit(h, fr, k, c[j], sqrt_a * (double)c[j]);
                b[j] = k < kdim ? c[j] : 0.f;
            }
            blk[h] = make_float4(b[0], b[1], b[2], b[3]);
        }
    }
    // element e of this thread is component m4 of block e, held by lane e / 2 of the quad as its block e % 2
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const float4 &b = blk[e % 2];
        const float c0 = quad_broadcast(b.x, e / 2), c1 = quad_broadcast(b.y, e / 2), c2 = quad_broadcast(b.z, e / 2), c3 = quad_broadcast(b.w, e / 2);
        rb[e] = sqrt_a * (double)(m4 == 0 ? c0 : m4 == 1 ? c1 : m4 == 2 ? c2 : c3);
    }
}

static inline int check_draws(const char *who, int64_t sample0, int64_t S) {
    if (S < 0 || sample0 < 0) return fail(SCASML_ERR_ARG, "%s: negative draw count or index", who);
    if (sample0 > (int64_t)1 << 32 || S > ((int64_t)1 << 32) - sample0)
        return fail(SCASML_ERR_UNSUPPORTED, "%s: draw indices %lld .. %lld reach 2^32 (the Philox root word is 32 bits)", who, (long long)sample0,
                    (long long)sample0 + (long long)S - 1);
    return 0;
}

}  // namespace scasml
