// The prior term of a pathwise GP posterior draw (Matheron's rule; Wilson et al., ICML 2020): random Fourier features (Rahimi & Recht 2007) of
// kappa(x, y) = exp(-a |x - y|^2 / 2) on (x_1 .. x_d, t), whose spectral measure is omega ~ N(0, a I_{d+1}).  models/GP.py has no counterpart (it
// keeps only right_vector); GP.sample_functions adds the data term with scasml_trsm_lower, scasml_gp_cross_rows and scasml_gemm_nt_sub.
//
//   theta_f = omega_f . x (time last)         P_f = wc_f cos theta_f + ws_f sin theta_f         Q_f = ws_f cos theta_f - wc_f sin theta_f
//   u = F^-1/2 sum P_f      Lap = F^-1/2 sum -|omega_f,x|^2 P_f      dt = F^-1/2 sum omega_f,t Q_f      div = F^-1/2 sum (sum_k omega_f,k) Q_f
//
// Feature f of draw r is v = normal4(quad, site = f, root = r, stream = SCASML_STREAM_GP_RFF, key = seed), quads 0 .. (d + 2) / 4, i.e.
// oracle.philox.normals(seed, SCASML_STREAM_GP_RFF, [r], f, d + 3)[0]:  omega_f = sqrt(a) * (double)v[0 : d+1],  wc_f = v[d+1],  ws_f = v[d+2].
//
// ONE workgroup (4 waves) owns one draw and 64 points and sweeps the feature tiles, 64 features at a time, in rising order.  theta (64 points x
// 64 features) is a K = d + 1 product on v_mfma_f64_16x16x4_f64 through the shared tile (f64_mfma_tile.hpp: TileAcc, mfma_tile_k_loop).  The A
// operand is the points, float32 widened.  The B operand, the 64 x 32 stage of omega, is GENERATED: the four threads that park one 4-column
// group of the stage (columns 4 q .. 4 q + 3 of rows r, r + 8, .. r + 56) draw two of its eight Philox blocks each and hand the components round
// inside the quad of lanes (DPP quad_perm: no LDS, no barrier) -- two Philox blocks per thread and stage, none drawn twice, and no S x F x (d+1)
// array in HBM.  The K loop runs over d + 3 columns so that wc and ws are met on the way (they enter B as zeros).
// (The generation of a stage is rff_stage_fetch of gp_rff_stage.hpp, shared with the gradient kernel of gp_rff_grad.hip.)
// The per-feature statistics (|omega_x|^2, sum omega_x, omega_t, wc, ws) are formed while the stages are generated: a thread draws the same
// column group (mod 8) of the same two features in every stage, so it sums its share in registers; after the K loop the eight shares of a
// feature are added in rising order in LDS.
// Epilogue of a feature tile: sincos of the 64 x 64 theta in double, P and Q, four fused multiply-adds into four running sums per accumulator
// row and lane.  After the last tile: a lane has added its column fragments in rising order; the 16 lanes of a row combine by the xor butterfly
// 8, 4, 2, 1 (the f64 C/D map: a lane's registers are rows, its low four bits the column); the two waves side by side add in wave order through
// LDS; one multiplication by F^-1/2.  No atomics, no scratch.
// A point's four values are a function of (x_i, d, a, F, seed, draw index) alone, bit for bit: an MFMA output row depends on its own A row and
// on B, B and the statistics on (seed, draw, feature tile), and the order of every sum is fixed by the feature index.
#include "gp_rff_stage.hpp"

namespace scasml {

constexpr int kRffStats = 5;                 // -|omega_x|^2, omega_t, sum omega_x, wc, ws

__global__ __launch_bounds__(kRffThreads) void gp_rff_kernel(int d, double sqrt_a, const float *__restrict__ x, int64_t n, int64_t ld_x, int F, double inv_sqrt_f,
                                                            uint32_t k0, uint32_t k1, uint32_t root0, int64_t tiles, double *__restrict__ out) {
    constexpr int NT = 2, PER = kRffTile * NB / kRffThreads;
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double share[kRffTile][8][2];               // a feature's |omega_x|^2 and sum omega_x by column group mod 8
    __shared__ double stat[kRffTile][kRffStats];
    __shared__ double red[2][kRffTile][4];
    normal_table_to_lds();
    const int64_t s = (int64_t)blockIdx.x / tiles, p0 = ((int64_t)blockIdx.x % tiles) * kRffTile;
    const uint32_t root = root0 + (uint32_t)s;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = (wv >> 1) * (16 * NT), wc = (wv & 1) * (16 * NT);
    const int l15 = lane & 15, l4 = lane >> 4;
    const int m4 = tid & 3, qs = (tid >> 2) & 7, rbase = tid >> 5;       // this thread parks column 4 qs + m4 of rows rbase + 8 e
    const int kdim = d + 1, kend = d + 3;
    double sum[NT][4][4];                                    // [row fragment][register][u, Lap, dt, div]
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) sum[i][e][q] = 0.0;

    for (int f0 = 0; f0 < F; f0 += kRffTile) {
        double w2[2] = {0.0, 0.0}, w1[2] = {0.0, 0.0};      // this thread's share of its two features' statistics
        TileAcc<NT> t;
        mfma_tile_zero(t);
        mfma_tile_k_loop<NT>(smem, 0, kend, [&](int64_t kk, double (&ra)[PER], double (&rb)[PER]) {
            rff_stage_fetch(d, sqrt_a, x, n, ld_x, F, k0, k1, root, p0, f0, kk, ra, rb, [&](int h, int fr, int k, float c, double om) {
                if (k < d) {
                    w2[h] = fma(om, om, w2[h]);
                    w1[h] += om;
                } else if (k == d) {
                    stat[fr][1] = om;
                } else if (k == d + 1) {
                    stat[fr][3] = (double)c;
                } else if (k == d + 2) {
                    stat[fr][4] = (double)c;
                }
            });
        }, [] {}, t);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            share[rbase + 8 * (2 * m4 + h)][qs][0] = w2[h];
            share[rbase + 8 * (2 * m4 + h)][qs][1] = w1[h];
        }
        __syncthreads();
        if (tid < kRffTile) {
            double a2 = 0.0, a1 = 0.0;
#pragma unroll
            for (int g = 0; g < 8; ++g) {
                a2 += share[tid][g][0];
                a1 += share[tid][g][1];
            }
            stat[tid][0] = -a2;
            stat[tid][2] = a1;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int fc = wc + 16 * j + l15;
            const double mlap = stat[fc][0], mdt = stat[fc][1], mdiv = stat[fc][2], fwc = stat[fc][3], fws = stat[fc][4];
#pragma unroll
            for (int i = 0; i < NT; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    double sn, cs;
                    sincos(t.v[i][j][e], &sn, &cs);
                    const double P = fma(fws, sn, fwc * cs), Q = fma(-fwc, sn, fws * cs);
                    sum[i][e][0] += P;
                    sum[i][e][1] = fma(mlap, P, sum[i][e][1]);
                    sum[i][e][2] = fma(mdt, Q, sum[i][e][2]);
                    sum[i][e][3] = fma(mdiv, Q, sum[i][e][3]);
                }
        }
        __syncthreads();                                      // stat, share and the operand panels are the next tile's
    }
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double v = sum[i][e][q];
#pragma unroll
                for (int m = 8; m > 0; m >>= 1) v += __shfl_xor(v, m);
                if (l15 == 0) red[wv & 1][wr + 16 * i + l4 + 4 * e][q] = v;
            }
    __syncthreads();
    const int pr = tid >> 2, q = tid & 3;
    if (p0 + pr < n) out[((s * n) + p0 + pr) * 4 + q] = (red[0][pr][q] + red[1][pr][q]) * inv_sqrt_f;
}

// out[s * ld + j] = (double) component j % 4 of normal4(quad = j / 4, site = 0, root = sample0 + s, stream = SCASML_STREAM_GP_RFF_NOISE)
__global__ __launch_bounds__(kRffThreads) void gp_rff_noise_kernel(int64_t M, uint32_t k0, uint32_t k1, uint32_t root0, double *__restrict__ out, int64_t ld) {
    normal_table_to_lds();
    const int64_t quad = (int64_t)blockIdx.x * kRffThreads + threadIdx.x, s = blockIdx.y;
    if (4 * quad >= M) return;
    const float4 v = normal4((uint32_t)quad, 0u, root0 + (uint32_t)s, SCASML_STREAM_GP_RFF_NOISE, k0, k1);
    const float c[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if (4 * quad + j < M) out[s * ld + 4 * quad + j] = (double)c[j];
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_gp_rff_functionals(int32_t d, double a, const float *x, int64_t n, int64_t ld_x, int32_t F, uint64_t seed, int64_t sample0,
                                         int64_t S, double *out, void *stream) {
    if (!x || !out) return fail(SCASML_ERR_ARG, "gp_rff_functionals: null argument");
    if (d < 1 || d > SCASML_MAX_DIM) return fail(SCASML_ERR_ARG, "gp_rff_functionals: d=%d outside 1..%d", (int)d, SCASML_MAX_DIM);
    if (!(a > 0.0) || !isfinite(a)) return fail(SCASML_ERR_ARG, "gp_rff_functionals: a=%g is not a positive scale", a);
    if (F < 1) return fail(SCASML_ERR_ARG, "gp_rff_functionals: F=%d features", (int)F);
    if (n < 0 || ld_x < (int64_t)d + 1) return fail(SCASML_ERR_ARG, "gp_rff_functionals: n=%lld, ld_x=%lld (d + 1 = %d)", (long long)n, (long long)ld_x, (int)d + 1);
    if (const int rc = check_draws("gp_rff_functionals", sample0, S)) return rc;
    if (n == 0 || S == 0) return 0;
    const int64_t tiles = (n + kRffTile - 1) / kRffTile;
    if (tiles > (int64_t)1 << 30) return fail(SCASML_ERR_UNSUPPORTED, "gp_rff_functionals: too many points for one launch");
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(gp_rff_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds_bytes<2>()) != hipSuccess)
        return fail(SCASML_ERR_HIP, "gp_rff_functionals: cannot reserve %zu bytes of LDS", tile_lds_bytes<2>());
    const int64_t per = ((int64_t)1 << 30) / tiles;           // draws per launch: a 1-D grid below 2^31 workgroups
    for (int64_t s0 = 0; s0 < S; s0 += per) {
        const int64_t c = S - s0 < per ? S - s0 : per;
        hipLaunchKernelGGL(gp_rff_kernel, dim3((unsigned)(c * tiles)), dim3(kRffThreads), tile_lds_bytes<2>(), (hipStream_t)stream, (int)d, sqrt(a), x, n, ld_x,
                           (int)F, 1.0 / sqrt((double)F), (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)(sample0 + s0), tiles,
                           out + s0 * n * 4);
        if (const int rc = check_launch("gp_rff_functionals launch")) return rc;
    }
    return 0;
}

extern "C" int scasml_gp_rff_noise(int64_t M, uint64_t seed, int64_t sample0, int64_t S, double *out, int64_t ld, void *stream) {
    if (!out) return fail(SCASML_ERR_ARG, "gp_rff_noise: null argument");
    if (M < 0 || ld < M) return fail(SCASML_ERR_ARG, "gp_rff_noise: M=%lld, ld=%lld", (long long)M, (long long)ld);
    if (const int rc = check_draws("gp_rff_noise", sample0, S)) return rc;
    if (M == 0 || S == 0) return 0;
    const int64_t gx = ((M + 3) / 4 + kRffThreads - 1) / kRffThreads;
    if (gx > 0x7FFFFFFF) return fail(SCASML_ERR_UNSUPPORTED, "gp_rff_noise: M=%lld is too long for one launch", (long long)M);
    for (int64_t s0 = 0; s0 < S; s0 += 65535) {
        const int64_t c = S - s0 < 65535 ? S - s0 : 65535;
        hipLaunchKernelGGL(gp_rff_noise_kernel, dim3((unsigned)gx, (unsigned)c), dim3(kRffThreads), 0, (hipStream_t)stream, M, (uint32_t)(seed & 0xFFFFFFFFu),
                           (uint32_t)(seed >> 32), (uint32_t)(sample0 + s0), out + s0 * ld, ld);
        if (const int rc = check_launch("gp_rff_noise launch")) return rc;
    }
    return 0;
}
