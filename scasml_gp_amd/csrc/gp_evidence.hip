// The GP log marginal likelihood's device pieces (no counterpart in models/GP.py, which hard-codes sigma and the nugget, :25-26):
//   LML = -1/2 z^T alpha - 1/2 log det K_p - M/2 log(2 pi),   dLML/da = 1/2 alpha^T K_a alpha - 1/2 tr(K_p^-1 K_a),   K_a = dK/da, a = 1 / sigma^2.
// (1) scasml_chol_logdet: 2 sum_i log L[i][i] of the factor scasml_cholesky leaves (its identity padding adds log 1 = 0).
// (2) scasml_gp_gram_da_contract: sum_ij alpha_i alpha_j K_a[i][j] and sum_ij A[i][j] K_a[i][j] in ONE pass of Gram-tile size, K_a never stored.
//
// The pass is the Gram's 64 x 64 pair tile (gp_gram_tile.hpp): x.y on v_mfma_f64_16x16x4_f64, K = d + 1 streamed through LDS, per-point
// statistics in LDS.  An entry of K is P(ox, oy) kappa with kappa = exp(-a r^2 / 2), so the entry of K_a is (P_a - r^2 P / 2) kappa, P_a = dP/da at
// fixed geometry (gp_gram_table.hpp).  The visit evaluates that table for the pair's up to 16 entries and multiplies each by its A entry and its alpha_i alpha_j (the
// alphas of the tile's 64 + 64 points sit in LDS beside the statistics).  K_a is symmetric and A is read as a full symmetric matrix (what
// scasml_cholesky_inverse leaves), so only the tiles on or below the diagonal are walked and the off-diagonal ones count twice.
//
// Reduction, one fixed order and no atomics (the two sums are the same bits on every run): a thread adds its entries in the order of its loops
// (column tile, row tile, fragment register, x-operator, y-operator); a wave combines its lanes by the xor butterfly 32, 16, .., 1; the workgroup's
// thread 0 adds the four waves in wave order, doubles an off-diagonal tile's pair and writes it to the workgroup's slot of the partials; a second
// launch of one workgroup adds the slots -- thread t those with index = t mod 256 in rising order, then a halving tree over the 256 threads in LDS.
#include <math.h>

#include "common.hpp"
#include "gp_gram_tile.hpp"

namespace scasml {

constexpr int kEvThreads = 256;

// sum of v over the workgroup's 256 threads in a fixed order: the halving tree in LDS; every thread must call it; the result is thread 0's
__device__ __forceinline__ double ev_block_sum(double v, double *red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int s = kEvThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kEvThreads) void chol_logdet_kernel(const double *__restrict__ L, int64_t Mp, double *out) {
    __shared__ double red[kEvThreads];
    double s = 0.0;
    for (int64_t i = threadIdx.x; i < Mp; i += kEvThreads) s += log(L[i * Mp + i]);
    const double tot = ev_block_sum(s, red);
    if (threadIdx.x == 0) out[0] = 2.0 * tot;
}

// which tile of the lower triangle (ti >= tj) is block b, in the order (0,0), (1,0), (1,1), (2,0), ...
__device__ __forceinline__ void ev_tile_of_block(int64_t b, int &ti, int &tj) {
    int64_t r = (int64_t)((sqrt(8.0 * (double)b + 1.0) - 1.0) * 0.5);
    while (r * (r + 1) / 2 > b) --r;
    while ((r + 1) * (r + 2) / 2 <= b) ++r;
    ti = (int)r;
    tj = (int)(b - r * (r + 1) / 2);
}

__global__ __launch_bounds__(kGramThreads) void gp_gram_da_contract_kernel(GramPoints pts, double a, const double *__restrict__ A, int64_t lda,
                                                                           const double *__restrict__ alpha, double *partials) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double stat[2 * kGramTile][4];
    __shared__ double alf[2 * kGramTile][4];     // alpha at the point's u, Lap, dt, div features (0 where a boundary point has none)
    __shared__ double wsum[kGramThreads / 64][2];
    int ti, tj;
    ev_tile_of_block(blockIdx.x, ti, tj);
    const int i0 = ti * kGramTile, j0 = tj * kGramTile;
    {   // two threads per point as in the tile's statistics; this thread's two of the point's four alphas: operators par and par + 2
        const int q = threadIdx.x >> 1, par = threadIdx.x & 1;
        const int p = q < kGramTile ? i0 + q : j0 + q - kGramTile;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int op = par + 2 * h;
            alf[q][op] = p < pts.N() && op < pts.nops(p) ? alpha[pts.feature(op, p)] : 0.0;
        }
    }   // visible to everyone after the barriers of the tile's K loop
    const double fd = (double)pts.d;
    double acc_q = 0.0, acc_t = 0.0;             // alpha^T K_a alpha and <A, K_a> over this thread's pairs
    gram_pair_tile(pts, i0, pts.N(), j0, smem, stat, [&](int i, int j, int il, int jl, double r2, double rt, double S) {
        double ka[4][4];
        gram_pair<kGramKa>(a, fd, r2, rt, S, ka);
        const int nops_i = pts.nops(i), nops_j = pts.nops(j);
#pragma unroll
        for (int ox = 0; ox < 4; ++ox) {
            if (ox >= nops_i) continue;
            const double *Arow = A + pts.feature(ox, i) * lda;
#pragma unroll
            for (int oy = 0; oy < 4; ++oy) {
                if (oy >= nops_j) continue;
                acc_q = fma(alf[il][ox] * alf[kGramTile + jl][oy], ka[ox][oy], acc_q);
                acc_t = fma(Arow[pts.feature(oy, j)], ka[ox][oy], acc_t);
            }
        }
    });
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
        acc_q += __shfl_xor(acc_q, m);
        acc_t += __shfl_xor(acc_t, m);
    }
    if (lane == 0) {
        wsum[wv][0] = acc_q;
        wsum[wv][1] = acc_t;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double w = ti == tj ? 1.0 : 2.0;   // the mirrored tile above the diagonal holds the same products
        partials[2 * (int64_t)blockIdx.x] = w * (((wsum[0][0] + wsum[1][0]) + wsum[2][0]) + wsum[3][0]);
        partials[2 * (int64_t)blockIdx.x + 1] = w * (((wsum[0][1] + wsum[1][1]) + wsum[2][1]) + wsum[3][1]);
    }
}

__global__ __launch_bounds__(kEvThreads) void gp_evidence_sum_kernel(const double *__restrict__ partials, int64_t n, double *out) {
    __shared__ double red[kEvThreads];
    double sq = 0.0, st = 0.0;
    for (int64_t b = threadIdx.x; b < n; b += kEvThreads) {
        sq += partials[2 * b];
        st += partials[2 * b + 1];
    }
    const double tq = ev_block_sum(sq, red);
    __syncthreads();
    const double tt = ev_block_sum(st, red);
    if (threadIdx.x == 0) {
        out[0] = tq;
        out[1] = tt;
    }
}

static int64_t ev_tiles(int32_t n_dom, int32_t n_bdy) {
    const int64_t gt = ((int64_t)n_dom + n_bdy + 63) / 64;
    return gt * (gt + 1) / 2;
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_chol_logdet(const double *L, int64_t Mp, double *out_dev, void *stream) {
    if (!L || !out_dev || Mp < 1) return fail(SCASML_ERR_ARG, "chol_logdet: bad argument");
    hipLaunchKernelGGL(chol_logdet_kernel, dim3(1), dim3(kEvThreads), 0, (hipStream_t)stream, L, Mp, out_dev);
    return check_launch("chol_logdet launch");
}

extern "C" int64_t scasml_gp_gram_da_contract_doubles(int32_t n_dom, int32_t n_bdy) {
    if (n_dom < 1 || n_bdy < 0) return 0;
    return 2 + 2 * ev_tiles(n_dom, n_bdy);
}

extern "C" int scasml_gp_gram_da_contract(int32_t d, double a, const float *x_dom, int32_t n_dom, const float *x_bdy, int32_t n_bdy, const double *A,
                                          int64_t lda, const double *alpha, double *out_dev, void *stream) {
    if (!x_dom || !A || !alpha || !out_dev || (n_bdy > 0 && !x_bdy)) return fail(SCASML_ERR_ARG, "gp_gram_da_contract: null argument");
    if (d < 1 || n_dom < 1 || n_bdy < 0 || lda < 4 * (int64_t)n_dom + n_bdy) return fail(SCASML_ERR_ARG, "gp_gram_da_contract: bad sizes");
    if (((int64_t)n_dom + n_bdy + 63) / 64 > 65535)
        return fail(SCASML_ERR_UNSUPPORTED, "gp_gram_da_contract: too many collocation points for one launch");
    const int64_t tiles = ev_tiles(n_dom, n_bdy);      // <= 65535 * 65536 / 2 < 2^31: one grid dimension
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(gp_gram_da_contract_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kGramLdsBytes) != hipSuccess)
        return fail(SCASML_ERR_HIP, "gp_gram_da_contract: cannot reserve LDS");
    double *partials = out_dev + 2;
    hipLaunchKernelGGL(gp_gram_da_contract_kernel, dim3((unsigned)tiles), dim3(kGramThreads), kGramLdsBytes, (hipStream_t)stream,
                       GramPoints{d, x_dom, n_dom, x_bdy, n_bdy}, a, A, lda, alpha, partials);
    hipLaunchKernelGGL(gp_evidence_sum_kernel, dim3(1), dim3(kEvThreads), 0, (hipStream_t)stream, partials, tiles, out_dev);
    return check_launch("gp_gram_da_contract launch");
}
