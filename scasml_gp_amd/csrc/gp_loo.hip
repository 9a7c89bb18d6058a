// The device pieces of the GP leave-one-out gradient in the scale (no counterpart in models/GP.py, which hard-codes sigma and the nugget, :25-26).
// With A = K_p^-1, alpha = A z and K_a = dK/da (a = 1 / sigma^2) the gradient of the LOO predictive log-likelihood needs, for every feature i,
//   q_i = [A K_a A]_ii = sum_jk A[i][j] K_a[j][k] A[i][k]     and     v_i = [K_a alpha]_i
// (Rasmussen & Williams 5.4.2).  q is an M^3 product with a matrix the library never stores whole:
// (1) scasml_gp_gram_da_rows: feature rows of K_a, the twin of scasml_gp_gram_rows (gp_train.hip) -- the same rows kernel of the 64 x 64 pair
//     tile (gp_gram_tile.hpp), instantiated for the entries (P_a - r^2 P / 2) kappa of gp_gram_table.hpp in place of P kappa.
// (2) scasml_gp_loo_da: K_a is walked in panels of panel_rows feature rows.  A panel P (panel_rows x M) is written by (1) into the workspace, v of
//     its rows is one row reduction of it, and the tile kernel forms T = A[I, :] P^T for a block I of 64 rows of A and 64 rows c of the panel on
//     v_mfma_f64_16x16x4_f64 (K dimension M, streamed through LDS by mfma_tile_k_loop).  K_a is symmetric, so T[i][c] = [A K_a]_i,row0+c and the
//     epilogue multiplies it by A[i][row0 + c] and sums along the row instead of storing T: q_i = sum_c A[i][c] [A K_a]_ic.
//
// Reduction of q, one fixed order and no atomics: a lane adds its two columns (c = l15, then l15 + 16 of the wave's 32), the 16 lanes of a row
// combine by the xor butterfly 8, 4, 2, 1, the two waves side by side add in wave order through LDS: that is the partial of (row i, 64-column tile
// ct) and goes to partials[ct][i].  Panels start at multiples of 64, so a column tile is the same 64 features whatever panel_rows is, an entry of
// T is one dot product over k in rising chunks, and the last kernel adds a row's partials in rising ct: q is the same bits for every panel_rows.
// v_i: lane l of the row's wave adds columns l, l + 64, .. in rising order, then the xor butterfly 32 .. 1 -- a function of the row alone.
#include <math.h>

#include "common.hpp"
#include "f64_mfma_tile.hpp"
#include "gp_gram_tile.hpp"

namespace scasml {

constexpr int kLooThreads = 256;
constexpr int kLooTile = 64;                 // rows of A and rows of the panel per workgroup
constexpr int kLooDefaultPanelRows = 512;

// v_out[r] = sum_j P[r][j] alpha[j] for the panel's rows r < nrows: one wave per row
__global__ __launch_bounds__(kLooThreads) void gp_loo_panel_gemv_kernel(const double *__restrict__ P, int64_t ldp, int nrows, int64_t M,
                                                                        const double *__restrict__ alpha, double *v_out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kLooThreads / 64) + (threadIdx.x >> 6);
    if (r >= nrows) return;                      // wave-uniform
    const double *row = P + r * ldp;
    double s = 0.0;
    for (int64_t j = lane; j < M; j += 64) s = fma(row[j], alpha[j], s);
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if (lane == 0) v_out[r] = s;
}

// partials[ct][i] = sum over the 64 panel rows c of column tile ct = (row0 + 64 blockIdx.y) / 64 of A[i][row0 + c] * sum_k A[i][k] P[c][k],
// for the 64 rows i of block blockIdx.x.  A is read inside its first M rows and columns only, the panel inside its nrows x M written part.
__global__ __launch_bounds__(kLooThreads) void gp_loo_tile_kernel(const double *__restrict__ A, int64_t lda, int64_t M, const double *__restrict__ P,
                                                                  int64_t ldp, int64_t row0, int nrows, double *partials) {
    constexpr int NT = 2, TBX = 32 * NT, PER = TBX * NB / kLooThreads;
    static_assert(TBX == kLooTile, "the column tile of the partials is the workgroup's tile");
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double red[2][TBX];
    const int64_t i0 = (int64_t)blockIdx.x * TBX;
    const int c0 = blockIdx.y * TBX;
    const bool interior = i0 + TBX <= M && c0 + TBX <= nrows;        // block-uniform
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = (wv >> 1) * (16 * NT), wc = (wv & 1) * (16 * NT);
    const int l15 = lane & 15, l4 = lane >> 4;
    TileAcc<NT> t;
    mfma_tile_zero(t);
    double w[NT][NT][4];                         // A[i][row0 + c] of this lane's entries of T
    const int64_t kend = (M + NB - 1) / NB * NB;
    mfma_tile_k_loop<NT>(smem, 0, kend, [&](int64_t kk, double (&ra)[PER], double (&rb)[PER]) {
        if (interior && kk + NB <= M) {          // no bounds tests, loads issued back to back
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const int idx = threadIdx.x + e * kLooThreads, rr = idx / NB, cc = idx % NB;
                ra[e] = A[(i0 + rr) * lda + kk + cc];
                rb[e] = P[(int64_t)(c0 + rr) * ldp + kk + cc];
            }
        } else {
#pragma unroll
            for (int e = 0; e < PER; ++e) {
                const int idx = threadIdx.x + e * kLooThreads, rr = idx / NB, cc = idx % NB;
                const bool k_in = kk + cc < M;
                ra[e] = (k_in && i0 + rr < M) ? A[(i0 + rr) * lda + kk + cc] : 0.0;
                rb[e] = (k_in && c0 + rr < nrows) ? P[(int64_t)(c0 + rr) * ldp + kk + cc] : 0.0;
            }
        }
    }, [&] {                                     // the weights' loads fly under the last chunk's matrix work
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
            for (int jt = 0; jt < NT; ++jt)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int64_t i = i0 + wr + 16 * it + l4 + 4 * e;
                    const int c = c0 + wc + 16 * jt + l15;
                    w[it][jt][e] = (i < M && c < nrows) ? A[i * lda + row0 + c] : 0.0;
                }
    }, t);
#pragma unroll
    for (int it = 0; it < NT; ++it)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            double s = w[it][0][e] * t.v[it][0][e];
            s = fma(w[it][1][e], t.v[it][1][e], s);
#pragma unroll
            for (int m = 8; m > 0; m >>= 1) s += __shfl_xor(s, m);
            if (l15 == 0) red[wv & 1][wr + 16 * it + l4 + 4 * e] = s;
        }
    __syncthreads();
    if (threadIdx.x < TBX && i0 + threadIdx.x < M) {
        const int64_t ct = (row0 + c0) / TBX;
        partials[ct * M + i0 + threadIdx.x] = red[0][threadIdx.x] + red[1][threadIdx.x];
    }
}

// q_out[i] = the row's partials added in rising column-tile order
__global__ __launch_bounds__(kLooThreads) void gp_loo_sum_kernel(const double *__restrict__ partials, int64_t M, int64_t nct, double *q_out) {
    const int64_t i = (int64_t)blockIdx.x * kLooThreads + threadIdx.x;
    if (i >= M) return;
    double s = 0.0;
    for (int64_t ct = 0; ct < nct; ++ct) s += partials[ct * M + i];
    q_out[i] = s;
}

// the panel height in use: the caller's, else the default; never more than M rounded up to the tile
static int64_t loo_panel_rows(int64_t M, int32_t panel_rows) {
    const int64_t cover = (M + kLooTile - 1) / kLooTile * kLooTile;
    const int64_t pr = panel_rows > 0 ? panel_rows : kLooDefaultPanelRows;
    return pr < cover ? pr : cover;
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_gp_gram_da_rows(int32_t d, double a, const float *x_dom, int32_t n_dom, const float *x_bdy, int32_t n_bdy, int64_t row0,
                                      int32_t nrows, int64_t ncols, double *out, int64_t ld, void *stream) {
    if (!x_dom || !out || (n_bdy > 0 && !x_bdy)) return fail(SCASML_ERR_ARG, "gp_gram_da_rows: null argument");
    const int64_t M = 4 * (int64_t)n_dom + n_bdy;
    if (d < 1 || n_dom < 1 || n_bdy < 0 || row0 < 0 || nrows < 0 || row0 + nrows > M || ncols < 0 || ncols > M || ld < ncols)
        return fail(SCASML_ERR_ARG, "gp_gram_da_rows: bad sizes");
    if (((int64_t)n_dom + n_bdy + 63) / 64 > 65535)
        return fail(SCASML_ERR_UNSUPPORTED, "gp_gram_da_rows: too many collocation points for one launch");
    if (((int64_t)nrows + 63) / 64 > 65535) return fail(SCASML_ERR_UNSUPPORTED, "gp_gram_da_rows: too many rows per call");
    if (nrows == 0 || ncols == 0) return 0;
    const int rc = launch_gram_rows<kGramKa>("gp_gram_da_rows", {d, x_dom, n_dom, x_bdy, n_bdy}, a, row0, nrows, ncols, out, ld, (hipStream_t)stream);
    return rc ? rc : check_launch("gp_gram_da_rows launch");
}

extern "C" int64_t scasml_gp_loo_da_doubles(int32_t n_dom, int32_t n_bdy, int32_t panel_rows) {
    if (n_dom < 1 || n_bdy < 0 || panel_rows < 0 || panel_rows % kLooTile) return 0;
    const int64_t M = 4 * (int64_t)n_dom + n_bdy;
    return loo_panel_rows(M, panel_rows) * M + (M + kLooTile - 1) / kLooTile * M;      // the panel, then partials[column tile][row]
}

extern "C" int scasml_gp_loo_da(int32_t d, double a, const float *x_dom, int32_t n_dom, const float *x_bdy, int32_t n_bdy, const double *A, int64_t lda,
                                const double *alpha, int32_t panel_rows, double *q_out, double *v_out, double *work, void *stream) {
    if (!x_dom || !A || !alpha || !q_out || !v_out || !work || (n_bdy > 0 && !x_bdy)) return fail(SCASML_ERR_ARG, "gp_loo_da: null argument");
    const int64_t M = 4 * (int64_t)n_dom + n_bdy;
    if (d < 1 || n_dom < 1 || n_bdy < 0 || lda < M) return fail(SCASML_ERR_ARG, "gp_loo_da: bad sizes");
    if (panel_rows < 0 || panel_rows % kLooTile)
        return fail(SCASML_ERR_ARG, "gp_loo_da: panel_rows=%d is not a non-negative multiple of %d", (int)panel_rows, kLooTile);
    if (((int64_t)n_dom + n_bdy + 63) / 64 > 65535)
        return fail(SCASML_ERR_UNSUPPORTED, "gp_loo_da: too many collocation points for one launch");
    const int64_t pr = loo_panel_rows(M, panel_rows);
    if (pr / kLooTile > 65535) return fail(SCASML_ERR_UNSUPPORTED, "gp_loo_da: panel_rows=%d is more than one launch takes", (int)panel_rows);
    hipStream_t s = (hipStream_t)stream;
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(gp_loo_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)tile_lds_bytes<2>()) !=
        hipSuccess)
        return fail(SCASML_ERR_HIP, "gp_loo_da: cannot reserve LDS");
    const int64_t nct = (M + kLooTile - 1) / kLooTile;               // <= 4 * 65535: the row blocks ride on grid.x
    double *panel = work, *partials = work + pr * M;
    for (int64_t row0 = 0; row0 < M; row0 += pr) {
        const int nrows = (int)(M - row0 < pr ? M - row0 : pr);
        const int rc = launch_gram_rows<kGramKa>("gp_gram_da_rows", {d, x_dom, n_dom, x_bdy, n_bdy}, a, row0, nrows, M, panel, M, s);
        if (rc) return rc;
        hipLaunchKernelGGL(gp_loo_panel_gemv_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(kLooThreads), 0, s, panel, M, nrows, M, alpha, v_out + row0);
        hipLaunchKernelGGL(gp_loo_tile_kernel, dim3((unsigned)nct, (unsigned)((nrows + kLooTile - 1) / kLooTile)), dim3(kLooThreads), tile_lds_bytes<2>(), s,
                           A, lda, M, panel, M, row0, nrows, partials);
    }
    hipLaunchKernelGGL(gp_loo_sum_kernel, dim3((unsigned)((M + kLooThreads - 1) / kLooThreads)), dim3(kLooThreads), 0, s, partials, M, nct, q_out);
    return check_launch("gp_loo_da launch");
}
