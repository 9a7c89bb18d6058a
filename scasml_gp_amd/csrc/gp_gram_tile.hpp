// The Gram pair tile: the geometry of a 64 x 64 tile of collocation pairs on the FP64 matrix cores, shared by everything that walks K(phi, phi) or
// K_a = dK/da pair by pair -- the full Gram and its feature rows (gp_train.hip), the contraction of K_a (gp_evidence.hip) and the rows of K_a
// (gp_loo.hip).  The only O(N^2 d) part of a pair's 16 entries is x_i . y_j, so the tile is ONE tile of the GEMM X Y^T (v_mfma_f64_16x16x4_f64,
// K = d + 1 streamed through LDS by mfma_tile_k_loop) and the rest is per pair:  |x - y|^2 = |x|^2 + |y|^2 - 2 x.y,  r_t = t_x - t_y,
// S = sum x - sum y  from per-point statistics computed once per tile into LDS.  A kernel is its tile origin, its early exit and a `visit` that
// turns a pair's geometry into entries (gp_gram_table.hpp) and stores or sums them.  float64 throughout: the reference factors K in x64
// (models/GP.py:258) and the norm expansion loses ~1e-15 of r^2.
//
// The results of the four kernels are compared bit for bit (rows of K against K, rows of K_a against K_a, K against its transpose): what a pair's
// geometry is -- the statistics' summation order, the zero fill of the K loop, the clamp -- is stated here and nowhere else.
#pragma once
#include "common.hpp"
#include "f64_mfma_tile.hpp"
#include "gp_gram_table.hpp"

namespace scasml {

constexpr int kGramTile = 64;                                 // collocation points per tile side: (NT, WS) = (2, 2) of f64_mfma_tile.hpp
constexpr int kGramThreads = 256;                             // four waves, each a 32 x 32 quadrant
constexpr int kGramPer = kGramTile * NB / kGramThreads;       // doubles of one operand chunk per thread
constexpr size_t kGramLdsBytes = tile_lds_bytes<2>();         // dynamic LDS of a launch: the operand panels of the K loop

// The collocation set: n_dom domain points, then n_bdy boundary points, rows of d + 1 floats (x, t).  Feature order of K (models/GP.py:251-258):
// [u(dom), u(bdy), Lap(dom), dt(dom), div(dom)]; ops: 0 = I, 1 = Lap, 2 = dt, 3 = div.
struct GramPoints {
    int d;
    const float *x_dom;
    int n_dom;
    const float *x_bdy;
    int n_bdy;
    SCASML_HD int N() const { return n_dom + n_bdy; }
    SCASML_HD const float *row(int p) const { return p < n_dom ? x_dom + (int64_t)p * (d + 1) : x_bdy + (int64_t)(p - n_dom) * (d + 1); }
    SCASML_HD int nops(int p) const { return p < n_dom ? 4 : 1; }          // a boundary point carries u alone
    SCASML_HD int64_t feature(int op, int p) const { return op == 0 ? p : (int64_t)N() + (int64_t)(op - 1) * n_dom + p; }
};

// The tile of the points [i0, i0 + 64) below i_end against the points [j0, j0 + 64) below N.  smem: kGramLdsBytes of dynamic LDS; stat: the
// kernel's own __shared__ array, (|x|^2 with t, sum of the spatial coordinates, t) of the tile's 64 + 64 points.  Every thread of the workgroup
// must call it.  visit(i, j, il, jl, r2, rt, S) is called for each live pair of this thread -- il, jl the tile-local indices, r2 clamped at 0 --
// in the order column tile, row tile, fragment register (the contraction's reduction order is stated in these terms).
// A visit that stores captures by value: through references the stores might alias what it captured, and the pair-invariant products of the
// table were then evaluated per pair (half again as many multiplications in the rows of K_a).
template <class Visit>
__device__ __forceinline__ void gram_pair_tile(const GramPoints &pts, int i0, int i_end, int j0, double *smem, double (*stat)[4], Visit visit) {
    constexpr int NT = 2;
    const int N = pts.N(), d = pts.d;
    {   // two threads per point, even / odd coordinates, combined with one shuffle
        const int q = threadIdx.x >> 1, par = threadIdx.x & 1;
        const int p = q < kGramTile ? i0 + q : j0 + q - kGramTile;
        double n = 0.0, sx = 0.0, tt = 0.0;
        if (p < (q < kGramTile ? i_end : N)) {
            const float *x = pts.row(p);
            for (int k = par; k < d; k += 2) {
                const double v = (double)x[k];
                n = fma(v, v, n);
                sx += v;
            }
            tt = (double)x[d];
        }
        n += __shfl_xor(n, 1);
        sx += __shfl_xor(sx, 1);
        if (par == 0) {
            stat[q][0] = fma(tt, tt, n);
            stat[q][1] = sx;
            stat[q][2] = tt;
        }
    }   // visible to everyone after the barriers of the K loop below
    TileAcc<NT> t;
    mfma_tile_zero(t);
    const int64_t kend = ((int64_t)d + 1 + NB - 1) / NB * NB;
    mfma_tile_k_loop<NT>(smem, 0, kend, [&](int64_t kk, double (&ra)[kGramPer], double (&rb)[kGramPer]) {
#pragma unroll
        for (int e = 0; e < kGramPer; ++e) {
            const int idx = threadIdx.x + e * kGramThreads, rr = idx / NB, cc = idx % NB;
            const int k = (int)kk + cc;
            ra[e] = (i0 + rr < i_end && k <= d) ? (double)pts.row(i0 + rr)[k] : 0.0;
            rb[e] = (j0 + rr < N && k <= d) ? (double)pts.row(j0 + rr)[k] : 0.0;
        }
    }, [] {}, t);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = (wv >> 1) * (16 * NT), wc = (wv & 1) * (16 * NT);
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
        const int jl = wc + 16 * jt + l15, j = j0 + jl;
        if (j >= N) continue;
        const double nj = stat[kGramTile + jl][0], sj = stat[kGramTile + jl][1], tj = stat[kGramTile + jl][2];
#pragma unroll
        for (int it = 0; it < NT; ++it)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int il = wr + 16 * it + l4 + 4 * e, i = i0 + il;
                if (i >= i_end) continue;
                const double ni = stat[il][0], si = stat[il][1], ti = stat[il][2];
                double r2 = fma(-2.0, t.v[it][jt][e], ni + nj);
                r2 = r2 < 0.0 ? 0.0 : r2;
                visit(i, j, il, jl, r2, ti - tj, si - sj);
            }
    }
}

// ---- feature rows of K or K_a (scasml_gp_gram_rows, scasml_gp_gram_da_rows, the panels of scasml_gp_loo_da) -----------------------------------
// The rows of ONE operator OX at the points [i_lo, i_lo + n_i) against every collocation point j: each pair writes its 1 or 4 entries of that row,
// columns < ncols only (the distributed factor stores the lower triangle).  out points at the first of those rows; tiles whose smallest column (the
// u column of their first point) is already >= ncols have nothing to write.  OX is a template argument so that the row of the table is picked at
// compile time (indexed at run time the 4 x 4 table of K_a went to scratch memory).
template <GramTable T, int OX>
__global__ __launch_bounds__(kGramThreads) void gp_gram_rows_kernel(GramPoints pts, double a, int i_lo, int n_i, int64_t ncols, double *out, int64_t ld) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    __shared__ double stat[2 * kGramTile][4];
    const int i0 = i_lo + blockIdx.y * kGramTile, j0 = blockIdx.x * kGramTile;
    if ((int64_t)j0 >= ncols) return;             // block-uniform: every column of this tile lies beyond the asked part of these rows
    const double fd = (double)pts.d;
    gram_pair_tile(pts, i0, i_lo + n_i, j0, smem, stat, [=](int i, int j, int, int, double r2, double rt, double S) {
        double k[4][4];
        gram_pair<T>(a, fd, r2, rt, S, k);
        double *orow = out + (int64_t)(i - i_lo) * ld;
        const int nops_j = pts.nops(j);
#pragma unroll
        for (int oy = 0; oy < 4; ++oy) {
            if (oy >= nops_j) continue;
            const int64_t col = pts.feature(oy, j);
            if (col < ncols) orow[col] = k[OX][oy];
        }
    });
}

// The feature rows [row0, row0 + nrows) x columns [0, ncols) of table T into out: one launch per operator segment of the row range.  The caller
// has checked the arguments; `who` prefixes the two refusals left (their texts are the entry points').
template <GramTable T>
static int launch_gram_rows(const char *who, const GramPoints &pts, double a, int64_t row0, int32_t nrows, int64_t ncols, double *out, int64_t ld,
                            hipStream_t stream) {
    const unsigned gx = (unsigned)((pts.N() + kGramTile - 1) / kGramTile);
    return for_each_operator_segment(pts.n_dom, pts.n_bdy, row0, nrows, [&](int ox, int i_lo, int n_i, int64_t row_offset) {
        const unsigned gy = (unsigned)((n_i + kGramTile - 1) / kGramTile);
        if (gy > 65535) return fail(SCASML_ERR_UNSUPPORTED, "%s: too many rows per call", who);
        auto kern = ox == 0 ? gp_gram_rows_kernel<T, 0> : ox == 1 ? gp_gram_rows_kernel<T, 1> : ox == 2 ? gp_gram_rows_kernel<T, 2> : gp_gram_rows_kernel<T, 3>;
        if (hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kGramLdsBytes) != hipSuccess)
            return fail(SCASML_ERR_HIP, "%s: cannot reserve LDS", who);
        hipLaunchKernelGGL(kern, dim3(gx, gy), dim3(kGramThreads), kGramLdsBytes, stream, pts, a, i_lo, n_i, ncols, out + row_offset * ld, ld);
        return 0;
    });
}

}  // namespace scasml
