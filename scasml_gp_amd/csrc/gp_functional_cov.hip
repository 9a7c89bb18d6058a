// Posterior covariance of the four functionals [u, Lap u, dt u, div u] of the GP surrogate at a point:
//   cov(x_i)[o][p] = prior[o][p] - (L^-1 k_o(x_i)) . (L^-1 k_p(x_i)),   k_o(x_i) = K_o(x_i, phi) the op-o feature row of scasml_gp_cross_rows
// against the lower Cholesky factor L of K(phi, phi) + nugget I (models/GP.py keeps only right_vector and has no counterpart; compat=None only: the
// as-coded matrix is not the Gram of one kernel).  One launch: rows <- rows L^-T in place, the ten inner products of every point in the same kernel.
// The kernel is the OPS = 4 instantiation of the variance tile (gp_variance_tile.hpp): the 64 rows of a tile are 16 points x 4 operators, row 4 i + o
// the op-o row of point i, so in the substitution the four rows of a point sit in one lane quad of wave 0.  For every solved column k, in rising k,
// lane r adds fma(x_r[k], x_r[k], .) to its sum of squares and fma(x_r[k], x_q[k], .) for its three quad partners q = r ^ 1, r ^ 2, r ^ 3 (DPP
// quad_perm), each entry one chain started at 0.0.  Lane 4 i + o ends with row o of point i's block.  Entries (o, p) and (p, o) are the same chain with
// the factors of every fma swapped: the block is exactly symmetric.  Entry (o, o) and the solved rows are the bits scasml_gp_variance gives on the
// same 4 n rows.  No atomics, no scratch, the tile's LDS and nothing more.
#include "gp_variance_tile.hpp"

namespace scasml {

struct FunctionalPrior {
    double v[16];      // row-major 4 x 4
};

__global__ __launch_bounds__(kVarThreads) void gp_functional_covariance_kernel(const double *__restrict__ L, int64_t Mp, double *rows, int64_t ld, int64_t n_rows,
                                                                               FunctionalPrior prior, double *__restrict__ cov_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double sums[4];                                        // sums[q]: this lane's row against the row of lane ^ q
    gp_variance_tile<4>(L, Mp, rows, ld, n_rows, smem, sums);
    const int64_t r = (int64_t)blockIdx.x * kVarRows + threadIdx.x;     // row 4 i + o: row o of point i's block starts at cov_out[16 i + 4 o] = cov_out[4 r]
    if (threadIdx.x < kVarRows && r < n_rows) {
        const int o = (int)threadIdx.x & 3;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int p = o ^ q;
            double pr = prior.v[0];                        // prior[o][p] by selects: a lane-dependent index into the kernel argument would go through scratch
#pragma unroll
            for (int k = 1; k < 16; ++k) pr = (4 * o + p == k) ? prior.v[k] : pr;
            cov_out[4 * r + p] = pr - sums[q];
        }
    }
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_gp_functional_covariance(const double *L, int64_t Mp, double *rows, int64_t ld, int64_t n_points, const double *prior_h, double *cov_out,
                                               void *stream) {
    if (!L || !rows || !prior_h || !cov_out || Mp < 1 || n_points < 0 || ld < Mp) return fail(SCASML_ERR_ARG, "gp_functional_covariance: bad argument");
    if (Mp % kVarNB) return fail(SCASML_ERR_UNSUPPORTED, "gp_functional_covariance: Mp=%lld is not a multiple of %d", (long long)Mp, kVarNB);
    if (n_points == 0) return 0;
    constexpr int kPoints = kVarRows / 4;                  // points of one tile
    const int64_t blocks = (n_points + kPoints - 1) / kPoints;
    if (blocks > 0x7fffffffLL) return fail(SCASML_ERR_UNSUPPORTED, "gp_functional_covariance: too many points for one launch");
    FunctionalPrior prior;
    for (int k = 0; k < 16; ++k) prior.v[k] = prior_h[k];
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(gp_functional_covariance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVarLdsBytes) !=
        hipSuccess)
        return fail(SCASML_ERR_HIP, "gp_functional_covariance: cannot reserve %zu bytes of LDS", kVarLdsBytes);
    hipLaunchKernelGGL(gp_functional_covariance_kernel, dim3((unsigned)blocks), dim3(kVarThreads), kVarLdsBytes, (hipStream_t)stream, L, Mp, rows, ld,
                       4 * n_points, prior, cov_out);
    return check_launch("gp_functional_covariance launch");
}
