// Posterior variance of the GP surrogate:  var(x_i) = prior - |L^-1 k(x_i)|^2  for n feature rows k(x_i) = K(x_i, phi) against the lower Cholesky
// factor L of K(phi, phi) + nugget I (models/GP.py keeps only right_vector and has no counterpart; the factor is the one scasml_cholesky leaves).
// One launch: rows <- rows L^-T in place, the sum of squares of every solved row in the same kernel, no second n x M buffer.  The kernel is the
// OPS = 1 instantiation of the variance tile (gp_variance_tile.hpp: the sweep over the block columns of L, the substitutions, the sums, what is bit
// for bit a function of what); a workgroup owns 64 point rows, and lane r of wave 0 ends with point row r's sum of squares.
#include "gp_variance_tile.hpp"

namespace scasml {

__global__ __launch_bounds__(kVarThreads) void gp_variance_kernel(const double *__restrict__ L, int64_t Mp, double *rows, int64_t ld, int64_t n, double prior,
                                                                  double *__restrict__ var_out) {
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double ssq[1];
    gp_variance_tile<1>(L, Mp, rows, ld, n, smem, ssq);
    const int64_t r = (int64_t)blockIdx.x * kVarRows + threadIdx.x;
    if (threadIdx.x < kVarRows && r < n) var_out[r] = prior - ssq[0];
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_gp_variance(const double *L, int64_t Mp, double *rows, int64_t ld, int64_t n, double prior, double *var_out, void *stream) {
    if (!L || !rows || !var_out || Mp < 1 || n < 0 || ld < Mp) return fail(SCASML_ERR_ARG, "gp_variance: bad argument");
    if (Mp % kVarNB) return fail(SCASML_ERR_UNSUPPORTED, "gp_variance: Mp=%lld is not a multiple of %d", (long long)Mp, kVarNB);
    if (n == 0) return 0;
    const int64_t blocks = (n + kVarRows - 1) / kVarRows;
    if (blocks > 0x7fffffffLL) return fail(SCASML_ERR_UNSUPPORTED, "gp_variance: too many rows for one launch");
    if (hipFuncSetAttribute(reinterpret_cast<const void *>(gp_variance_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kVarLdsBytes) != hipSuccess)
        return fail(SCASML_ERR_HIP, "gp_variance: cannot reserve %zu bytes of LDS", kVarLdsBytes);
    hipLaunchKernelGGL(gp_variance_kernel, dim3((unsigned)blocks), dim3(kVarThreads), kVarLdsBytes, (hipStream_t)stream, L, Mp, rows, ld, n, prior, var_out);
    return check_launch("gp_variance launch");
}
