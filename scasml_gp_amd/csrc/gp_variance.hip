// Posterior variance of the GP surrogate:  var(x_i) = prior - |L^-1 k(x_i)|^2  for n feature rows k(x_i) = K(x_i, phi) against the lower Cholesky
// factor L of K(phi, phi) + nugget I (models/GP.py keeps only right_vector and has no counterpart; the factor is the one scasml_cholesky leaves).
// One launch: rows <- rows L^-T in place, the sum of squares of every solved row in the same kernel, no second n x M buffer.
//
// Points are independent, so ONE workgroup (4 waves) owns a tile of 64 point rows and sweeps the block columns of L left to right by itself, 64
// columns at a time.  For block column J (columns j0 .. j0 + 63):
//   1. acc = sum_{k < j0} X[:, k] L[j0 + c][k]   on v_mfma_f64_16x16x4_f64 -- the 64 x 64 tile of dist_linalg.hip's gemm_nt_sub_kernel<2> (each wave
//      2 x 2 MFMA tiles, K streamed through LDS 32 columns at a time, register-staged double buffer); the A operand is the workgroup's OWN earlier
//      result, read back from `rows`, the B operand the rows j0 .. j0 + 63 of L;
//   2. C = R_J - acc goes to LDS with the diagonal block L_JJ; the 64 x 64 triangular solve X_J L_JJ^T = C runs as two 32-column substitutions
//      (one thread per point row, the row in registers) around one 64 x 32 x 32 MFMA update out of LDS;
//   3. the row's thread adds x^2 column by column to the sum it carries in a register; X_J is written back over R_J (later block columns read it;
//      the workgroup's own stores are made visible to its own later loads by an agent-scope fence and a barrier).
// No inter-workgroup synchronisation and no atomics.  Every point row's arithmetic -- the order of every sum -- is fixed by Mp alone: it does not
// depend on n, on the row's place in its tile or on the other rows of the tile (an MFMA output row is a function of its own A row and of B).  Rows
// beyond n in the last tile re-read the last valid row and are never stored.  Mp a multiple of 32: the last block column may be 32 wide (its upper
// half is run against an identity block and dropped).
// Work: n Mp^2 flop.  Traffic: every workgroup reads the lower triangle of L once (all workgroups walk it in the same order: HBM once, then L2 /
// Infinity Cache) and its own earlier block columns once per later block column, n Mp^2 / 16 bytes in all.
#include "common.hpp"

namespace scasml {

typedef double var_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kVarRows = 64, kVarCols = 64, kVarNB = 32, kVarThreads = 256;
constexpr int kVarLDP = kVarNB + 2;      // padded leading dimension of an operand stage (gp_train.hip, dist_linalg.hip)
constexpr int kVarLDC = kVarCols + 1;    // ... of the solve's C tile and diagonal block
// the operand stages (2 operands x 2 buffers x 64 x 34) and, after them in time, the solve's two 64 x 65 tiles share one allocation
constexpr size_t kVarLdsDoubles = (size_t)2 * 2 * kVarRows * kVarLDP > (size_t)2 * kVarRows * kVarLDC ? (size_t)2 * 2 * kVarRows * kVarLDP : (size_t)2 * kVarRows * kVarLDC;
constexpr size_t kVarLdsBytes = kVarLdsDoubles * sizeof(double);

// x Lk^T = rhs for one point row: 32 columns of Cs[r][c0 ..] against the lower-triangular 32 x 32 block at Ld[c0][c0]; returns the row's sum of
// squares over these columns, added in column order to `ssq`
__device__ __forceinline__ double var_solve32(double (*Cs)[kVarLDC], const double (*Ld)[kVarLDC], int r, int c0, double ssq) {
    double x[kVarNB];
#pragma unroll
    for (int j = 0; j < kVarNB; ++j) x[j] = Cs[r][c0 + j];
#pragma unroll
    for (int j = 0; j < kVarNB; ++j) {
        double v = x[j];
#pragma unroll
        for (int p = 0; p < j; ++p) v = fma(-x[p], Ld[c0 + j][c0 + p], v);
        x[j] = v / Ld[c0 + j][c0 + j];
        ssq = fma(x[j], x[j], ssq);
    }
#pragma unroll
    for (int j = 0; j < kVarNB; ++j) Cs[r][c0 + j] = x[j];
    return ssq;
}

__global__ __launch_bounds__(kVarThreads) void gp_variance_kernel(const double *__restrict__ L, int64_t Mp, double *rows, int64_t ld, int64_t n, double prior,
                                                                  double *__restrict__ var_out) {
    constexpr int PER = kVarRows * kVarNB / kVarThreads;   // doubles of one operand stage per thread
    extern __shared__ __attribute__((aligned(16))) double smem[];
    double (*Pa)[kVarRows][kVarLDP] = reinterpret_cast<double (*)[kVarRows][kVarLDP]>(smem);
    double (*Pb)[kVarCols][kVarLDP] = reinterpret_cast<double (*)[kVarCols][kVarLDP]>(smem + 2 * kVarRows * kVarLDP);
    double (*Cs)[kVarLDC] = reinterpret_cast<double (*)[kVarLDC]>(smem);
    double (*Ld)[kVarLDC] = reinterpret_cast<double (*)[kVarLDC]>(smem + kVarRows * kVarLDC);
    const int64_t r0 = (int64_t)blockIdx.x * kVarRows;
    const int valid = (int)(n - r0 < kVarRows ? n - r0 : kVarRows);   // >= 1: the grid covers n
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = (wv >> 1) * 32, wc = (wv & 1) * 32;
    const int l15 = lane & 15, l4 = lane >> 4;
    double *X = rows + r0 * ld;
    double ssq = 0.0;                                      // wave 0: lane r carries point row r's sum of squares
    // this thread's share of an operand stage: element e is (row tid / 32 + 8 e, column scol) of the 64 x 32 stage; rows beyond the tile's valid
    // ones re-read the last valid row (their products land in output rows that are never stored)
    const int scol = tid % kVarNB;
    int64_t xoff[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int rr = (tid + e * kVarThreads) / kVarNB;
        xoff[e] = (int64_t)(rr < valid ? rr : valid - 1) * ld + scol;
    }
    for (int64_t j0 = 0; j0 < Mp; j0 += kVarCols) {
        const int cw = (int)(Mp - j0 < kVarCols ? Mp - j0 : kVarCols);   // 64, or 32 in the last block column
        var_f64x4 acc[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = (var_f64x4){0.0, 0.0, 0.0, 0.0};
        if (j0 > 0) {
            double ra[PER], rb[PER];
            auto fetch = [&](int64_t kk) {
#pragma unroll
                for (int e = 0; e < PER; ++e) {
                    const int rr = (tid + e * kVarThreads) / kVarNB;
                    ra[e] = X[xoff[e] + kk];
                    rb[e] = rr < cw ? L[(j0 + rr) * Mp + kk + scol] : 0.0;
                }
            };
            auto park = [&](int buf) {
#pragma unroll
                for (int e = 0; e < PER; ++e) {
                    const int rr = (tid + e * kVarThreads) / kVarNB;
                    Pa[buf][rr][scol] = ra[e];
                    Pb[buf][rr][scol] = rb[e];
                }
            };
            auto accumulate = [&](int cur) {
#pragma unroll
                for (int k0 = 0; k0 < kVarNB; k0 += 4) {
                    double av[2], bv[2];
#pragma unroll
                    for (int i = 0; i < 2; ++i) av[i] = Pa[cur][wr + 16 * i + l15][k0 + l4];
#pragma unroll
                    for (int j = 0; j < 2; ++j) bv[j] = Pb[cur][wc + 16 * j + l15][k0 + l4];
#pragma unroll
                    for (int i = 0; i < 2; ++i)
#pragma unroll
                        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[i], bv[j], acc[i][j], 0, 0, 0);
                }
            };
            fetch(0);
            park(0);
            __syncthreads();
            int cur = 0;
            for (int64_t kk = kVarNB; kk < j0; kk += kVarNB) {
                fetch(kk);
                accumulate(cur);
                park(cur ^ 1);
                __syncthreads();
                cur ^= 1;
            }
            accumulate(cur);
            __syncthreads();                               // the stages are dead: the solve's tiles take their place
        }
        // C = R_J - acc in the MFMA's output layout (register e of lane (l4, l15) is row l4 + 4 e, column l15), and the diagonal block
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int r = wr + 16 * i + l4 + 4 * e, c = wc + 16 * j + l15;
                    const double rin = c < cw ? X[(int64_t)(r < valid ? r : valid - 1) * ld + j0 + c] : 0.0;
                    Cs[r][c] = rin - acc[i][j][e];
                }
        for (int idx = tid; idx < kVarCols * kVarCols; idx += kVarThreads) {
            const int r = idx / kVarCols, c = idx % kVarCols;
            Ld[r][c] = (r < cw && c < cw) ? L[(j0 + r) * Mp + j0 + c] : (r == c ? 1.0 : 0.0);
        }
        __syncthreads();
        if (wv == 0) ssq = var_solve32(Cs, Ld, lane, 0, ssq);
        if (cw > kVarNB) {                                 // block-uniform
            __syncthreads();
            // Cs[:, 32 .. 63] -= Cs[:, 0 .. 31] Ld[32 .. 63][0 .. 31]^T: wave w takes point rows 16 w .. 16 w + 15, both column tiles
            var_f64x4 upd[2];
#pragma unroll
            for (int j = 0; j < 2; ++j) upd[j] = (var_f64x4){0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int k0 = 0; k0 < kVarNB; k0 += 4) {
                const double av = Cs[16 * wv + l15][k0 + l4];
#pragma unroll
                for (int j = 0; j < 2; ++j) upd[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, Ld[kVarNB + 16 * j + l15][k0 + l4], upd[j], 0, 0, 0);
            }
#pragma unroll
            for (int j = 0; j < 2; ++j)
#pragma unroll
                for (int e = 0; e < 4; ++e) Cs[16 * wv + l4 + 4 * e][kVarNB + 16 * j + l15] -= upd[j][e];   // one writer per element, columns nobody reads here
            __syncthreads();
            if (wv == 0) ssq = var_solve32(Cs, Ld, lane, kVarNB, ssq);
        }
        __syncthreads();
        for (int idx = tid; idx < kVarRows * kVarCols; idx += kVarThreads) {
            const int r = idx / kVarCols, c = idx % kVarCols;
            if (r < valid && c < cw) X[(int64_t)r * ld + j0 + c] = Cs[r][c];
        }
        // the next block columns read these values back through the vector L1, which may still hold R_J: write back, invalidate, meet
        __threadfence();
        __syncthreads();
    }
    if (wv == 0 && lane < valid) var_out[r0 + lane] = prior - ssq;
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
