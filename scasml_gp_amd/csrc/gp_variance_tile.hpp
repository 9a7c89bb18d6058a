// The variance tile: rows <- rows L^-T in place for one tile of 64 feature rows against the lower Cholesky factor L of K(phi, phi) + nugget I, with the
// inner products of the solved rows taken in the same sweep.  Shared by the posterior variance (gp_variance.hip, OPS = 1: 64 point rows, each row's sum
// of squares) and the posterior covariance of the four functionals (gp_functional_cov.hip, OPS = 4: 16 points x 4 operator rows, each row's products
// with the three other rows of its point as well).  models/GP.py keeps only right_vector and has no counterpart; the factor is the one scasml_cholesky
// leaves.
//
// Rows are independent, so ONE workgroup (4 waves) owns a tile of 64 rows and sweeps the block columns of L left to right by itself, 64 columns at a
// time.  For block column J (columns j0 .. j0 + 63):
//   1. acc = sum_{k < j0} X[:, k] L[j0 + c][k]   on v_mfma_f64_16x16x4_f64 -- the 64 x 64 tile of dist_linalg.hip's gemm_nt_sub_kernel<2> (each wave
//      2 x 2 MFMA tiles, K streamed through LDS 32 columns at a time, register-staged double buffer); the A operand is the workgroup's OWN earlier
//      result, read back from `rows`, the B operand the rows j0 .. j0 + 63 of L;
//   2. C = R_J - acc goes to LDS with the diagonal block L_JJ; the 64 x 64 triangular solve X_J L_JJ^T = C runs as two 32-column substitutions
//      (one thread per row, the row in registers) around one 64 x 32 x 32 MFMA update out of LDS;
//   3. the row's thread adds x^2 column by column to the sum it carries in a register -- and, OPS = 4, x times the same column of each of its three
//      quad partners (a DPP quad_perm exchange, no LDS) to three more; X_J is written back over R_J (later block columns read it; the workgroup's own
//      stores are made visible to its own later loads by an agent-scope fence and a barrier).
// No inter-workgroup synchronisation and no atomics.  Every row's arithmetic -- the order of every sum -- is fixed by Mp alone: it does not depend on
// n, on the row's place in its tile or on the other rows of the tile (an MFMA output row is a function of its own A row and of B), and OPS adds sums
// without touching the solve: the solved rows and the sums of squares are the same bits for both.  Rows beyond n in the last tile re-read the last
// valid row and are never stored.  Mp a multiple of 32: the last block column may be 32 wide (its upper half is run against an identity block and
// dropped).
// Work: n Mp^2 flop.  Traffic: every workgroup reads the lower triangle of L once (all workgroups walk it in the same order: HBM once, then L2 /
// Infinity Cache) and its own earlier block columns once per later block column, n Mp^2 / 16 bytes in all.
#pragma once
#include "common.hpp"

namespace scasml {

typedef double var_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kVarRows = 64, kVarCols = 64, kVarNB = 32, kVarThreads = 256;
constexpr int kVarLDP = kVarNB + 2;      // padded leading dimension of an operand stage (gp_train.hip, dist_linalg.hip)
constexpr int kVarLDC = kVarCols + 1;    // ... of the solve's C tile and diagonal block
// the operand stages (2 operands x 2 buffers x 64 x 34) and, after them in time, the solve's two 64 x 65 tiles share one allocation
constexpr size_t kVarLdsDoubles = (size_t)2 * 2 * kVarRows * kVarLDP > (size_t)2 * kVarRows * kVarLDC ? (size_t)2 * 2 * kVarRows * kVarLDP : (size_t)2 * kVarRows * kVarLDC;
constexpr size_t kVarLdsBytes = kVarLdsDoubles * sizeof(double);

// the value lane (l ^ Q) of this lane's quad holds, Q in 1 .. 3: v_mov_b32 with a DPP quad_perm on each half of the double.  Every lane of the wave
// must be active.
template <int Q>
__device__ __forceinline__ double var_quad_xor(double v) {
    static_assert(Q >= 1 && Q <= 3, "a partner inside the lane quad");
    constexpr int ctrl = (0 ^ Q) | ((1 ^ Q) << 2) | ((2 ^ Q) << 4) | ((3 ^ Q) << 6);    // quad_perm:[0^Q, 1^Q, 2^Q, 3^Q]
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, ctrl, 0xf, 0xf, false), __builtin_amdgcn_update_dpp(0, lo, ctrl, 0xf, 0xf, false));
}

// x Lk^T = rhs for one row: 32 columns of Cs[r][c0 ..] against the lower-triangular 32 x 32 block at Ld[c0][c0].  Added in column order: the row's
// squares to sums[0] and, OPS = 4, its products with the same column of lane r ^ q's row to sums[q] (the whole wave calls it: lane r owns row r).
// Lanes r and r ^ q run one chain with the factors of every fma swapped: their two sums are the same bits.
template <int OPS>
__device__ __forceinline__ void var_solve32(double (*Cs)[kVarLDC], const double (*Ld)[kVarLDC], int r, int c0, double (&sums)[OPS]) {
    double x[kVarNB];
#pragma unroll
    for (int j = 0; j < kVarNB; ++j) x[j] = Cs[r][c0 + j];
#pragma unroll
    for (int j = 0; j < kVarNB; ++j) {
        double v = x[j];
#pragma unroll
        for (int p = 0; p < j; ++p) v = fma(-x[p], Ld[c0 + j][c0 + p], v);
        x[j] = v / Ld[c0 + j][c0 + j];
        sums[0] = fma(x[j], x[j], sums[0]);
        if constexpr (OPS == 4) {
            sums[1] = fma(x[j], var_quad_xor<1>(x[j]), sums[1]);
            sums[2] = fma(x[j], var_quad_xor<2>(x[j]), sums[2]);
            sums[3] = fma(x[j], var_quad_xor<3>(x[j]), sums[3]);
        }
    }
#pragma unroll
    for (int j = 0; j < kVarNB; ++j) Cs[r][c0 + j] = x[j];
}

// The tile of the rows [r0, r0 + 64) below n, r0 = 64 blockIdx.x: solved in place; on return lane r of wave 0 holds row r's sums (the other waves'
// are 0).  smem: kVarLdsBytes of dynamic LDS.  Every thread of the 256-thread workgroup must call it; the grid covers n.
template <int OPS>
__device__ __forceinline__ void gp_variance_tile(const double *__restrict__ L, int64_t Mp, double *rows, int64_t ld, int64_t n, double *smem, double (&sums)[OPS]) {
    static_assert(OPS == 1 || OPS == 4, "one row per point, or the four operator rows of a point in a lane quad");
    constexpr int PER = kVarRows * kVarNB / kVarThreads;   // doubles of one operand stage per thread
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
#pragma unroll
    for (int q = 0; q < OPS; ++q) sums[q] = 0.0;           // wave 0: lane r carries row r's sums
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
        if (wv == 0) var_solve32<OPS>(Cs, Ld, lane, 0, sums);
        if (cw > kVarNB) {                                 // block-uniform
            __syncthreads();
            // Cs[:, 32 .. 63] -= Cs[:, 0 .. 31] Ld[32 .. 63][0 .. 31]^T: wave w takes rows 16 w .. 16 w + 15, both column tiles
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
            if (wv == 0) var_solve32<OPS>(Cs, Ld, lane, kVarNB, sums);
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
}

}  // namespace scasml
