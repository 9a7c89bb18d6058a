// Draws from a joint Gaussian:  out[s][i] = mean[i] + sum_{j <= i} Lc[i][j] z(seed, sample0 + s, j)  for the lower Cholesky factor Lc of an n x n
// covariance (models/GP.py keeps only right_vector and has no counterpart; GP.sample_posterior factors predict_covariance with scasml_cholesky).
// The normals are never in HBM: z(seed, r, j) is component j % 4 of normal4(quad = j / 4, site = 0, root = r, stream = SCASML_STREAM_GP_SAMPLE,
// key = seed) (philox_normal.hpp; oracle.philox.normals(seed, stream, r, 0, n)[j]), widened to double.
//
// ONE workgroup (4 waves) owns a tile of 64 samples x 64 points and walks K = 0 .. end of the tile's diagonal block, 32 columns at a time, on
// v_mfma_f64_16x16x4_f64 -- the 64 x 64 register-staged double buffer of dist_linalg.hip's gemm_nt_sub_kernel<2> / gp_variance.hip (each wave 2 x 2
// MFMA tiles; the next stage is fetched into registers while the current one feeds the matrix cores).  The A operand (64 samples x 32 k) is
// GENERATED: thread t draws the quads t % 8 of sample rows t / 8 and t / 8 + 32 -- two Philox blocks per thread and stage -- and parks them in LDS
// as float (half the bytes: two workgroups per CU, so one's Philox arithmetic runs under the other's matrix work); they are widened on the way
// into the MFMA.  The B operand is the tile's 64 rows of Lc.  Tiles strictly above the diagonal are never visited (the K loop ends at the tile's
// own last column) and in the diagonal stages an entry with j > i is not even loaded: the upper triangle of Lc is not trusted to be zero.
// An MFMA output row (one sample) is a function of its own A row and of B; the A row is a function of (seed, sample index); the K range and order
// of point i are fixed by i and np.  So out[s][:] depends on (Lc, mean, seed, sample0 + s) alone, bit for bit: not on S, not on how a caller
// splits a run of samples over calls, not on the other samples of the tile.  No atomics, no inter-workgroup synchronisation, no scratch.
// Work: S n^2 flop (the lower triangle at MFMA granularity) and S n^2 / 128 Philox blocks (every point tile draws its sample tile's normals
// again -- the price of not storing them).  Traffic: every sample tile reads the lower triangle of Lc once (L2 / Infinity Cache after the first).
#include "common.hpp"
#include "philox_normal.hpp"

namespace scasml {

typedef double smp_f64x4 __attribute__((ext_vector_type(4)));
constexpr int kSmpTile = 64, kSmpNB = 32, kSmpThreads = 256;
constexpr int kSmpLDL = kSmpNB + 2;      // padded leading dimension of the Lc stage, in doubles (gp_variance.hip, dist_linalg.hip)
constexpr int kSmpLDZ = kSmpNB + 2;      // ... of the normal stage, in floats: 16 rows x 2 k of one ds_read_b32 half fall on 32 distinct banks
constexpr int kSmpPer = kSmpTile * kSmpNB / kSmpThreads;   // doubles of one Lc stage per thread

__global__ __launch_bounds__(kSmpThreads) void gp_sample_kernel(const double *__restrict__ Lc, int64_t np, int64_t n, const double *__restrict__ mean, uint32_t k0,
                                                               uint32_t k1, uint32_t root0, int64_t S, double *__restrict__ out, int64_t ld_out) {
    __shared__ __attribute__((aligned(16))) double Pl[2][kSmpTile][kSmpLDL];
    __shared__ __attribute__((aligned(16))) float Pz[2][kSmpTile][kSmpLDZ];
    normal_table_to_lds();
    const int64_t s0 = (int64_t)blockIdx.x * kSmpTile;
    const int64_t i0 = (int64_t)(gridDim.y - 1 - blockIdx.y) * kSmpTile;   // the longest K loops first
    const int64_t kend = i0 + kSmpTile < np ? i0 + kSmpTile : np;         // a multiple of 32, >= 32
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int wr = (wv >> 1) * 32, wc = (wv & 1) * 32;                     // this wave's samples (MFMA rows) and points (MFMA columns)
    const int l15 = lane & 15, l4 = lane >> 4;
    const int scol = tid % kSmpNB, srow = tid / kSmpNB;                    // Lc stage: element e is (row srow + 8 e, column scol)
    const int zq = tid & 7, zrow = tid >> 3;                               // normal stage: quad zq of sample rows zrow and zrow + 32
    smp_f64x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (smp_f64x4){0.0, 0.0, 0.0, 0.0};
    double rl[kSmpPer];
    float4 rz[2];
    auto fetch = [&](int64_t kk) {
#pragma unroll
        for (int e = 0; e < kSmpPer; ++e) {
            const int64_t i = i0 + srow + 8 * e, j = kk + scol;
            rl[e] = (i < np && j <= i) ? Lc[i * np + j] : 0.0;             // rows n .. np are the identity padding: computed, never stored
        }
#pragma unroll
        for (int e = 0; e < 2; ++e)   // samples beyond S draw too (their root index wraps at worst) and are never stored
            rz[e] = normal4((uint32_t)(kk / 4) + (uint32_t)zq, 0u, root0 + (uint32_t)(s0 + zrow + 32 * e), SCASML_STREAM_GP_SAMPLE, k0, k1);
    };
    auto park = [&](int buf) {
#pragma unroll
        for (int e = 0; e < kSmpPer; ++e) Pl[buf][srow + 8 * e][scol] = rl[e];
#pragma unroll
        for (int e = 0; e < 2; ++e) {                                      // rows are 136 bytes: 8-byte aligned halves
            float2 *p = reinterpret_cast<float2 *>(&Pz[buf][zrow + 32 * e][4 * zq]);
            p[0] = make_float2(rz[e].x, rz[e].y);
            p[1] = make_float2(rz[e].z, rz[e].w);
        }
    };
    auto accumulate = [&](int cur) {
#pragma unroll
        for (int kq = 0; kq < kSmpNB; kq += 4) {
            double av[2], bv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) av[i] = (double)Pz[cur][wr + 16 * i + l15][kq + l4];
#pragma unroll
            for (int j = 0; j < 2; ++j) bv[j] = Pl[cur][wc + 16 * j + l15][kq + l4];
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
    for (int64_t kk = kSmpNB; kk < kend; kk += kSmpNB) {
        fetch(kk);
        accumulate(cur);
        park(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    accumulate(cur);
    // register e of lane (l4, l15) is MFMA row l4 + 4 e (sample), column l15 (point): 16 consecutive doubles of one output row per lane group
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int64_t pt = i0 + wc + 16 * j + l15;
            const double mu = pt < n ? mean[pt] : 0.0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int64_t s = s0 + wr + 16 * i + l4 + 4 * e;
                if (s < S && pt < n) out[s * ld_out + pt] = mu + acc[i][j][e];
            }
        }
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_gp_sample(const double *Lc, int64_t np, int64_t n, const double *mean, uint64_t seed, int64_t sample0, int64_t S, double *out,
                                int64_t ld_out, void *stream) {
    if (!Lc || !mean || !out || n < 1 || n > np || ld_out < n || S < 0 || sample0 < 0) return fail(SCASML_ERR_ARG, "gp_sample: bad argument");
    if (np % kSmpNB) return fail(SCASML_ERR_UNSUPPORTED, "gp_sample: np=%lld is not a multiple of %d", (long long)np, kSmpNB);
    if (sample0 > (int64_t)1 << 32 || S > ((int64_t)1 << 32) - sample0)
        return fail(SCASML_ERR_UNSUPPORTED, "gp_sample: sample indices %lld .. %lld reach 2^32 (the Philox root word is 32 bits)", (long long)sample0,
                    (long long)sample0 + (long long)S - 1);
    if (S == 0) return 0;
    const int64_t gx = (S + kSmpTile - 1) / kSmpTile, gy = (n + kSmpTile - 1) / kSmpTile;
    if (gy > 65535) return fail(SCASML_ERR_UNSUPPORTED, "gp_sample: too many points for one launch");
    hipLaunchKernelGGL(gp_sample_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kSmpThreads), 0, (hipStream_t)stream, Lc, np, n, mean,
                       (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), (uint32_t)sample0, S, out, ld_out);
    return check_launch("gp_sample launch");
}
