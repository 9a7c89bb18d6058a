// The FP64 matrix-core tile: accumulators, the LDS operand panels and the double-buffered K loop.  Its users: gp_train.hip (Cholesky and
// triangular-solve updates), gp_gram_tile.hpp (the Gram pair tile of gp_train.hip, gp_evidence.hip and gp_loo.hip), gp_loo.hip (A K_a) and
// gp_rff.hip and gp_rff_grad.hip (x . omega).  gp_variance.hip keeps a K loop of its own over the same LDS layout: on this one it measured 0.3 % slower.
//
// ---- C(TB x TB) += A(TB x K) * B(K x TB) on the FP64 matrix cores ------------------------------------
// v_mfma_f64_16x16x4_f64: lane l supplies A[row = l&15][k = l>>4] and B[k = l>>4][col = l&15]; the four
// results of a lane are C[row = (l>>4) + 4*i][col = l&15], i = 0..3 (cdna_hip_programming.md section 3: the
// f64 C/D map differs from the f32 one).  Four waves per workgroup, each owning a quadrant of NT x NT MFMA tiles:
// NT = 2 -> 64 x 64 output tile (the one in use: the K = 256 updates of large matrices are L2-bandwidth-bound at
// 6.4 flop/B with it, 32 TFLOP/s; NT = 4 -> 128 x 128 doubles the flops per operand byte but needs 438 VGPRs, one wave
// per SIMD, and measured 23 TFLOP/s).  Operands come from LDS panels
// [TB][LDP] (A rows / B^T rows), double-buffered: the global loads of chunk k+1 are in flight while chunk k feeds
// the matrix cores.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace scasml {

constexpr int NB = 32;
typedef double f64x4 __attribute__((ext_vector_type(4)));
constexpr int LDP = NB + 2;      // padded leading dimension: 2 (row LDP + k) mod 64 is distinct over a ds_read_b64 group (16 rows x 2 k)

template <int NT>
struct TileAcc {
    f64x4 v[NT][NT];
};
// WS = waves per tile side: a workgroup is WS x WS waves (64 WS^2 threads), each owning NT x NT MFMA tiles of 16 x 16, i.e. an
// output tile of (16 NT WS)^2.  (NT, WS) = (2, 2): 64 x 64, 4 waves, 8 flop per operand byte; (2, 4): 128 x 128, 16 waves --
// the same registers per wave, half the operand traffic per flop and four waves per SIMD to hide it (139 KB of LDS: one
// workgroup per CU).  The large trailing updates use (2, 4), everything small (2, 2).
template <int NT, int WS = 2>
constexpr size_t tile_lds_bytes() { return (size_t)2 * 2 * (16 * NT * WS) * LDP * sizeof(double); }   // 2 operands x 2 buffers

template <int NT>
__device__ __forceinline__ void mfma_tile_zero(TileAcc<NT> &t) {
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) t.v[i][j] = (f64x4){0.0, 0.0, 0.0, 0.0};
}

// t += As (TB x NB) * Bt (TB x NB)^T
template <int NT, int WS = 2>
__device__ __forceinline__ void mfma_tile_accumulate(const double (*As)[LDP], const double (*Bt)[LDP], TileAcc<NT> &t) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int wr = (wv / WS) * (16 * NT), wc = (wv % WS) * (16 * NT);   // this wave's origin inside the tile
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int k0 = 0; k0 < NB; k0 += 4) {
        double a[NT], b[NT];
#pragma unroll
        for (int i = 0; i < NT; ++i) a[i] = As[wr + 16 * i + l15][k0 + l4];
#pragma unroll
        for (int j = 0; j < NT; ++j) b[j] = Bt[wc + 16 * j + l15][k0 + l4];
#pragma unroll
        for (int i = 0; i < NT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) t.v[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[i], b[j], t.v[i][j], 0, 0, 0);
    }
}

// The K loop shared by the Cholesky and triangular-solve updates: `fetch(kk, ra, rb)` loads this thread's elements
// of the two operand chunks of columns [kk, kk + NB) into registers (element e of a thread is panel entry
// idx = tid + 256 e, row idx / NB, column idx % NB).
// Which chunk entry (tile row rr, chunk column cc) is a thread's element e: consecutive lanes walk the direction that is contiguous
// in memory -- chunk columns for a row-major panel, tile rows for an operand stored k-major (KMAJOR: entry (rr, cc) at P[cc * ld + rr];
// with the row-major mapping there every lane of a load touched a cache line of its own).
template <int TBX, int THREADS, bool KMAJOR>
__device__ __forceinline__ void chunk_entry(int e, int &rr, int &cc) {
    const int idx = threadIdx.x + e * THREADS;
    if (KMAJOR) {
        rr = idx % TBX;
        cc = idx / TBX;
    } else {
        rr = idx / NB;
        cc = idx % NB;
    }
}

template <int NT, int WS = 2, bool KMAJOR_A = false, bool KMAJOR_B = false, class Fetch, class PreTail>
__device__ __forceinline__ void mfma_tile_k_loop(double *smem, int64_t k_begin, int64_t k_end, Fetch fetch, PreTail pre_tail, TileAcc<NT> &t) {
    constexpr int TBX = 16 * NT * WS, THREADS = 64 * WS * WS, PER = TBX * NB / THREADS;
    double (*Pa)[TBX][LDP] = reinterpret_cast<double (*)[TBX][LDP]>(smem);
    double (*Pb)[TBX][LDP] = reinterpret_cast<double (*)[TBX][LDP]>(smem + 2 * TBX * LDP);
    double ra[PER], rb[PER];
    auto park = [&](int buf) {
#pragma unroll
        for (int e = 0; e < PER; ++e) {
            int rr, cc;
            chunk_entry<TBX, THREADS, KMAJOR_A>(e, rr, cc);
            Pa[buf][rr][cc] = ra[e];
            chunk_entry<TBX, THREADS, KMAJOR_B>(e, rr, cc);
            Pb[buf][rr][cc] = rb[e];
        }
    };
    fetch(k_begin, ra, rb);
    park(0);
    __syncthreads();
    int cur = 0;
    for (int64_t kk = k_begin; kk + NB < k_end; kk += NB) {
        fetch(kk + NB, ra, rb);
        mfma_tile_accumulate<NT, WS>(Pa[cur], Pb[cur], t);
        park(cur ^ 1);
        __syncthreads();
        cur ^= 1;
    }
    pre_tail();   // the caller's loads of the output tile: in flight under the last chunk
    mfma_tile_accumulate<NT, WS>(Pa[cur], Pb[cur], t);
}

}  // namespace scasml
