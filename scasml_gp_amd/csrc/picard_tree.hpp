// Picard-tree walker (Walker), kernel template (picard_tree_kernel) and launch ladder (launch_tree: which instantiations exist, and the
// variant / mode / equation / level selection among them), shared by the translation units that instantiate them:
//   picard_tree.hip                                        the Philox stream, levels 1..5; the entry points' validation (picard_tree_run)
//   picard_tree_jax.hip / picard_tree_jax_deep.hip         the reference's own stream (SCASML_RNG_JAX_STREAM, compat_rng = "jax"), levels 1..3 / 4, 5
//   picard_tree_stderr.hip / picard_tree_stderr_deep.hip   the kernels that also estimate the standard error of u, levels 1..3 / 4, 5
//   picard_tree_stderr_uz.hip / picard_tree_stderr_uz_deep.hip   the kernels that estimate the standard errors of u and of every z_i
//                                                          (picard_se_uz_kernel: the same walker under its SEZ flag), levels 1..3 / 4, 5
//   picard_tree_summands.hip / picard_tree_summands_deep.hip     the kernels that store the root call's summands of u (picard_sum_kernel:
//   picard_tree_summands_uz.hip / picard_tree_summands_uz_deep.hip   the walker's SUM flavour) or of (u, z), levels 1..3 / 4, 5
//   picard_staged.hip                                      the staged walk (its own kernel; shares the lane helpers and the args filler below)
// Each of the first eleven holds ONE call of launch_tree, whose <JAX, SE, N_LO, N_HI, SEZ, SUM> decide what that unit compiles -- split so that the build
// compiles the instantiations in parallel (the JAX-stream kernels inline one Threefry + erf_inv per normal at every site of the unrolled tree).
#pragma once
#include <string.h>
#include "common.hpp"
#include "equations.hpp"
#include "philox_normal.hpp"

namespace scasml {

struct TreeArgs {
    scasml_plan plan;
    const float *x_t;
    float *points;
    const float4 *gpv;
    float *out_uz;
    float *out_uhat;
    int64_t B;
    int64_t Bs;   // site stride: row of (site, root) = site * Bs + root (>= B)
    int64_t ppr;  // points per root = plan.sites[n] + 1
    uint32_t k0, k1, stream, root0;
    int32_t rank, world;
    const uint8_t *owner;   // unit -> rank (scasml_plan_deal_units), or null: unit % world
    int32_t crn;  // SCASML_RNG_COMPAT_CRN: terminal draws keyed by the call's k = 0 position (reference key reuse, E-2/E-3)
    int32_t f16;  // SCASML_RNG_COMPAT_F16: the reference's solver-level float16 casts (g, f and every uz_solve return; E-5)
    const uint32_t *jk;   // SCASML_RNG_JAX_STREAM: key words [terminal k0 k1 | path sub-key 0 k0 k1 | sub-key 1 ...] (scasml_rng.jax_keys)
    int32_t d, G, logG, kp;
    float T, mu, sigma, clip;
    float *out_se;   // picard_tree_kernel<..., SE = true> only: B standard errors of the root call's u (scasml_picard_tree_stderr);
                     // picard_se_uz_kernel: B rows of 1 + d, the standard errors of (u, z_1 .. z_d) (scasml_picard_tree_stderr_uz)
};

__device__ __forceinline__ float4 f4(float v) { return make_float4(v, v, v, v); }
__device__ __forceinline__ float4 fma4(float s, float4 a, float4 b) {  // s*a + b
    return make_float4(fmaf(s, a.x, b.x), fmaf(s, a.y, b.y), fmaf(s, a.z, b.z), fmaf(s, a.w, b.w));
}
__device__ __forceinline__ float4 add4(float4 a, float s) { return make_float4(a.x + s, a.y + s, a.z + s, a.w + s); }
__device__ __forceinline__ float4 f4_scale(float4 a, float s) { return make_float4(a.x * s, a.y * s, a.z * s, a.w * s); }
__device__ __forceinline__ float4 mul4(float4 a, float4 b) { return make_float4(a.x * b.x, a.y * b.y, a.z * b.z, a.w * b.w); }
__device__ __forceinline__ float clip1(float v, float c) { return v < -c ? -c : (v > c ? c : v); }  // keeps NaN (jnp.clip)
__device__ __forceinline__ float4 clip4(float4 v, float c) { return make_float4(clip1(v.x, c), clip1(v.y, c), clip1(v.z, c), clip1(v.w, c)); }
// A NaN leaves through out_uz as ONE bit pattern.  Which sign a NaN carries that an operation produced or passed on is the compiler's choice (a
// negation folded into an operand flips it), so two kernels that run the same arithmetic may disagree on it, and the entries promise each other's
// out_uz bit for bit: picard_sum_kernel<0, ACCUMULATE, 5, cubic> returned +NaN in the z of a NaN root where picard_tree_kernel returns -NaN.
__device__ __forceinline__ float one_nan(float v) { return v != v ? __builtin_nanf("") : v; }
__device__ __forceinline__ float4 one_nan4(float4 v) { return make_float4(one_nan(v.x), one_nan(v.y), one_nan(v.z), one_nan(v.w)); }
// A lane holds spatial dims dim0 .. dim0 + 3 of every d-vector: 1 on those below d (live), 0 on padding
__device__ __forceinline__ float4 live_mask(int dim0, int d) {
    return make_float4(dim0 + 0 < d ? 1.0f : 0.0f, dim0 + 1 < d ? 1.0f : 0.0f, dim0 + 2 < d ? 1.0f : 0.0f, dim0 + 3 < d ? 1.0f : 0.0f);
}
// this lane's live dims of z into a root's out_uz row (u, z_1 .. z_d).  (u, which lane 0 of the group stores, stays with the callers: the
// tree kernel writes u_hat and the standard error between the two, and stores that may alias keep their order)
__device__ __forceinline__ void store_z(float *out, int dim0, int d, float4 z) {
    if (dim0 + 0 < d) out[1 + dim0 + 0] = z.x;
    if (dim0 + 1 < d) out[1 + dim0 + 1] = z.y;
    if (dim0 + 2 < d) out[1 + dim0 + 2] = z.z;
    if (dim0 + 3 < d) out[1 + dim0 + 3] = z.w;
}
__device__ __forceinline__ float r16(float v) { return (float)(_Float16)v; }                          // .astype(jnp.float16), RNE
// Hardware reciprocal / square root / exp2 (<= 1 ulp) for the arithmetic that is NOT part of the bit-exact
// RNG specification: the IEEE-correct expansions cost ~10 VALU instructions each and these kernels are
// VALU-bound; the parity tolerance (1e-4 relative) is five orders of magnitude above the difference.
__device__ __forceinline__ float rcp_fast(float v) { return __builtin_amdgcn_rcpf(v); }
__device__ __forceinline__ float sqrt_fast(float v) { return __builtin_amdgcn_sqrtf(v); }
__device__ __forceinline__ float exp_fast(float v) { return __builtin_amdgcn_exp2f(v * 1.44269504088896341f); }

// ACCUMULATE recovers the terminal normals as (X_T - x - drift) / vol.  X_T was rounded to binary32 when it was stored
// (|X_T| 2^-24 ~ 3e-8), so the recovered normal is off by ~3e-8 / vol and the z estimator, which divides by T - t, by
// ~g 1.2e-7 / (sqrt(T-t) (T-t) sqrt(mg)): 1e-4 g at T - t = 1.6e-3 but 0.03 g one fp16 ulp below T.  Below this
// volatility (sigma sqrt(T-t) < 1e-2, i.e. T - t < 1.6e-3 at sigma = 0.25) the normals are replayed instead.
constexpr float kReadbackMinVol = 1e-2f;
// Terminal samples whose rows ACCUMULATE requests ahead of the one it consumes.  Measured at the headline shape (same box,
// profiles/r02_accumulate_prefetch.txt): 1 -> 1.29 ms, 2 -> 1.30, 3 -> 1.65, 5 -> 1.66: beyond one the extra registers and
// moves cost more than the bytes in flight buy.
#ifndef SCASML_ACC_AHEAD
#define SCASML_ACC_AHEAD 1
#endif
constexpr int kAhead = SCASML_ACC_AHEAD;

// ---- SCASML_RNG_JAX_STREAM: the reference's own normals, jax.random.normal(key, shape, float16) under jax_threefry_partitionable,
// addressed by counter (oracle/jax_random.py is the NumPy statement; tests/test_gpu_jax_stream.py compares the two bit for bit):
// element with row-major index i of a draw under key (k0, k1) = low 16 bits of y0 ^ y1, (y0, y1) = Threefry-2x32-20(key, (i >> 32, i));
// bits >> 6 | 0x3C00 is a float16 in [1, 2); minus 1, times 2, plus nextafter(-1, 0), clamped below (each a float16 operation);
// sqrt(2) * erf_inv in float32 (XLA's ErfInv32) rounded to float16 before the float16 product.  One Threefry per normal: this is the
// parity mode, ~7x the integer work of the Philox stream.  The transform itself depends on ten bits only and is tabulated per workgroup.
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) { return (x << r) | (x >> (32 - r)); }
__device__ __forceinline__ uint32_t threefry_bits16(uint32_t k0, uint32_t k1, uint64_t index) {
    const uint32_t ks[3] = {k0, k1, k0 ^ k1 ^ 0x1BD11BDAu};
    uint32_t x0 = (uint32_t)(index >> 32) + ks[0], x1 = (uint32_t)index + ks[1];
    const int rot[2][4] = {{13, 15, 26, 6}, {17, 29, 16, 24}};
#pragma unroll
    for (int i = 0; i < 5; ++i) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            x0 += x1;
            x1 = rotl32(x1, rot[i & 1][j]) ^ x0;
        }
        x0 += ks[(i + 1) % 3];
        x1 += ks[(i + 2) % 3] + (uint32_t)(i + 1);
    }
    return (x0 ^ x1) & 0xFFFFu;
}
// the float16 transform of the draw's TEN live bits (the float16 uniform has a 10-bit mantissa): a function of 1024 inputs, which the tree kernels
// tabulate once per workgroup (jax_table_to_lds) instead of evaluating log1p, a square root and a polynomial per normal
__device__ __forceinline__ float jax_normal_of_bits10(uint32_t b10) {
    const unsigned short hb = (unsigned short)(b10 | 0x3C00u);
    const _Float16 lo = (_Float16)-0.99951171875f;                      // nextafter(float16(-1), 0)
    _Float16 u = __builtin_bit_cast(_Float16, hb) - (_Float16)1.0f;
    u = u * (_Float16)2.0f + lo;                                        // (1 - lo) rounds to 2 in float16; both operations are exact or rounded once
    u = u < lo ? lo : u;
    const float x = (float)u;
    float w = -log1pf(-x * x);
    float p;
    if (w < 5.0f) {
        w -= 2.5f;
        p = 2.81022636e-08f;
        p = fmaf(p, w, 3.43273939e-07f);
        p = fmaf(p, w, -3.5233877e-06f);
        p = fmaf(p, w, -4.39150654e-06f);
        p = fmaf(p, w, 0.00021858087f);
        p = fmaf(p, w, -0.00125372503f);
        p = fmaf(p, w, -0.00417768164f);
        p = fmaf(p, w, 0.246640727f);
        p = fmaf(p, w, 1.50140941f);
    } else {
        w = sqrtf(w) - 3.0f;
        p = -0.000200214257f;
        p = fmaf(p, w, 0.000100950558f);
        p = fmaf(p, w, 0.00134934322f);
        p = fmaf(p, w, -0.00367342844f);
        p = fmaf(p, w, 0.00573950773f);
        p = fmaf(p, w, -0.0076224613f);
        p = fmaf(p, w, 0.00943887047f);
        p = fmaf(p, w, 1.00167406f);
        p = fmaf(p, w, 2.83297682f);
    }
    const _Float16 e = (_Float16)(p * x);
    return (float)((_Float16)1.4140625f * e);                           // float16(sqrt(2)) * float16(erf_inv): a float16 product
}
constexpr int kJaxTableRows = 1024;
__device__ __forceinline__ float *jax_table_lds() {
    __shared__ float t[kJaxTableRows];
    return t;
}
// every thread of the workgroup, before any return: the 1024 possible normals of jax.random.normal(float16), 4 KB of LDS
__device__ __forceinline__ void jax_table_to_lds() {
    float *t = jax_table_lds();
    for (int i = threadIdx.x; i < kJaxTableRows; i += blockDim.x) t[i] = jax_normal_of_bits10((uint32_t)i);
    __syncthreads();
}
__device__ __forceinline__ float jax_normal_f16(uint32_t k0, uint32_t k1, uint64_t index) {
    return jax_table_lds()[threefry_bits16(k0, k1, index) >> 6];
}
// jax.random.uniform(key, shape, float16): one of the 1024 values k / 1024 (0 included)
__device__ __forceinline__ float jax_uniform_f16(uint32_t k0, uint32_t k1, uint64_t index) {
    const unsigned short hb = (unsigned short)((threefry_bits16(k0, k1, index) >> 6) | 0x3C00u);
    return (float)(__builtin_bit_cast(_Float16, hb) - (_Float16)1.0f);
}

// ACCUMULATE's read-ahead of terminal rows (kAhead samples); empty in the other modes
template <bool ON>
struct PrefetchQueue {
    float4 XT[kAhead], gp[kAhead];
};
template <>
struct PrefetchQueue<false> {};

// Monte-Carlo variance of the ROOT call's u (scasml_picard_tree_stderr, DESIGN.md "Standard errors"): the root sum is a sum of independent
// terms -- the terminal samples, then one term per level l < n -- and every term a sum of N i.i.d. summands Y_0 .. Y_{N-1} that the walk
// visits one after another.  A term accumulates the deviations from its FIRST summand, D_i = Y_i - Y_0 (S1 = sum D_i, S2 = sum D_i^2), and
// closes with N / (N - 1) (S2 - S1^2 / N): near t = T, where every sample of g coincides, a float32 sum of Y^2 would cancel to noise and
// this form gives exactly 0.  Every lane of a root's group holds the same Y (dim_sum is group-uniform): no shuffles.
template <bool ON>
struct SeTerm {
    float y0, s1, s2;
    __device__ __forceinline__ void begin() { y0 = s1 = s2 = 0.0f; }
    __device__ __forceinline__ void add(float y, bool first) {
        if (first) {
            y0 = y;
        } else {
            const float dv = y - y0;
            s1 += dv;
            s2 = fmaf(dv, dv, s2);
        }
    }
    // N >= 2 (the entry point refuses a term of one sample)
    __device__ __forceinline__ float close(int N) const {
        const float fn = (float)N;
        return (fn / (fn - 1.0f)) * fmaf(-s1 / fn, s1, s2);
    }
};
template <>
struct SeTerm<false> {};
template <bool ON>
struct SeState {
    float var;
};
template <>
struct SeState<false> {};
// The same estimate for z (scasml_picard_tree_stderr_uz), component by component: a summand is the float4 of this lane's four dims of what a
// sample adds to the root call's z, so every lane accumulates its own dims and again nothing is shuffled.  Padding dims are accumulated
// like the others (they may come to hold 0 * inf) and never stored.
template <bool ON>
struct SeTerm4 {
    float4 y0, s1, s2;
    __device__ __forceinline__ void begin() { y0 = s1 = s2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    __device__ __forceinline__ void add(float4 y, bool first) {
        if (first) {
            y0 = y;
        } else {
            const float4 dv = make_float4(y.x - y0.x, y.y - y0.y, y.z - y0.z, y.w - y0.w);
            s1 = make_float4(s1.x + dv.x, s1.y + dv.y, s1.z + dv.z, s1.w + dv.w);
            s2 = make_float4(fmaf(dv.x, dv.x, s2.x), fmaf(dv.y, dv.y, s2.y), fmaf(dv.z, dv.z, s2.z), fmaf(dv.w, dv.w, s2.w));
        }
    }
    // N >= 2, as for SeTerm; scale: what the closed variance of the accumulated summands is multiplied by
    __device__ __forceinline__ void close_into(float4 &var, int N, float scale) const {
        const float fn = (float)N, c = fn / (fn - 1.0f);
        var.x = fmaf(c * fmaf(-s1.x / fn, s1.x, s2.x), scale, var.x);
        var.y = fmaf(c * fmaf(-s1.y / fn, s1.y, s2.y), scale, var.y);
        var.z = fmaf(c * fmaf(-s1.z / fn, s1.z, s2.z), scale, var.z);
        var.w = fmaf(c * fmaf(-s1.w / fn, s1.w, s2.w), scale, var.w);
    }
};
template <>
struct SeTerm4<false> {};
template <bool ON>
struct SezState {
    float4 var;
};
template <>
struct SezState<false> {};

// The third flavour of the TOP-frame bookkeeping (scasml_picard_tree_summands): where SE / SEZ accumulate a summand into a term's variance,
// SUM stores it -- into a table that adds across the ranks of a sample-sharded solve, which sums of squares do not.  SUM = 1: the summands
// of u; 2: those of (u, z_1 .. z_d).  The walk visits the summands in the table's order -- terminal sample 0, 1, ..., then the paths of level
// 0, 1, ... -- and stores exactly one per visit, so the lane's address of its root's entry steps from summand to summand, and its top bit
// (no address has it) says that the lane stores nothing: no index arithmetic and no separate predicate are kept across the walk.
template <int SUM>
struct SumState {
    uint64_t at;      // address of the next summand's entry for this lane's root; | kNoStore in a lane that shadows the last root and,
                      // SUM = 1, in every lane of a group but its first
    uint32_t stride;  // bytes between consecutive summands: 4 ldy * ncol
    static constexpr uint64_t kNoStore = 1ull << 63;
};
template <>
struct SumState<0> {};
template <bool ON>
struct SumScale {     // what a terminal sample's g and g nrm are stored times: 1 / mg, and the zs of uz()
    float inv_mg, zs;
};
template <>
struct SumScale<false> {};

template <int VAR, int MODE, int EQ, bool JAX = false, bool SE = false, bool SEZ = false, int SUM = 0>
struct Walker {
    static_assert(!SEZ || SE, "the standard errors of z come with that of u");
    static_assert(SUM == 0 || (!SE && !JAX && (MODE == SCASML_MODE_MLP || MODE == SCASML_MODE_ACCUMULATE)), "summands: MLP and ACCUMULATE on the Philox stream, instead of the fused estimate");
    const TreeArgs &a;
    SumState<SUM> sum; // SUM: where the root call's summands go (TOP frames only)
    SeState<SE> se;    // SE: the variance estimate of the root call's u, summed over its terms (TOP frames only)
    SezState<SEZ> sez; // SEZ: those of this lane's four dims of the root call's z
    float4 mask;       // 1 on this lane's live spatial dims, 0 on padding
    float4 tmask;      // 1 on the component that holds t in a stored row (column d)
    uint32_t row_off4; // (local * kp + 4 * gl) / 4: this lane's float4 inside a site's block of B rows
    uint32_t gp_off;   // local
    bool row_lane;     // 4 * gl < kp
    uint32_t gl;       // lane index inside the root's group = Philox quad index
    uint32_t root;     // global root index (Philox counter word 2)
    int64_t local;     // this root's index inside the call's batch: row of site s = s * B + local
    int unit;          // running unit index of the ROOT call (sample sharding)

    // Sum over the G lanes of a root's group, the same value in every lane: the xor butterfly o = G / 2, .., 1, every lane adding the value of
    // lane i ^ o (float addition commutes: both partners get the same bits).  Only how the partner's value arrives is chosen per step: a
    // run-time loop of ds_bpermute was five dependent LDS round trips per sum at d = 100 (address arithmetic, the LDS queue, an lgkmcnt wait
    // and an add each), along a chain of 666 sites that each wave walks serially.  Now o = 8, 4, 2, 1 are DPP operands of the add itself
    // (row_ror:8; row_half_mirror then a reversed quad, together lane i ^ 4; two quad permutations), o = 16 is one ds_swizzle (still an LDS-queue
    // instruction, but without an address register), and o = 32 (d > 124 only) stays a ds_bpermute.  G is wave-uniform (a kernel argument): a
    // scalar switch enters the ladder at its step.  (v_permlane16_swap for o = 16 was measured through inline assembly, the builtin's second
    // result being unusable with this compiler: ACCUMULATE 4.2 ms against 1.07, profiles/r09_picard_dim_sum_ab.txt.)
    // EVERY lane of the wave must be active at a call: a DPP or swizzle read of an inactive lane is not the partner's value.  It is so today
    // -- ownership tests are scalar, idle lanes shadow the last root instead of leaving, and uz's per-lane `readback` branch closes before
    // g_terminal -- and a call inside a lane-dependent branch would break it.
    template <int CTRL>
    static __device__ __forceinline__ float dpp(float v) {
        return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, false));
    }
    __device__ __forceinline__ float group_sum(float v) const {
        // The reference-stream kernels keep the loop of ds_bpermute (the same sum, the same bits): with the ladder their ACCUMULATE n = 3 kernel
        // went from 111 to 146 VGPRs and the parity mode's pass from 1.40 to 1.64 ms (profiles/r09_picard_dim_sum_ab.txt)
        if constexpr (JAX) {
            for (int o = a.G >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o);
            return v;
        }
        // Where the o = 32 step stands changes nothing but the register allocation, and that in opposite ways: as the switch's first case the
        // MLP-mode kernels of quadrature n = 2 hold one VGPR more than with the loop (82 for 81; with standard errors 94 for 93), in front of
        // the switch ACCUMULATE with standard errors grows from 94 to 101.  Each mode gets the place that costs it nothing
        // (tests/test_picard_registers.py; profiles/r09_picard_dim_sum_ab.txt, "Registers").
        constexpr bool kWideFirst = MODE == SCASML_MODE_MLP;
        if constexpr (kWideFirst) {
            if (a.logG == 6) v += __shfl_xor(v, 32);
        }
        switch (a.logG) {
            case 6:
                if constexpr (!kWideFirst) v += __shfl_xor(v, 32);
                [[fallthrough]];
            case 5: v += __builtin_bit_cast(float, __builtin_amdgcn_ds_swizzle(__builtin_bit_cast(int, v), 0x401F));   // swizzle(SWAP,16)
                [[fallthrough]];
            case 4: v += dpp<0x128>(v);                          // row_ror:8
                [[fallthrough]];
            case 3: v += dpp<0x1B>(dpp<0x141>(v));               // row_half_mirror, quad_perm:[3,2,1,0]
                [[fallthrough]];
            default:                                             // G >= 4 (fill_common_args)
                v += dpp<0x4E>(v);                               // quad_perm:[2,3,0,1]
                v += dpp<0xB1>(v);                               // quad_perm:[1,0,3,2]
        }
        return v;
    }
    __device__ __forceinline__ float dim_sum(float4 v) const {
        return group_sum(fmaf(mask.x, v.x, fmaf(mask.y, v.y, fmaf(mask.z, v.z, mask.w * v.w))));
    }
    __device__ __forceinline__ float4 normals(uint32_t site) const {
        return mul4(normal4(gl, site, root, a.stream, a.k0, a.k1), mask);
    }
    // sample m of a (batch, width, d) draw under key (k0, k1), for this root's row of the reference's flattened batch
    __device__ __forceinline__ float4 normals_jax(uint32_t kslot, uint64_t row, uint32_t width, uint32_t m) const {
        const uint32_t k0 = a.jk[2 * kslot], k1 = a.jk[2 * kslot + 1];
        const uint64_t first = (row * width + m) * (uint64_t)a.d + 4u * gl;
        float4 v;
        v.x = mask.x != 0.0f ? jax_normal_f16(k0, k1, first + 0) : 0.0f;
        v.y = mask.y != 0.0f ? jax_normal_f16(k0, k1, first + 1) : 0.0f;
        v.z = mask.z != 0.0f ? jax_normal_f16(k0, k1, first + 2) : 0.0f;
        v.w = mask.w != 0.0f ? jax_normal_f16(k0, k1, first + 3) : 0.0f;
        return v;
    }
    // path sub-keys one uz_solve call at level N consumes, its children's included (MLP.py:213-220, 231, 253)
    template <int N>
    __device__ __forceinline__ uint32_t nsplits() const {
        if constexpr (N <= 0) {
            return 0u;
        } else {
            return nsplits_from<N, 0>();
        }
    }
    template <int N, int L>
    __device__ __forceinline__ uint32_t nsplits_from() const {
        if constexpr (L >= N) {
            return 0u;
        } else {
            const uint32_t per = 1u + nsplits<L>() + nsplits<L - 1>();
            return (uint32_t)a.plan.term[N][L].q * per + nsplits_from<N, L + 1>();
        }
    }
    // Row addressing: row = site * B + local, so a site's rows start at a wave-uniform base (scalar 64-bit arithmetic) and
    // the lane contributes a fixed 32-bit element offset -- a 64-bit VGPR product per access costs three v_mad_u64_u32.
    __device__ __forceinline__ void emit_point(float4 X, float t, uint32_t site) const {
        if (!row_lane) return;                                    // lanes past the padded row
        float4 *base = reinterpret_cast<float4 *>(a.points + (int64_t)site * a.Bs * a.kp);
        base[row_off4] = fma4(t, tmask, mul4(X, mask));           // (X, t, zero pad)
    }
    __device__ __forceinline__ float4 gp_at(uint32_t site) const { return (a.gpv + (int64_t)site * a.Bs)[gp_off]; }
    __device__ __forceinline__ float4 load_point(uint32_t site) const {   // this lane's four dims of a stored tree point
        const float4 *base = reinterpret_cast<const float4 *>(a.points + (int64_t)site * a.Bs * a.kp);
        return base[row_off4];
    }
    __device__ __forceinline__ bool mine_at(int un) const {   // wave-uniform: scalar load
        return a.owner ? (int)a.owner[un] == a.rank : (un % a.world) == a.rank;
    }
    __device__ __forceinline__ bool owned(bool top) {
        if (!top || a.world == 1) return true;
        const bool mine = mine_at(unit);
        ++unit;
        return mine;
    }

    // The two parity flags of scasml_rng.  The summand kernels run under flags = 0 only (picard_tree_run refuses anything else), so in them both
    // are compile-time false: the key-reuse bookkeeping (cbase, c_plus, c_minus) and the float16 branches leave the unrolled tree, and with
    // them the scalar registers that the table's stores inside the sample loops would otherwise push into a stack slot
    // (profiles/picard_summands_regs.txt)
    __device__ __forceinline__ bool crn() const { return SUM != 0 ? false : a.crn != 0; }
    __device__ __forceinline__ bool f16() const { return SUM != 0 ? false : a.f16 != 0; }

    // SUM: the next summand of the root call, every entry of it: lane 0 of the group stores u's, every lane its live dims of z's.  Lane-predicated
    // stores only -- no dim_sum inside (group_sum: every lane is active at a sum)
    __device__ __forceinline__ void put(float yu, float4 yz) {
        if constexpr (SUM != 0) {
            if (!(sum.at & SumState<SUM>::kNoStore)) {
                float *row = reinterpret_cast<float *>(sum.at);
                if constexpr (SUM == 1) {
                    row[0] = yu;
                } else {
                    if (gl == 0) row[0] = yu;
                    store_z(row, 4 * (int)gl, a.d, yz);
                }
            }
            sum.at += sum.stride;
        }
    }

    // Equation.g at time T (equations/equations.py:146-162, 248-261) through the registry; ScaSML.py:61-63 subtracts the surrogate
    __device__ __forceinline__ float g_terminal(float4 XT, float u_hat) const {
        float g = EqDef<EQ>::G(dim_sum(EqDef<EQ>::phi(XT)), a.T);
        if (f16()) g = r16(g);                                    // terminal_constraint(...).astype(float16), equations.py:261
        if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
            g -= u_hat;
            if (f16()) g = r16(g);                                // float16 - float16 (ScaSML.py:62): a float16 value
        }
        return g;
    }
    // Equation.f (equations/equations.py:290-304, MLP.py:27-41); ScaSML.py:29-47: f(u_hat + u, sigma grad u_hat + z) - f(u_hat, sigma grad u_hat),
    // where f sees the gradient through its sum only, sum_i sigma d_i u_hat = sigma div u_hat
    __device__ __forceinline__ float f_eval(float uc, float4 zc, float4 gp) const {
        const float sz = dim_sum(zc);
        const float fd = (float)a.d;
        if constexpr (EqDef<EQ>::kGradSquare) {                   // f(u, sum z, |z|^2): one more sum over the dims (surrogate-free modes only)
            static_assert(MODE != SCASML_MODE_ACCUMULATE, "an f of |z|^2 needs the surrogate's full gradient per site: not in the fused evaluation");
            const float v = EqDef<EQ>::f2(uc, sz, dim_sum(mul4(zc, zc)), a.sigma, fd);
            return f16() ? r16(v) : v;
        } else if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
            const float sg = a.sigma * gp.y;
            const float v1 = EqDef<EQ>::f(uc + gp.x, sg + sz, a.sigma, fd), v2 = EqDef<EQ>::f(gp.x, sg, a.sigma, fd);
            return f16() ? r16(r16(v1) - r16(v2)) : v1 - v2;      // generator(...).astype(float16) twice, then float16 - float16 (equations.py:304, ScaSML.py:45-47)
        } else {
            const float v = EqDef<EQ>::f(uc, sz, a.sigma, fd);
            return f16() ? r16(v) : v;
        }
    }

    // ---- one (n', l) term of the Picard sum ------------------------------------------------
    // jrow: this root's row in the reference's flattened batch of THIS call; jfirst: sub-key index of node (L, k = 0) of this call
    template <int N, int L, bool TOP>
    __device__ __forceinline__ void level(float4 x, float t, float tau, uint32_t base, uint32_t cbase, uint32_t &o, float &u, float4 &z,
                                          uint64_t jrow = 0, uint32_t jfirst = 0) {
        const scasml_term &tm = a.plan.term[N][L];
        const int q = tm.q, mc = tm.mc;
        const uint32_t s_l = (uint32_t)tm.sites_l, s_lm = (uint32_t)tm.sites_lm1;
        const float inv_mc = rcp_fast((float)mc);
        SeTerm<SE && TOP> st;
        if constexpr (SE && TOP) st.begin();
        SeTerm4<SEZ && TOP> zt;
        if constexpr (SEZ && TOP) zt.begin();
        for (int m = 0; m < mc; ++m) {
            float4 X = x, W = f4(0.0f);
            float ym = 0.0f;                                     // SE: what sample path m adds to u (unused otherwise)
            float4 zm = f4(0.0f);                                // SEZ: what it adds to z
            // compat_crn: the children of every node k draw their terminal normals where the k = 0 children do
            // (MLP.py:167-168,178: one fixed key per uz_solve call, so calls of equal shape share their draws)
            const uint32_t c_plus = cbase + o + 1u, c_minus = c_plus + s_l;
            // sample sharding, quadrature paths: the draws of nodes other ranks own are replayed only up to the LAST node of this path that
            // this rank owns an addend of (every rank used to walk every path to its end: 35 steps per root at n = rho = 3, 5 % of a whole
            // step's draws on each of 8 ranks)
            int klast = q - 1;
            if constexpr (TOP && VAR == 0 && MODE != SCASML_MODE_ACCUMULATE) {
                if (a.world > 1) {
                    constexpr int per = L > 0 ? 2 : 1;
                    klast = -1;
                    for (int k = 0; k < q; ++k)
                        if (mine_at(unit + k * per) || (L > 0 && mine_at(unit + k * per + 1))) klast = k;
                }
            }
            for (int k = 0; k < q; ++k) {
                if constexpr (TOP && VAR == 0 && MODE != SCASML_MODE_ACCUMULATE) {
                    if (k > klast) {                             // nothing of this rank's further along the path
                        o += (uint32_t)(q - k) * (1u + s_l + s_lm);
                        unit += (q - k) * (L > 0 ? 2 : 1);
                        break;
                    }
                }
                const uint32_t site = base + o;
                o += 1;
                // Monte-Carlo sample sharding: the units dealt to ranks are the two ADDENDS a node (l, m, k) of the root call contributes to the root's
                // sums -- "+": w_k f(P_k, uz(l)) with the level-l subtree below the node (and, at l = 0, the surrogate's residual term), "-": the
                // level-(l-1) subtree's term (l > 0) -- not whole sample paths: the node's state is read back (ACCUMULATE), drawn directly (full
                // history) or replayed from the path's own cheap draws (below), and its surrogate values are evaluated by whoever owns either
                // addend.  At n = rho = 3 the largest unit shrinks from 264 sites to 58 and the dealt-load imbalance over 8 ranks from 3.19 to 1.00
                const bool mine = owned(TOP);                    // the "+" addend
                bool mine_minus = false;
                if constexpr (L > 0) mine_minus = owned(TOP);
                if constexpr (VAR == 1 || MODE == SCASML_MODE_ACCUMULATE) {
                    if (!mine && !mine_minus) {                  // nothing incremental in these forms
                        o += s_l + s_lm;
                        continue;
                    }
                }
                float tk, wk;
                float4 wvec;  // the vector multiplying y in the z estimator
                float dplus, dminus;
                if constexpr (VAR == 0 && MODE == SCASML_MODE_ACCUMULATE) {
                    // The pass that emitted the points already produced X_k, bit for bit; read it back instead
                    // of replaying Philox and the normal transform, and recover W_k = (X_k - x - mu (t_k - t)) / sigma (one
                    // rounding of a difference of O(1) numbers divided by sigma: ~1e-6 relative).
                    const float ck = tau * tm.cfrac[k];
                    X = load_point(site);
                    W = mul4(fma4(1.0f / a.sigma, add4(X, -a.mu * ck), f4_scale(x, -1.0f / a.sigma)), mask);
                    tk = t + ck;
                    wk = tau * tm.wfrac[k];
                    wvec = W;
                    dplus = rcp_fast(fmaf(tau, tm.dplus[k], 1e-6f));
                    dminus = rcp_fast(fmaf(tau, tm.cfrac[k], 1e-6f));
                } else if constexpr (VAR == 0) {                 // MLP.py:219-225
                    float4 xi;
                    if constexpr (JAX) xi = normals_jax(1u + jfirst + (uint32_t)k * (1u + nsplits<L>() + nsplits<L - 1>()), jrow, (uint32_t)mc, (uint32_t)m);
                    else xi = normals(site);
                    const float dk = tau * tm.dfrac[k];
                    const float sdk = sqrt_fast(dk);
                    W = fma4(sdk, xi, W);
                    X = fma4(a.sigma * sdk, xi, add4(X, a.mu * dk));
                    tk = fmaf(tau, tm.cfrac[k], t);
                    wk = tau * tm.wfrac[k];
                    wvec = W;
                    dplus = rcp_fast(fmaf(tau, tm.dplus[k], 1e-6f));   // MLP.py:249 (stale) / ScaSML.py:253
                    dminus = rcp_fast(fmaf(tau, tm.cfrac[k], 1e-6f));  // MLP.py:270
                } else {                                         // MLP_full_history.py:133-145
                    // JAX stream: the time and the normals of sample m of this call, and its terminal draws, all come from the ONE key
                    // split(PRNGKey(0), 1)[0] (MLP_full_history.py:92-93, 99, 133, 138), each at its own row-major index
                    float D;
                    if constexpr (JAX) D = jax_uniform_f16(a.jk[0], a.jk[1], jrow * (uint32_t)mc + (uint32_t)m) * tau;
                    else D = uniform_tau(site, root, a.stream, a.k0, a.k1) * tau;
                    const float sD = sqrt_fast(D);
                    // compat_crn: the level-0 draws ARE the terminal draws (MLP_full_history.py:92-93,99,138: one subkey).
                    // (ACCUMULATE replays these normals: reading the stored X back instead, as the terminal samples do, was
                    // measured slower -- 5.9 against 5.4 ms at n = 4, M = 3 -- the pass is bound by its reads, not its RNG.)
                    float4 xi;
                    if constexpr (JAX) xi = normals_jax(0u, jrow, (uint32_t)mc, (uint32_t)m);
                    else xi = normals(crn() && L == 0 ? base + (uint32_t)m : site);
                    X = fma4(a.sigma * sD, xi, add4(x, a.mu * D));
                    tk = t + D;
                    wk = tau;
                    wvec = xi;
                    dplus = dminus = __builtin_amdgcn_rsqf(D + 1e-6f);     // :158-159
                }
                if constexpr (VAR == 0 && MODE != SCASML_MODE_ACCUMULATE) {
                    if (!mine && !mine_minus) {                  // the path has advanced (X, W); this node's terms belong to other ranks
                        o += s_l + s_lm;
                        continue;
                    }
                }
                if constexpr (MODE == SCASML_MODE_GENERATE) emit_point(X, tk, site);
                float4 gp = f4(0.0f);
                if constexpr (MODE == SCASML_MODE_ACCUMULATE) gp = gp_at(site);

                float uc;
                float4 zc;
                const uint32_t jkid = jfirst + (uint32_t)k * (1u + nsplits<L>() + nsplits<L - 1>()) + 1u;   // the children's first sub-key
                const uint64_t jkrow = jrow * (uint32_t)mc + (uint32_t)m;
                // ACCUMULATE at l = 0: the "+" addend is f(u_hat + 0, sigma div u_hat + dim_sum(0)) - f(u_hat, sigma div u_hat) under the zero child
                // uz<0>, an exact +0 whenever f(u_hat, .) is finite, and u + 0 = u, fma(0 dplus, W, z) = z for finite dplus and W: it is not emitted
                // (380 of the headline tree's 666 sites; one dim_sum and two f each).  Only the sign of a zero u or z can differ.  Where f(u_hat, .)
                // is not finite the addend was NaN and made the root NaN; it still becomes NaN, through the residual addend below, whose eps_PDE
                // contains the same f(u_hat, .).  MLP mode keeps the addend: f(0, 0) = 0 holds for the registered equations, not by construction.
                if constexpr (!(MODE == SCASML_MODE_ACCUMULATE && L == 0)) {
                    if (mine) {
                        uz<L, false>(X, tk, base + o, (crn() && VAR == 0) ? c_plus : base + o, uc, zc, jkrow, jkid);
                        if constexpr (MODE != SCASML_MODE_GENERATE) {
                            const float y = f_eval(uc, zc, gp) * (wk * inv_mc);
                            u += y;                              // MLP.py:248
                            if constexpr ((SE || SUM != 0) && TOP) ym += y;
                            z = fma4(y * dplus, wvec, z);        // MLP.py:249
                            if constexpr ((SEZ || SUM == 2) && TOP) zm = fma4(y * dplus, wvec, zm);
                        }
                    }
                }
                o += s_l;
                if constexpr (L > 0) {
                    if (mine_minus) {
                        uz<L - 1, false>(X, tk, base + o, (crn() && VAR == 0) ? c_minus : base + o, uc, zc, jkrow, jkid + nsplits<L>());
                        if constexpr (MODE != SCASML_MODE_GENERATE) {
                            const float y = f_eval(uc, zc, gp) * (wk * inv_mc);
                            u -= y;                              // MLP.py:269
                            if constexpr ((SE || SUM != 0) && TOP) ym -= y;
                            z = fma4(-y * dminus, wvec, z);      // MLP.py:271
                            if constexpr ((SEZ || SUM == 2) && TOP) zm = fma4(-y * dminus, wvec, zm);
                        }
                    }
                    o += s_lm;
                } else if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
                    const float e = gp.z * (wk * inv_mc);        // ScaSML.py:274-280 (l = 0: one addend, mine)
                    u += e;
                    if constexpr ((SE || SUM != 0) && TOP) ym += e;
                    z = fma4(e * dminus, wvec, z);
                    if constexpr ((SEZ || SUM == 2) && TOP) zm = fma4(e * dminus, wvec, zm);
                }
            }
            if constexpr (SE && TOP) st.add(ym, m == 0);
            if constexpr (SEZ && TOP) zt.add(zm, m == 0);
            // SUM: after the node loop, which the klast break and both `continue`s leave with what this rank owns of the path (0: nothing)
            if constexpr (SUM != 0 && TOP) put(ym, zm);
        }
        if constexpr (SE && TOP) se.var += st.close(mc);
        if constexpr (SEZ && TOP) zt.close_into(sez.var, mc, 1.0f);
        if constexpr (L + 1 < N) level<N, L + 1, TOP>(x, t, tau, base, cbase, o, u, z, jrow, jfirst + (uint32_t)q * (1u + nsplits<L>() + nsplits<L - 1>()));
    }

    // ---- uz_solve at compile-time level N -----------------------------------------------------
    template <int N, bool TOP>
    __device__ __forceinline__ void uz(float4 x, float t, uint32_t base, uint32_t cbase, float &u_out, float4 &z_out, uint64_t jrow = 0,
                                       uint32_t jsplit = 0) {
        if constexpr (N == 0) {                                  // MLP.py:205-207
            u_out = 0.0f;
            z_out = f4(0.0f);
        } else {
            // a child's time t + U (T - t) can round up to (or one ulp past) T in binary32: its horizon is then 0, not negative
            // (sqrt of a negative horizon would poison the whole root with NaN: seen once per ~1e7 full-history draws)
            const float tau = fmaxf(a.T - t, 0.0f);
            const int mg = a.plan.mg[N];
            const float drift = a.mu * tau, vol = a.sigma * sqrt_fast(tau);
            float su = 0.0f;
            float4 sz = f4(0.0f);
            // ACCUMULATE reads the stored X_T back: the rows of the next kAhead samples are requested before this one is
            // consumed (one dependent HBM round trip per sample otherwise; the pass is bound by the bytes it keeps in flight)
            const bool readback = MODE == SCASML_MODE_ACCUMULATE && vol >= kReadbackMinVol;
            // (the queue exists in ACCUMULATE only.  The 36 bytes of scratch rocprof reports for the level-3 / level-4 MLP and GENERATE kernels are
            // not these arrays but the stack slot of six spilled SGPRs -- v_writelane / v_readlane, no scratch instruction: DESIGN.md 4.1)
            PrefetchQueue<MODE == SCASML_MODE_ACCUMULATE> pq;
            if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
#pragma unroll
                for (int p = 0; p < kAhead; ++p) {
                    pq.XT[p] = f4(0.0f);
                    pq.gp[p] = f4(0.0f);
                    if (!(TOP && a.world > 1) && p < mg) {
                        if (readback) pq.XT[p] = load_point(base + (uint32_t)p);
                        pq.gp[p] = gp_at(base + (uint32_t)p);
                    }
                }
            }
            SeTerm<SE && TOP> st;
            if constexpr (SE && TOP) st.begin();
            SeTerm4<SEZ && TOP> zt;
            if constexpr (SEZ && TOP) zt.begin();
            SumScale<SUM != 0 && TOP> ss;
            if constexpr (SUM != 0 && TOP) {
                ss.inv_mg = rcp_fast((float)mg);
                ss.zs = ss.inv_mg * rcp_fast(VAR == 0 ? tau + 1e-6f : tau);
            }
            for (int m = 0; m < mg; ++m) {                       // MLP.py:175-202
                const uint32_t site = base + (uint32_t)m;
                float4 nrm, XT, gpv = f4(0.0f);
                if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
                    if (!(TOP && a.world > 1)) {                 // un-sharded: software-pipelined reads
                        XT = pq.XT[0];
                        gpv = pq.gp[0];
#pragma unroll
                        for (int p = 0; p + 1 < kAhead; ++p) {
                            pq.XT[p] = pq.XT[p + 1];
                            pq.gp[p] = pq.gp[p + 1];
                        }
                        if (m + kAhead < mg) {
                            if (readback) pq.XT[kAhead - 1] = load_point(site + kAhead);
                            pq.gp[kAhead - 1] = gp_at(site + kAhead);
                        }
                    } else {
                        if (!owned(TOP)) {
                            if constexpr (SUM != 0 && TOP) put(0.0f, f4(0.0f));   // another rank's sample: this rank's partial is 0
                            continue;
                        }
                        if (readback) XT = load_point(site);
                        gpv = gp_at(site);
                    }
                    // The emitting pass stored X_T bit for bit: recover the normals (one rounding of a difference
                    // of O(1) numbers: ~1e-6 relative) instead of replaying Philox and the normal transform, which would be most
                    // of this pass's VALU work.  Close to T they cannot be recovered accurately (kReadbackMinVol): replay.
                    if (__builtin_expect(readback, 1)) {
                        const float rv = rcp_fast(vol);
                        nrm = mul4(fma4(rv, add4(XT, -drift), f4_scale(x, -rv)), mask);
                    } else {
                        if constexpr (JAX) nrm = normals_jax(0u, jrow, (uint32_t)mg, (uint32_t)m);
                        else nrm = normals(cbase + (uint32_t)m);
                        XT = fma4(vol, nrm, add4(x, drift));
                    }
                } else {
                    if (!owned(TOP)) {
                        if constexpr (SUM != 0 && TOP) put(0.0f, f4(0.0f));
                        continue;
                    }
                    if constexpr (JAX) nrm = normals_jax(0u, jrow, (uint32_t)mg, (uint32_t)m);   // every call: split(PRNGKey(0), 1)[0] (MLP.py:167-168, 178)
                    else nrm = normals(cbase + (uint32_t)m);
                    XT = fma4(vol, nrm, add4(x, drift));
                }
                if constexpr (MODE == SCASML_MODE_GENERATE) {
                    emit_point(XT, a.T, site);
                } else {
                    const float g = g_terminal(XT, gpv.x);
                    su += g;
                    if constexpr (SE && TOP) st.add(g, m == 0);
                    sz = fma4(g, nrm, sz);
                    if constexpr (SEZ && TOP) zt.add(f4_scale(nrm, g), m == 0);   // P_m = g nrm: what the line above adds
                    if constexpr (SUM != 0 && TOP) put(g * ss.inv_mg, f4_scale(f4_scale(nrm, g), ss.zs));   // g / mg and P_m zs
                }
            }
            const float inv_mg = rcp_fast((float)mg);
            if constexpr (SE && TOP) se.var += st.close(mg) * (inv_mg * inv_mg);   // the summands are g / mg
            float u = su * inv_mg;
            const float zs = inv_mg * rcp_fast(VAR == 0 ? tau + 1e-6f : tau);   // MLP.py:201 / MLP_full_history.py:122
            // the summands are P_m zs: at the full history's T - t = 0 the variance is that of inf P_m, inf or NaN and never a finite number
            if constexpr (SEZ && TOP) zt.close_into(sez.var, mg, zs * zs);
            // padding dims carry sz = 0: at T - t = 0 the full-history scale is 1/0 (MLP_full_history.py:122 has no epsilon) and
            // 0 * inf would put a NaN into the padding that dim_sum's 0 * NaN then spreads to the whole root
            float4 z = make_float4(mask.x != 0.0f ? sz.x * zs : 0.0f, mask.y != 0.0f ? sz.y * zs : 0.0f,
                                   mask.z != 0.0f ? sz.z * zs : 0.0f, mask.w != 0.0f ? sz.w * zs : 0.0f);
            uint32_t o = (uint32_t)mg;
            level<N, 0, TOP>(x, t, tau, base, cbase, o, u, z, jrow, jsplit);
            if (!(TOP && a.world > 1)) {                         // MLP.py:272-274
                u = clip1(u, a.clip);
                z = clip4(z, a.clip);
                // jnp.clip(...).astype(jnp.float16): MLP.py:274, ScaSML.py:284, MLP_full_history.py:180 -- ScaSML_full_history.py:199 does not cast
                if (f16() && !(VAR == 1 && MODE != SCASML_MODE_MLP)) {
                    u = r16(u);
                    z = make_float4(r16(z.x), r16(z.y), r16(z.z), r16(z.w));
                }
            }
            u_out = u;
            z_out = z;
        }
    }
};

// (An occupancy hint for ACCUMULATE was measured, profiles/r02_accumulate_prefetch.txt: 5 waves/SIMD 1.22 ms against 1.26, but the
// deeper levels then spill inside their loops; 6 and 8 are slower.  No hint.)
template <int VAR, int MODE, int N, int EQ, bool JAX = false, bool SE = false>
__global__ __launch_bounds__(256) void picard_tree_kernel(const TreeArgs a) {
    static_assert(!SE || (!JAX && MODE != SCASML_MODE_GENERATE), "standard errors: MLP and ACCUMULATE on the Philox stream");
    if constexpr (JAX) jax_table_to_lds();   // every thread, before any return below: the reference's stream needs its own 4 KB table only
    else normal_table_to_lds();
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * (blockDim.x >> 6)) + (threadIdx.x >> 6);
    int64_t local;
    uint32_t gl;
    if constexpr (MODE == SCASML_MODE_GENERATE) {
        // GENERATE takes no sum over dims: lanes need not form power-of-two groups.  Flat (root, quad) mapping over the
        // kp / 4 float4 of a row, so no lane idles through the Philox and the normal transform work (at d = 100: 28 lanes per root
        // instead of 32, 25 of them drawing normals).  (Mapping the lanes to the 25 quads that hold a spatial dim, with the row's other
        // float4 -- t, padding -- as a second store of the root's first lanes, saves the three idle draws but was measured much slower:
        // 1.66 ms against 1.08, profiles/r09_picard_dim_sum_ab.txt.  A row is written whole by neighbouring lanes of one store.)
        const int64_t flat = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
        const int quads = a.kp >> 2;
        local = flat / quads;
        gl = (uint32_t)(flat - local * quads);
    } else {
        const int rpw = 64 >> a.logG;
        local = (int64_t)wave * rpw + (lane >> a.logG);
        gl = (uint32_t)(lane & (a.G - 1));
    }
    const bool valid = local < a.B;
    if (!valid) local = a.B - 1;  // idle lanes shadow the last root; their stores are masked

    Walker<VAR, MODE, EQ, JAX, SE> w{a};
    if constexpr (SE) w.se.var = 0.0f;
    w.gl = gl;
    w.root = a.root0 + (uint32_t)local;
    w.local = local;
    w.unit = 0;
    const int dim0 = 4 * (int)w.gl;
    w.mask = live_mask(dim0, a.d);
    w.tmask = make_float4(dim0 + 0 == a.d ? 1.0f : 0.0f, dim0 + 1 == a.d ? 1.0f : 0.0f,
                          dim0 + 2 == a.d ? 1.0f : 0.0f, dim0 + 3 == a.d ? 1.0f : 0.0f);
    w.row_lane = dim0 < a.kp && (MODE != SCASML_MODE_GENERATE || valid);
    w.row_off4 = (uint32_t)((local * a.kp + (dim0 < a.kp ? dim0 : 0)) >> 2);   // a chunk's point buffer is < 2^32 floats per site block
    w.gp_off = (uint32_t)local;
    const float *row = a.x_t + local * (a.d + 1);
    float4 x;
    x.x = dim0 + 0 < a.d ? row[dim0 + 0] : 0.0f;
    x.y = dim0 + 1 < a.d ? row[dim0 + 1] : 0.0f;
    x.z = dim0 + 2 < a.d ? row[dim0 + 2] : 0.0f;
    x.w = dim0 + 3 < a.d ? row[dim0 + 3] : 0.0f;
    const float t = row[a.d];

    if constexpr (MODE == SCASML_MODE_GENERATE) {
        if (valid) w.emit_point(x, t, (uint32_t)(a.ppr - 1));   // the root itself, for ScaSML.py:303
    }
    float u;
    float4 z;
    w.template uz<N, true>(x, t, 0u, 0u, u, z, (uint64_t)a.root0 + (uint64_t)local, 0u);
    if constexpr (MODE != SCASML_MODE_GENERATE) {
        if (valid) {
            float *out = a.out_uz + local * (a.d + 1);
            if (w.gl == 0) {
                out[0] = one_nan(u);
                if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
                    if (a.out_uhat) a.out_uhat[local] = w.gp_at((uint32_t)(a.ppr - 1)).x;
                }
                // Var <= 0 (rounding) gives 0; a NaN Var -- the root's u is NaN -- stays NaN (fmaxf would turn it into an exact-looking 0)
                if constexpr (SE) a.out_se[local] = w.se.var <= 0.0f ? 0.0f : sqrtf(w.se.var);
            }
            store_z(out, dim0, a.d, one_nan4(z));
        }
    }
}

// The standard errors of u and of every z_i (scasml_picard_tree_stderr_uz): the same walk under Walker's SEZ flag, a.out_se holding rows of
// 1 + d.  A kernel template of its own, so that the names and argument lists of picard_tree_kernel's instances stay what they are; MLP and
// ACCUMULATE on the Philox stream only, so the root set-up below is picard_tree_kernel's without its GENERATE and reference-stream branches.
// (It is repeated here and not shared through an inlined function taking the arguments by reference: with one, five existing instances
// changed their register counts -- <0,2,2,0> 89 -> 88 VGPRs, <0,2,5,0> 279 -> 280, the SE instance <0,2,5,1> 258 VGPRs and 3576 B of
// scratch -> 138 and none -- and the existing kernels are to compile to the code they had: profiles/picard_stderr_uz_regs.txt.)
template <int VAR, int MODE, int N, int EQ>
__global__ __launch_bounds__(256) void picard_se_uz_kernel(const TreeArgs a) {
    static_assert(MODE == SCASML_MODE_MLP || MODE == SCASML_MODE_ACCUMULATE, "standard errors: MLP and ACCUMULATE on the Philox stream");
    normal_table_to_lds();                   // every thread, before any return below
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * (blockDim.x >> 6)) + (threadIdx.x >> 6);
    const int rpw = 64 >> a.logG;
    int64_t local = (int64_t)wave * rpw + (lane >> a.logG);
    const bool valid = local < a.B;
    if (!valid) local = a.B - 1;  // idle lanes shadow the last root; their stores are masked

    Walker<VAR, MODE, EQ, false, true, true> w{a};
    w.se.var = 0.0f;
    w.sez.var = f4(0.0f);
    w.gl = (uint32_t)(lane & (a.G - 1));
    w.root = a.root0 + (uint32_t)local;
    w.local = local;
    w.unit = 0;
    const int dim0 = 4 * (int)w.gl;
    w.mask = live_mask(dim0, a.d);
    w.tmask = make_float4(dim0 + 0 == a.d ? 1.0f : 0.0f, dim0 + 1 == a.d ? 1.0f : 0.0f,
                          dim0 + 2 == a.d ? 1.0f : 0.0f, dim0 + 3 == a.d ? 1.0f : 0.0f);
    w.row_lane = dim0 < a.kp;
    w.row_off4 = (uint32_t)((local * a.kp + (dim0 < a.kp ? dim0 : 0)) >> 2);
    w.gp_off = (uint32_t)local;
    const float *row = a.x_t + local * (a.d + 1);
    float4 x;
    x.x = dim0 + 0 < a.d ? row[dim0 + 0] : 0.0f;
    x.y = dim0 + 1 < a.d ? row[dim0 + 1] : 0.0f;
    x.z = dim0 + 2 < a.d ? row[dim0 + 2] : 0.0f;
    x.w = dim0 + 3 < a.d ? row[dim0 + 3] : 0.0f;
    const float t = row[a.d];

    float u;
    float4 z;
    w.template uz<N, true>(x, t, 0u, 0u, u, z, (uint64_t)a.root0 + (uint64_t)local, 0u);
    if (valid) {
        float *out = a.out_uz + local * (a.d + 1);
        float *se = a.out_se + local * (a.d + 1);            // (se_u, se_z_1 .. se_z_d), the layout of the out_uz row
        if (w.gl == 0) {
            out[0] = one_nan(u);
            if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
                if (a.out_uhat) a.out_uhat[local] = w.gp_at((uint32_t)(a.ppr - 1)).x;
            }
            se[0] = w.se.var <= 0.0f ? 0.0f : sqrtf(w.se.var);   // as picard_tree_kernel: Var <= 0 gives 0, a NaN Var stays NaN
        }
        store_z(out, dim0, a.d, one_nan4(z));
        const float4 v = w.sez.var;                          // this lane's live dims; padding dims (which may hold 0 * inf) are not stored
        store_z(se, dim0, a.d, make_float4(v.x <= 0.0f ? 0.0f : sqrtf(v.x), v.y <= 0.0f ? 0.0f : sqrtf(v.y),
                                           v.z <= 0.0f ? 0.0f : sqrtf(v.z), v.w <= 0.0f ? 0.0f : sqrtf(v.w)));
    }
}

// The summands of the root call (scasml_picard_tree_summands): the same walk under Walker's SUM flavour, a.out_se carrying the table
// (TreeArgs stays what it is: a new field would move the kernel arguments of every instance) and ldy its roots per summand.  A kernel template
// of its own for the reason picard_se_uz_kernel is one, with the same root set-up.
template <int VAR, int MODE, int N, int EQ, int SUM>
__global__ __launch_bounds__(256) void picard_sum_kernel(const TreeArgs a, const int64_t ldy) {
    static_assert(SUM == 1 || SUM == 2, "summands of u, or of (u, z)");
    normal_table_to_lds();                   // every thread, before any return below
    const int lane = threadIdx.x & 63;
    const int wave = (blockIdx.x * (blockDim.x >> 6)) + (threadIdx.x >> 6);
    const int rpw = 64 >> a.logG;
    int64_t local = (int64_t)wave * rpw + (lane >> a.logG);
    const bool valid = local < a.B;
    if (!valid) local = a.B - 1;  // idle lanes shadow the last root; their stores are masked

    Walker<VAR, MODE, EQ, false, false, false, SUM> w{a};
    const int ncol = SUM == 2 ? a.d + 1 : 1;
    w.sum.stride = 4u * (uint32_t)ldy * (uint32_t)ncol;
    w.gl = (uint32_t)(lane & (a.G - 1));
    w.sum.at = reinterpret_cast<uint64_t>(a.out_se + local * ncol) | (valid && (SUM == 2 || w.gl == 0) ? 0ull : SumState<SUM>::kNoStore);
    w.root = a.root0 + (uint32_t)local;
    w.local = local;
    w.unit = 0;
    const int dim0 = 4 * (int)w.gl;
    w.mask = live_mask(dim0, a.d);
    w.tmask = make_float4(dim0 + 0 == a.d ? 1.0f : 0.0f, dim0 + 1 == a.d ? 1.0f : 0.0f,
                          dim0 + 2 == a.d ? 1.0f : 0.0f, dim0 + 3 == a.d ? 1.0f : 0.0f);
    w.row_lane = dim0 < a.kp;
    w.row_off4 = (uint32_t)((local * a.kp + (dim0 < a.kp ? dim0 : 0)) >> 2);
    w.gp_off = (uint32_t)local;
    const float *row = a.x_t + local * (a.d + 1);
    float4 x;
    x.x = dim0 + 0 < a.d ? row[dim0 + 0] : 0.0f;
    x.y = dim0 + 1 < a.d ? row[dim0 + 1] : 0.0f;
    x.z = dim0 + 2 < a.d ? row[dim0 + 2] : 0.0f;
    x.w = dim0 + 3 < a.d ? row[dim0 + 3] : 0.0f;
    const float t = row[a.d];

    float u;
    float4 z;
    w.template uz<N, true>(x, t, 0u, 0u, u, z, (uint64_t)a.root0 + (uint64_t)local, 0u);
    if (valid) {
        float *out = a.out_uz + local * (a.d + 1);
        if (w.gl == 0) {
            out[0] = one_nan(u);
            if constexpr (MODE == SCASML_MODE_ACCUMULATE) {
                if (a.out_uhat) a.out_uhat[local] = w.gp_at((uint32_t)(a.ppr - 1)).x;
            }
        }
        store_z(out, dim0, a.d, one_nan4(z));
    }
}

// ---- the launch ladder ---------------------------------------------------------------------------
// Which picard_tree_kernel<VAR, MODE, N, EQ, JAX, SE> (SEZ: picard_se_uz_kernel<VAR, MODE, N, EQ>, which exist where the SE kernels do) exist,
// for either variant and every level of a unit's range -- the one statement of it:
//   GENERATE evaluates neither f nor g, so one instantiation (equation 0) serves every equation, and it has no sum to take an error of;
//   an f of |z|^2 needs the surrogate's full gradient per site, so its equation runs surrogate-free (SCASML_MODE_MLP), and it is not one of
//   the reference's, so never on the reference's stream;
//   standard errors are estimated on the Philox stream only (picard_tree_kernel's static_assert).
template <int MODE, int EQ, bool JAX, bool SE>
constexpr bool tree_instance() {
    if (SE && JAX) return false;
    if (MODE == SCASML_MODE_GENERATE) return EQ == SCASML_EQ_GRAD_DEPENDENT_NONLINEAR && !SE;
    if (EqDef<EQ>::kGradSquare) return MODE == SCASML_MODE_MLP && !JAX;
    return true;
}

// level n among N .. N_HI (a short compile-time recursion), then the launch
template <int VAR, int MODE, int EQ, bool JAX, bool SE, int N, int N_HI, bool SEZ, int SUM>
int launch_level(const TreeArgs &a, int n, dim3 grid, hipStream_t s, int64_t ldy) {
    static_assert(!SEZ || SE, "the standard errors of z come with that of u");
    if constexpr (!tree_instance<MODE, EQ, JAX, SE>()) {
        return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: no kernel for mode %d of equation id %d%s%s", MODE, EQ, JAX ? " on the reference's stream" : "",
                    SE ? " with standard errors" : "");
    } else if constexpr (N > N_HI) {
        if (n < 1 || n > SCASML_MAX_LEVEL) return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: level n=%d outside 1..%d", n, SCASML_MAX_LEVEL);
        return fail(SCASML_ERR_UNSUPPORTED, "%s level n=%d is not in this translation unit", SE ? "picard_tree_stderr:" : "picard_tree: SCASML_RNG_JAX_STREAM", n);
    } else {
        if (n == N) {
            if constexpr (SUM != 0) hipLaunchKernelGGL((picard_sum_kernel<VAR, MODE, N, EQ, SUM>), grid, dim3(256), 0, s, a, ldy);
            else if constexpr (SEZ) hipLaunchKernelGGL((picard_se_uz_kernel<VAR, MODE, N, EQ>), grid, dim3(256), 0, s, a);
            else hipLaunchKernelGGL((picard_tree_kernel<VAR, MODE, N, EQ, JAX, SE>), grid, dim3(256), 0, s, a);
            return check_launch(SE ? "picard_tree_stderr launch" : "picard_tree launch");
        }
        return launch_level<VAR, MODE, EQ, JAX, SE, N + 1, N_HI, SEZ, SUM>(a, n, grid, s, ldy);
    }
}

template <int VAR, int MODE, bool JAX, bool SE, int N_LO, int N_HI, bool SEZ, int SUM>
int launch_equation(const TreeArgs &a, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy) {
    switch (MODE == SCASML_MODE_GENERATE ? SCASML_EQ_GRAD_DEPENDENT_NONLINEAR : eq_id) {   // the one redirection of GENERATE (tree_instance)
        case SCASML_EQ_GRAD_DEPENDENT_NONLINEAR: return launch_level<VAR, MODE, SCASML_EQ_GRAD_DEPENDENT_NONLINEAR, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, n, grid, s, ldy);
        case SCASML_EQ_CUBIC_REACTION_DIFFUSION: return launch_level<VAR, MODE, SCASML_EQ_CUBIC_REACTION_DIFFUSION, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, n, grid, s, ldy);
        case SCASML_EQ_QUADRATIC_GRADIENT_REACTION_DIFFUSION:
            return launch_level<VAR, MODE, SCASML_EQ_QUADRATIC_GRADIENT_REACTION_DIFFUSION, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, n, grid, s, ldy);
    }
    return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: unknown equation id %d", eq_id);
}

template <int VAR, bool JAX, bool SE, int N_LO, int N_HI, bool SEZ, int SUM>
int launch_mode(const TreeArgs &a, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy) {
    switch (mode) {
        case SCASML_MODE_MLP: return launch_equation<VAR, SCASML_MODE_MLP, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, eq_id, n, grid, s, ldy);
        case SCASML_MODE_GENERATE: return launch_equation<VAR, SCASML_MODE_GENERATE, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, eq_id, n, grid, s, ldy);
        case SCASML_MODE_ACCUMULATE: return launch_equation<VAR, SCASML_MODE_ACCUMULATE, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, eq_id, n, grid, s, ldy);
    }
    return fail(SCASML_ERR_ARG, "picard_tree: unknown mode %d", mode);
}

// A translation unit's kernels are those of the ONE launch_tree<JAX, SE, N_LO, N_HI, SEZ> it instantiates: every variant, mode and equation of
// tree_instance at levels N_LO .. N_HI.  Refuses an unknown mode, then a level outside the unit's range; launches nothing it refuses.
template <bool JAX, bool SE, int N_LO, int N_HI, bool SEZ = false, int SUM = 0>
int launch_tree(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy = 0) {
    return variant == 0 ? launch_mode<0, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, mode, eq_id, n, grid, s, ldy)
                        : launch_mode<1, JAX, SE, N_LO, N_HI, SEZ, SUM>(a, mode, eq_id, n, grid, s, ldy);
}

// the reference's own random stream (compat_rng = "jax"): picard_tree_jax.hip (n <= 3) and picard_tree_jax_deep.hip (n = 4, 5)
int launch_tree_jax(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s);
int launch_tree_jax_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s);
// the kernels that also estimate the standard error of u (SE = true): picard_tree_stderr.hip (n <= 3) and picard_tree_stderr_deep.hip (n = 4, 5)
int launch_tree_stderr(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s);
int launch_tree_stderr_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s);
// the kernels that estimate the standard errors of u and of every z_i (SE and SEZ): picard_tree_stderr_uz.hip (n <= 3) and picard_tree_stderr_uz_deep.hip (n = 4, 5)
int launch_tree_stderr_uz(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s);
int launch_tree_stderr_uz_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s);
// the kernels that store the root call's summands (SUM = 1: of u, 2: of (u, z)): picard_tree_summands.hip, picard_tree_summands_uz.hip (n <= 3)
// and their _deep.hip (n = 4, 5); a.out_se carries the table, ldy its roots per summand
int launch_tree_summands(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy);
int launch_tree_summands_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy);
int launch_tree_summands_uz(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy);
int launch_tree_summands_uz_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy);
// The fields TreeArgs and StageArgs (picard_staged.hip) have in common: the plan, the batch and its site-major row geometry, the Philox key
// and the problem's constants.  Returns the roots a wavefront holds, 64 / G, which sizes either grid.
template <class Args>
int fill_common_args(Args &a, const scasml_problem *prob, const scasml_plan *plan, const scasml_rng &rng, int64_t B, int64_t site_stride) {
    a.plan = *plan;
    a.B = B;
    a.Bs = site_stride ? site_stride : B;
    a.ppr = (int64_t)plan->sites[plan->n] + 1;
    a.k0 = (uint32_t)(rng.seed & 0xFFFFFFFFu);
    a.k1 = (uint32_t)(rng.seed >> 32);
    a.stream = rng.stream;
    a.root0 = rng.root0;
    a.d = prob->d;
    a.kp = scasml_point_stride(prob->d);
    a.G = ceil_pow2(a.kp / 4);
    a.logG = 0;
    while ((1 << a.logG) < a.G) ++a.logG;
    a.T = prob->T;
    a.mu = prob->mu;
    a.sigma = prob->sigma;
    a.clip = prob->clip;
    return 64 / a.G;
}

// scasml_picard_tree, scasml_picard_tree_stderr, scasml_picard_tree_stderr_uz and scasml_picard_tree_summands (want_se selects the kernels and
// says what out_se holds): one validation, one launch geometry
enum SeWanted {
    kSeNone = 0,    // no estimate
    kSeU = 1,       // out_se: B standard errors of u
    kSeUz = 2,      // out_se: B rows of 1 + d, those of (u, z)
    kSummands = 3   // out_se: the table of the root call's summands, `ncol` columns (1: of u, 1 + d: of (u, z)) and `ldy` roots per summand
};
int picard_tree_run(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t, int64_t B, int64_t site_stride, scasml_rng rng,
                    float *points, const float *gp_vals, float *out_uz, float *out_uhat, float *out_se, SeWanted want_se, void *stream,
                    int32_t ncol = 0, int64_t ldy = 0);

}  // namespace scasml
