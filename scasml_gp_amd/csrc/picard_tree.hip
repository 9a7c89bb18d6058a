// Picard-tree kernel: the whole multilevel-Picard recursion of one evaluation point, walked
// depth-first inside one group of lanes of a 64-wide wavefront.
//
// Replaces MLP.uz_solve (solvers/MLP.py:141-274), ScaSML.uz_solve (solvers/ScaSML.py:149-284),
// MLP_full_history.uz_solve (solvers/MLP_full_history.py:64-180) and
// ScaSML_full_history.uz_solve (solvers/ScaSML_full_history.py:75-199).
//
// Mapping (DESIGN.md "picard_tree"): a root point owns G = pow2 >= round_up(d+4,16)/4 lanes; lane
// `gl` of the group holds spatial dims 4gl..4gl+3 of every d-vector (x, X, W, z) in one float4,
// so one Philox4x32 block per lane per path-step yields exactly that lane's four normals.
// 64/G roots share a wavefront and walk the SAME static tree in lock step -- the tree depends
// only on the tables (MLP.py:111-139), never on data, so there is no divergence.  The
// recursion is unrolled at compile time (level is a template parameter): every frame lives in
// VGPRs, sum_i over the dims is a log2(G)-step xor-shuffle, sum over Monte-Carlo samples is a
// register accumulation, and nothing but the root row is read from or written to HBM in
// MODE_MLP.  For ScaSML the same walk runs twice around the batched GP evaluation:
// MODE_GENERATE emits every tree point (coalesced float4 rows), MODE_ACCUMULATE reads those states
// back (recovering the normals from them; it replays Philox only where that would be inaccurate, see
// kReadbackMinVol, and for the full-history draws) and consumes (u_hat, div u_hat, eps_PDE) per point.

#include "picard_tree.hpp"

namespace scasml {

__global__ void clip_kernel(float *v, int64_t n, float c, int round16) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        const float x = clip1(v[i], c);
        v[i] = round16 ? r16(x) : x;
    }
}

__global__ void debug_normals_kernel(uint32_t k0, uint32_t k1, uint32_t stream, uint32_t root0, uint32_t site,
                                     int d, int64_t B, float *out) {
    normal_table_to_lds();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int nq = (d + 3) / 4;
    if (i >= B * nq) return;
    const int64_t b = i / nq;
    const int q = (int)(i % nq);
    const float4 n = normal4((uint32_t)q, site, root0 + (uint32_t)b, stream, k0, k1);
    const float v[4] = {n.x, n.y, n.z, n.w};
    for (int j = 0; j < 4; ++j)
        if (4 * q + j < d) out[b * d + 4 * q + j] = v[j];
}

__global__ void debug_jax_normals_kernel(uint32_t k0, uint32_t k1, uint64_t index0, int64_t count, float *out) {
    jax_table_to_lds();             // the path the tree kernels take: the tabulated transform
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) out[i] = jax_normal_f16(k0, k1, index0 + (uint64_t)i);
}

int picard_tree_run(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t, int64_t B, int64_t site_stride, scasml_rng rng,
                    float *points, const float *gp_vals, float *out_uz, float *out_uhat, float *out_se, SeWanted want_se, void *stream,
                    int32_t ncol, int64_t ldy) {
    if (const int rc = check_batch("picard_tree", prob, plan, B, site_stride)) return rc;
    if (B == 0) return 0;
    if (!x_t) return fail(SCASML_ERR_ARG, "picard_tree: x_t is null");
    if (prob->d < 1 || prob->d > SCASML_MAX_DIM)
        return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: d=%d outside 1..%d", prob->d, SCASML_MAX_DIM);
    if (!eq_known(prob->eq_id) && !eq_mlp_only(prob->eq_id)) return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: unknown equation id %d", prob->eq_id);
    if (eq_mlp_only(prob->eq_id) && (mode != SCASML_MODE_MLP || (rng.flags & SCASML_RNG_JAX_STREAM)))
        return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: equation id %d (f of |z|^2) runs in SCASML_MODE_MLP on the Philox stream only", prob->eq_id);
    if (plan->variant != 0 && plan->variant != 1) return fail(SCASML_ERR_ARG, "picard_tree: variant %d", plan->variant);
    if (plan->n < 0 || plan->n > SCASML_MAX_LEVEL)
        return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: level n=%d outside 0..%d", plan->n, SCASML_MAX_LEVEL);
    if (rng.world < 1 || rng.rank < 0 || rng.rank >= rng.world) return fail(SCASML_ERR_ARG, "picard_tree: bad rank/world");
    if (mode == SCASML_MODE_GENERATE && !points) return fail(SCASML_ERR_ARG, "picard_tree: GENERATE needs points");
    if (mode == SCASML_MODE_ACCUMULATE && (!gp_vals || !points))
        return fail(SCASML_ERR_ARG, "picard_tree: ACCUMULATE needs gp_vals and the points emitted by GENERATE");
    if (mode != SCASML_MODE_GENERATE && !out_uz) return fail(SCASML_ERR_ARG, "picard_tree: out_uz is null");
    int np, lp;
    if (first_bad_term(*plan, np, lp)) return fail(SCASML_ERR_ARG, "picard_tree: bad term [%d][%d]", np, lp);
    if (want_se == kSummands) {   // scasml_picard_tree_summands: the refusals of the fused estimates but the sharded one -- a table adds across ranks
        if (mode != SCASML_MODE_MLP && mode != SCASML_MODE_ACCUMULATE)
            return fail(SCASML_ERR_ARG, "picard_tree_summands: mode %d has no summands (SCASML_MODE_MLP or SCASML_MODE_ACCUMULATE)", mode);
        if (!out_se) return fail(SCASML_ERR_ARG, "picard_tree_summands: out_y is null");
        if (ncol != 1 && ncol != prob->d + 1)
            return fail(SCASML_ERR_ARG, "picard_tree_summands: ncol = %d is neither 1 (u) nor 1 + d = %d (u, z)", ncol, prob->d + 1);
        if (ldy == 0) ldy = B;
        if (ldy < B) return fail(SCASML_ERR_ARG, "picard_tree_summands: ldy = %lld below the %lld roots of the call", (long long)ldy, (long long)B);
        if (ldy > 0x3FFFFFFF / ncol)   // the kernels step from summand to summand by a 32-bit count of bytes
            return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_summands: ldy * ncol = %lld x %d floats per summand exceed 2^30 - 1: walk the batch in root chunks",
                        (long long)ldy, ncol);
        if (rng.flags != 0)
            return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_summands: rng.flags = %u: SCASML_RNG_COMPAT_CRN shares draws between summands, SCASML_RNG_JAX_STREAM and "
                        "SCASML_RNG_COMPAT_F16 are parity modes; the summands need flags = 0", rng.flags);
        if (plan->n > 0 && plan->mg[plan->n] < 2)
            return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_summands: the terminal term of level %d has %d sample: no estimable variance", plan->n, plan->mg[plan->n]);
        for (int l = 0; l < plan->n; ++l)
            if (plan->term[plan->n][l].mc < 2)
                return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_summands: term [%d][%d] has %d sample path: no estimable variance", plan->n, l, plan->term[plan->n][l].mc);
    } else if (want_se) {   // scasml_picard_tree_stderr and _stderr_uz: what has no estimate is refused, never answered with a partial number
        if (mode != SCASML_MODE_MLP && mode != SCASML_MODE_ACCUMULATE)
            return fail(SCASML_ERR_ARG, "picard_tree_stderr: mode %d has no estimate (SCASML_MODE_MLP or SCASML_MODE_ACCUMULATE)", mode);
        if (!out_se) return fail(SCASML_ERR_ARG, "picard_tree_stderr: %s is null", want_se == kSeUz ? "out_se_uz" : "out_se");
        if (rng.world != 1)
            return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_stderr: world = %d: sample-sharded units split a path's addends across ranks, whose sums of squares do not add", rng.world);
        if (rng.flags != 0)
            return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_stderr: rng.flags = %u: SCASML_RNG_COMPAT_CRN shares draws between summands, SCASML_RNG_JAX_STREAM and "
                        "SCASML_RNG_COMPAT_F16 are parity modes; the estimate needs flags = 0", rng.flags);
        if (plan->n > 0 && plan->mg[plan->n] < 2)
            return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_stderr: the terminal term of level %d has %d sample: no estimable variance", plan->n, plan->mg[plan->n]);
        for (int l = 0; l < plan->n; ++l)
            if (plan->term[plan->n][l].mc < 2)
                return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_stderr: term [%d][%d] has %d sample path: no estimable variance", plan->n, l, plan->term[plan->n][l].mc);
    }
    hipStream_t s = (hipStream_t)stream;
    if (plan->n == 0) {  // MLP.py:205-207: zeros (ScaSML: u_hat still requested by the caller through gp_eval)
        if (mode != SCASML_MODE_GENERATE) {
            if (hipMemsetAsync(out_uz, 0, sizeof(float) * B * (prob->d + 1), s) != hipSuccess)
                return fail(SCASML_ERR_HIP, "picard_tree: memset failed");
        }
        if (want_se == kSummands) return 0;   // a level-0 call has no summand: the table has no entry
        if (want_se && hipMemsetAsync(out_se, 0, sizeof(float) * B * (want_se == kSeUz ? prob->d + 1 : 1), s) != hipSuccess)
            return fail(SCASML_ERR_HIP, "picard_tree_stderr: memset failed");
        return 0;
    }
    TreeArgs a;
    const int rpw = fill_common_args(a, prob, plan, rng, B, site_stride);
    a.x_t = x_t;
    a.points = points;
    a.gpv = reinterpret_cast<const float4 *>(gp_vals);
    a.out_uz = out_uz;
    a.out_uhat = out_uhat;
    a.out_se = want_se ? out_se : nullptr;
    a.rank = rng.rank;
    a.world = rng.world;
    a.owner = rng.world > 1 ? rng.unit_owner : nullptr;
    a.crn = (rng.flags & SCASML_RNG_COMPAT_CRN) ? 1 : 0;
    a.f16 = (rng.flags & SCASML_RNG_COMPAT_F16) ? 1 : 0;
    a.jk = (rng.flags & SCASML_RNG_JAX_STREAM) ? rng.jax_keys : nullptr;
    if ((rng.flags & SCASML_RNG_JAX_STREAM) && !rng.jax_keys) return fail(SCASML_ERR_ARG, "picard_tree: SCASML_RNG_JAX_STREAM needs scasml_rng.jax_keys");
    const int64_t waves = mode == SCASML_MODE_GENERATE ? (B * (a.kp / 4) + 63) / 64 : (B + rpw - 1) / rpw;   // GENERATE: flat (root, quad) lanes
    const int64_t blocks = (waves + 3) / 4;
    if (blocks > 0x7FFFFFFF) return fail(SCASML_ERR_UNSUPPORTED, "picard_tree: batch too large");
    const dim3 grid((unsigned)blocks);
    // the ladder (picard_tree.hpp) of the unit that holds the kernels: standard errors and the reference's stream have two units each
    const int v = plan->variant, eq = prob->eq_id, n = plan->n;
    if (want_se == kSummands) {
        if (ncol == 1) return n > 3 ? launch_tree_summands_deep(a, v, mode, eq, n, grid, s, ldy) : launch_tree_summands(a, v, mode, eq, n, grid, s, ldy);
        return n > 3 ? launch_tree_summands_uz_deep(a, v, mode, eq, n, grid, s, ldy) : launch_tree_summands_uz(a, v, mode, eq, n, grid, s, ldy);
    }
    if (want_se == kSeUz) return n > 3 ? launch_tree_stderr_uz_deep(a, v, mode, eq, n, grid, s) : launch_tree_stderr_uz(a, v, mode, eq, n, grid, s);
    if (want_se) return n > 3 ? launch_tree_stderr_deep(a, v, mode, eq, n, grid, s) : launch_tree_stderr(a, v, mode, eq, n, grid, s);
    if (a.jk) return n > 3 ? launch_tree_jax_deep(a, v, mode, eq, n, grid, s) : launch_tree_jax(a, v, mode, eq, n, grid, s);
    return launch_tree<false, false, 1, SCASML_MAX_LEVEL>(a, v, mode, eq, n, grid, s);
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_picard_tree(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t,
                                  int64_t B, int64_t site_stride, scasml_rng rng, float *points, const float *gp_vals, float *out_uz,
                                  float *out_uhat, void *stream) {
    return picard_tree_run(prob, plan, mode, x_t, B, site_stride, rng, points, gp_vals, out_uz, out_uhat, nullptr, kSeNone, stream);
}

extern "C" int scasml_debug_jax_normals(uint32_t key0, uint32_t key1, uint64_t index0, int64_t count, float *out, void *stream) {
    if (!out || count < 0) return fail(SCASML_ERR_ARG, "debug_jax_normals: bad argument");
    if (count == 0) return 0;
    hipLaunchKernelGGL(debug_jax_normals_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, key0, key1, index0, count, out);
    return check_launch("debug_jax_normals launch");
}

extern "C" int scasml_clip_round16(float *uz, int64_t count, float clip, int32_t round16, void *stream) {
    if (!uz || count < 0) return fail(SCASML_ERR_ARG, "clip: bad argument");
    if (count == 0) return 0;
    hipLaunchKernelGGL(clip_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, (hipStream_t)stream, uz, count, clip, round16 ? 1 : 0);
    return check_launch("clip launch");
}

extern "C" int scasml_clip(float *uz, int64_t count, float clip, void *stream) { return scasml_clip_round16(uz, count, clip, 0, stream); }

// the normal transform of the 24-bit word k (a normal depends on the top 24 bits of its Philox word only), for k = k0 .. k0 + n - 1:
// tests/test_gpu_rng.py checks all 2^24 inputs against NumPy
__global__ void debug_transform_kernel(uint32_t k0, int64_t n, float *out) {
    normal_table_to_lds();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = icdf_normal((k0 + (uint32_t)i) << 8, normal_table_lds());
}

extern "C" int scasml_debug_transform(uint32_t k0, int64_t n, float *out, void *stream) {
    if (!out || n < 0 || (uint64_t)k0 + (uint64_t)n > (1ull << 24)) return fail(SCASML_ERR_ARG, "debug_transform: bad argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(debug_transform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, k0, n, out);
    return check_launch("debug_transform launch");
}

extern "C" int scasml_debug_normals(scasml_rng rng, uint32_t site, int32_t d, int64_t B, float *out, void *stream) {
    if (!out || d < 1 || B < 0) return fail(SCASML_ERR_ARG, "debug_normals: bad argument");
    if (B == 0) return 0;
    const int64_t n = B * ((d + 3) / 4);
    hipLaunchKernelGGL(debug_normals_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (uint32_t)(rng.seed & 0xFFFFFFFFu), (uint32_t)(rng.seed >> 32), rng.stream, rng.root0, site, d, B, out);
    return check_launch("debug_normals launch");
}
