// The Picard-tree kernels that STORE the summands of the root call's u (scasml_picard_tree_summands with ncol = 1): levels 1..3
// (picard_tree_summands_deep.hip: 4 and 5; picard_tree_summands_uz*.hip: the (u, z) form).  A kernel template of their own, picard_sum_kernel,
// over the same walker (picard_tree.hpp: the SUM flavour touches TOP frames only, under if constexpr, as SE and SEZ do), in translation units
// of their own: every other kernel stays as it is, and the build compiles these beside them.
// Also here: the two entry points of the table, and the kernel that closes the variance from a completed one (scasml_picard_summands_stderr).
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_summands(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy) {
    return launch_tree<false, true, 1, 3, false, 1>(a, variant, mode, eq_id, n, grid, s, ldy);
}

// how many summands every term of the root call has: the terminal term, then the levels
struct SumTerms {
    int32_t nterms;
    int32_t count[SCASML_MAX_LEVEL + 1];
};

// One thread per (root, column) of the completed table: thread i = root * ncol + c reads y[j * stride + i], so neighbouring threads read
// neighbouring floats of every summand -- the kernel streams the table once and is bound by that.  The formula is SeTerm's, on the stored
// summands: per term the deviations from its first summand, N / (N - 1) (S2 - S1^2 / N); the sum over terms; sqrt.
__global__ __launch_bounds__(256) void summands_stderr_kernel(const float *__restrict__ y, int64_t cols, int64_t stride, SumTerms t, float *__restrict__ out_se) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cols) return;
    const float *p = y + i;
    float var = 0.0f;
    for (int j = 0; j < t.nterms; ++j) {
        const int N = t.count[j];
        SeTerm<true> st;
        st.begin();
        for (int m = 0; m < N; ++m, p += stride) st.add(*p, m == 0);
        var += st.close(N);
    }
    out_se[i] = var <= 0.0f ? 0.0f : sqrtf(var);   // Var <= 0 (rounding) gives 0; a NaN stays NaN (fmaxf would turn it into an exact-looking 0)
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_picard_tree_summands(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t, int64_t B, int64_t site_stride,
                                           scasml_rng rng, float *points, const float *gp_vals, float *out_uz, float *out_uhat, float *out_y, int32_t ncol,
                                           int64_t ldy, void *stream) {
    return picard_tree_run(prob, plan, mode, x_t, B, site_stride, rng, points, gp_vals, out_uz, out_uhat, out_y, kSummands, stream, ncol, ldy);
}

extern "C" int scasml_picard_summands_stderr(const scasml_plan *plan, const float *y, int64_t B, int64_t ldy, int32_t ncol, float *out_se, void *stream) {
    if (!plan) return fail(SCASML_ERR_ARG, "picard_summands_stderr: null plan");
    if (B < 0) return fail(SCASML_ERR_ARG, "picard_summands_stderr: negative batch");
    if (B == 0) return 0;
    if (plan->n < 0 || plan->n > SCASML_MAX_LEVEL) return fail(SCASML_ERR_UNSUPPORTED, "picard_summands_stderr: level n=%d outside 0..%d", plan->n, SCASML_MAX_LEVEL);
    if (ncol < 1) return fail(SCASML_ERR_ARG, "picard_summands_stderr: ncol = %d", ncol);
    if (!out_se) return fail(SCASML_ERR_ARG, "picard_summands_stderr: out_se is null");
    if (ldy == 0) ldy = B;
    if (ldy < B) return fail(SCASML_ERR_ARG, "picard_summands_stderr: ldy = %lld below the %lld roots", (long long)ldy, (long long)B);
    hipStream_t s = (hipStream_t)stream;
    const int n = plan->n;
    if (n == 0) {   // no summand: the level-0 call is exactly 0
        if (hipMemsetAsync(out_se, 0, sizeof(float) * B * ncol, s) != hipSuccess) return fail(SCASML_ERR_HIP, "picard_summands_stderr: memset failed");
        return 0;
    }
    if (!y) return fail(SCASML_ERR_ARG, "picard_summands_stderr: y is null");
    SumTerms t;
    t.nterms = n + 1;
    t.count[0] = plan->mg[n];
    for (int l = 0; l < n; ++l) t.count[1 + l] = plan->term[n][l].mc;
    for (int j = 0; j <= n; ++j)
        if (t.count[j] < 2)
            return fail(SCASML_ERR_UNSUPPORTED, "picard_summands_stderr: %s of level %d has %d sample: no estimable variance", j ? "a level term" : "the terminal term", n, t.count[j]);
    const int64_t cols = B * ncol, blocks = (cols + 255) / 256;
    if (blocks > 0x7FFFFFFF) return fail(SCASML_ERR_UNSUPPORTED, "picard_summands_stderr: batch too large");
    hipLaunchKernelGGL(summands_stderr_kernel, dim3((unsigned)blocks), dim3(256), 0, s, y, cols, ldy * (int64_t)ncol, t, out_se);
    return check_launch("picard_summands_stderr launch");
}
