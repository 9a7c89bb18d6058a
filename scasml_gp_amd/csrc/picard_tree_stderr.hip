// The Picard-tree kernels that also estimate the Monte-Carlo standard error of the root call's u (scasml_picard_tree_stderr): levels 1..3 (picard_tree_stderr_deep.hip: 4 and 5).
// A translation unit of its own so that the build compiles these instantiations beside picard_tree.hip's, whose kernels stay as they are
// (picard_tree.hpp: the SE flag touches TOP frames only, under if constexpr).
#include "picard_tree.hpp"

namespace scasml {

template <int VAR, int MODE, int EQ>
static int stderr_level(const TreeArgs &a, int n, dim3 grid, hipStream_t s) {
    switch (n) {
        case 1: hipLaunchKernelGGL((picard_tree_kernel<VAR, MODE, 1, EQ, false, true>), grid, dim3(256), 0, s, a); break;
        case 2: hipLaunchKernelGGL((picard_tree_kernel<VAR, MODE, 2, EQ, false, true>), grid, dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL((picard_tree_kernel<VAR, MODE, 3, EQ, false, true>), grid, dim3(256), 0, s, a); break;
        default: return fail(SCASML_ERR_UNSUPPORTED, "picard_tree_stderr: level n=%d is not in this translation unit", n);
    }
    return check_launch("picard_tree_stderr launch");
}

template <int VAR>
static int stderr_variant(const TreeArgs &a, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    if (eq_mlp_only(eq_id))   // picard_tree_run has refused every other mode for it
        return stderr_level<VAR, SCASML_MODE_MLP, SCASML_EQ_QUADRATIC_GRADIENT_REACTION_DIFFUSION>(a, n, grid, s);
    int rc = SCASML_ERR_UNSUPPORTED;
    SCASML_EQ_SWITCH(eq_id, rc = (mode == SCASML_MODE_MLP ? stderr_level<VAR, SCASML_MODE_MLP, EQ>(a, n, grid, s)
                                                          : stderr_level<VAR, SCASML_MODE_ACCUMULATE, EQ>(a, n, grid, s)));
    return rc;
}

int launch_tree_stderr(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    return variant == 0 ? stderr_variant<0>(a, mode, eq_id, n, grid, s) : stderr_variant<1>(a, mode, eq_id, n, grid, s);
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_picard_tree_stderr(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t, int64_t B,
                                         int64_t site_stride, scasml_rng rng, float *points, const float *gp_vals, float *out_uz,
                                         float *out_uhat, float *out_se, void *stream) {
    return picard_tree_run(prob, plan, mode, x_t, B, site_stride, rng, points, gp_vals, out_uz, out_uhat, out_se, true, stream);
}
