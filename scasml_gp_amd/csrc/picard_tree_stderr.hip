// The Picard-tree kernels that also estimate the Monte-Carlo standard error of the root call's u (scasml_picard_tree_stderr): levels 1..3 (picard_tree_stderr_deep.hip: 4 and 5).
// A translation unit of its own so that the build compiles these instantiations beside picard_tree.hip's, whose kernels stay as they are
// (picard_tree.hpp: the SE flag touches TOP frames only, under if constexpr).
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_stderr(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    return launch_tree<false, true, 1, 3>(a, variant, mode, eq_id, n, grid, s);
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_picard_tree_stderr(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t, int64_t B,
                                         int64_t site_stride, scasml_rng rng, float *points, const float *gp_vals, float *out_uz,
                                         float *out_uhat, float *out_se, void *stream) {
    return picard_tree_run(prob, plan, mode, x_t, B, site_stride, rng, points, gp_vals, out_uz, out_uhat, out_se, kSeU, stream);
}
