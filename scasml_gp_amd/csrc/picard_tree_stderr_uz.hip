// The Picard-tree kernels that estimate the Monte-Carlo standard errors of the root call's u AND of every component of its z (scasml_picard_tree_stderr_uz):
// levels 1..3 (picard_tree_stderr_uz_deep.hip: 4 and 5).  A kernel template of their own, picard_se_uz_kernel, over the same walker
// (picard_tree.hpp: the SEZ flag touches TOP frames only, under if constexpr, as SE does), in translation units of their own: the plain
// kernels and those of scasml_picard_tree_stderr stay as they are, and the build compiles these beside them.
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_stderr_uz(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    return launch_tree<false, true, 1, 3, true>(a, variant, mode, eq_id, n, grid, s);
}

}  // namespace scasml

using namespace scasml;

extern "C" int scasml_picard_tree_stderr_uz(const scasml_problem *prob, const scasml_plan *plan, int mode, const float *x_t, int64_t B,
                                            int64_t site_stride, scasml_rng rng, float *points, const float *gp_vals, float *out_uz,
                                            float *out_uhat, float *out_se_uz, void *stream) {
    return picard_tree_run(prob, plan, mode, x_t, B, site_stride, rng, points, gp_vals, out_uz, out_uhat, out_se_uz, kSeUz, stream);
}
