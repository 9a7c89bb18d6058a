// The Picard-tree kernels that estimate the Monte-Carlo standard errors of the root call's u AND of every component of its z (scasml_picard_tree_stderr_uz):
// levels 4 and 5 (picard_tree_stderr_uz.hip: 1..3 and the entry point).  A kernel template of their own, picard_se_uz_kernel, over the same
// walker (picard_tree.hpp: the SEZ flag touches TOP frames only, under if constexpr, as SE does).
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_stderr_uz_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    return launch_tree<false, true, 4, 5, true>(a, variant, mode, eq_id, n, grid, s);
}

}  // namespace scasml
