// The Picard-tree kernels that also estimate the Monte-Carlo standard error of the root call's u (scasml_picard_tree_stderr): levels 4 and 5 (picard_tree_stderr.hip: 1..3 and the entry point).
// A translation unit of its own so that the build compiles these instantiations beside picard_tree.hip's, whose kernels stay as they are
// (picard_tree.hpp: the SE flag touches TOP frames only, under if constexpr).
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_stderr_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    return launch_tree<false, true, 4, 5>(a, variant, mode, eq_id, n, grid, s);
}

}  // namespace scasml
