// The Picard-tree kernels that store the summands of the root call's u (scasml_picard_tree_summands with ncol = 1), levels 4 and 5: the deep
// half of picard_tree_summands.hip, split off so that the build compiles the two in parallel.
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_summands_deep(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy) {
    return launch_tree<false, true, 4, SCASML_MAX_LEVEL, false, 1>(a, variant, mode, eq_id, n, grid, s, ldy);
}

}  // namespace scasml
