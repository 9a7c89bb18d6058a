// The Picard-tree kernels that store the summands of the root call's u AND of every component of its z (scasml_picard_tree_summands with
// ncol = 1 + d): levels 1..3 (picard_tree_summands_uz_deep.hip: 4 and 5).  picard_sum_kernel under the walker's SUM = 2 flavour.
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_summands_uz(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s, int64_t ldy) {
    return launch_tree<false, true, 1, 3, false, 2>(a, variant, mode, eq_id, n, grid, s, ldy);
}

}  // namespace scasml
