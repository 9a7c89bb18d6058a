// The Picard-tree kernels on the reference's own random stream (SCASML_RNG_JAX_STREAM, compat_rng = "jax"): levels 1..3 (the reference's logged runs are n = 2).
// A translation unit of its own so that the build compiles these instantiations beside picard_tree.hip's (picard_tree.hpp).
#include "picard_tree.hpp"

namespace scasml {

int launch_tree_jax(const TreeArgs &a, int variant, int mode, int eq_id, int n, dim3 grid, hipStream_t s) {
    return launch_tree<true, false, 1, 3>(a, variant, mode, eq_id, n, grid, s);
}

}  // namespace scasml
