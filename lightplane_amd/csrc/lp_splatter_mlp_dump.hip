// lp_splatter_mlp_dump.hip -- DUMP twin (lp_mlp_splatter_backward_relu_dump) of the shape-generic MLP-Splatter backward
// (lp_splatter_mlp.h), compiled with the same flags as its production twin.
#include "lp_splatter_mlp.h"

namespace lp {

int splatter_mlp_backward_dump_launch(const LpSplatterArgs& a, hipStream_t stream) {
#ifdef LP_TEST_HOOKS
  return splat_mlp_bwd_launch<true>(a, stream);
#else
  (void)a, (void)stream;
  return set_error(LP_EUNSUPPORTED, "relu dump: this library was built without -DLP_TEST_HOOKS (no DUMP twins)");
#endif
}

}  // namespace lp
