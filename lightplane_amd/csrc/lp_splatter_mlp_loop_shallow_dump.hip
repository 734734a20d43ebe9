// lp_splatter_mlp_loop_shallow_dump.hip -- DUMP twins (lp_mlp_splatter_backward_relu_dump) of the two-layer backward of
// lp_splatter_mlp_loop_shallow.hip, compiled with the same flags (build.py FILE_FLAGS).
#include "lp_splatter_mlp_loop.h"

namespace lp {

int splatter_mlp_backward_loop_shallow_dump(const LpSplatterArgs& a, hipStream_t stream) {
#ifdef LP_TEST_HOOKS
  return sloop_bwd_table_shallow<true>(a, stream);
#else
  (void)a, (void)stream;
  return set_error(LP_EUNSUPPORTED, "relu dump: this library was built without -DLP_TEST_HOOKS (no DUMP twins)");
#endif
}

}  // namespace lp
