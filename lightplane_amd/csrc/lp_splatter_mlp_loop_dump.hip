// lp_splatter_mlp_loop_dump.hip -- DUMP twins (lp_mlp_splatter_backward_relu_dump) of lp_splatter_mlp_loop.hip's backward
// instantiations (E in {16, 32, 64}, Cout in {16, 32}, one or two blocks), compiled with the same flags as their production twins.
#include "lp_splatter_mlp_loop.h"

namespace lp {

int splatter_mlp_backward_loop_deep_dump(const LpSplatterArgs& a, hipStream_t stream) {
#ifdef LP_TEST_HOOKS
  return sloop_bwd_table_deep<true>(a, stream);
#else
  (void)a, (void)stream;
  return set_error(LP_EUNSUPPORTED, "relu dump: this library was built without -DLP_TEST_HOOKS (no DUMP twins)");
#endif
}

}  // namespace lp
