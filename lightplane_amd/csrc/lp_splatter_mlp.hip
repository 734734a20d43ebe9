// lp_splatter_mlp.hip -- host side of the shape-generic MLP-Splatter kernels (device code: lp_splatter_mlp.h).
#include "lp_splatter_mlp.h"

namespace lp {

int splatter_mlp_forward_launch(const LpSplatterArgs& a, hipStream_t stream) {
  SplatMlpArgs sa;
  sa.a = a;
  const int total = make_plan(a, sa.p);
  const unsigned blocks = (unsigned)((a.rays.n_rays + 63) / 64);
  if (blocks == 0) return LP_OK;
  if (total <= 256)
    hipLaunchKernelGGL(splat_mlp_fwd_kernel<256>, dim3(blocks), dim3(64), 0, stream, sa);
  else if (total <= 1024)
    hipLaunchKernelGGL(splat_mlp_fwd_kernel<1024>, dim3(blocks), dim3(64), 0, stream, sa);
  else
    return set_error(LP_EUNSUPPORTED, "MLP splatter: sum of layer widths %d exceeds 1024", total);
  return check_launch("splat_mlp_fwd_kernel");
}

int splatter_mlp_backward_launch(const LpSplatterArgs& a, hipStream_t stream) {
  return g_relu_dump ? splatter_mlp_backward_dump_launch(a, stream) : splat_mlp_bwd_launch<false>(a, stream);
}

int splatter_mlp_dump_words(const LpSplatterArgs& a) { return splat_mlp_dump_words(a.mlp); }

}  // namespace lp
