// lp_splatter_mlp_loop.hip -- host side of the layer-looped bf16x3 MFMA family of the MLP-Splatter + its forward kernels and the
// backward instantiations for up to four layers / widths of 64 (one wave per SIMD).  Device code: lp_splatter_mlp_loop.h; the
// two-layer backward at two waves per SIMD: lp_splatter_mlp_loop_shallow.hip.
#include "lp_splatter_mlp_loop.h"

namespace lp {

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------
bool splatter_mlp_loop_supported(const LpSplatterArgs& a) {
  const LpMlp& m = a.mlp;
  if (m.n_layers < 2 || m.n_layers > SLOOP_MAX) return false;
  if (!width_ok(m.dims[0])) return false;
  for (int l = 1; l < m.n_layers; ++l)
    if (!width_ok(m.dims[l]) || m.dims[l] != m.dims[1]) return false;
  const int CO = m.dims[m.n_layers];
  if (CO != 16 && CO != 32) return false;
  if (!grid_list_rows_ok(a.input_grid)) return false;  // 32-bit row indices
  if (a.out.n_rows >= (int64_t)1 << 31) return false;
  if (a.march.num_samples_inf > LOOP_N_INF) return false;
  const SplatLoopParams p = sloop_params(a, sloop_nb(a));
  return (size_t)p.img_end + (size_t)WAVES * SplatLoopTile::PER_WAVE * 4 <= 160 * 1024;
}

int splatter_mlp_forward_loop(const LpSplatterArgs& a, hipStream_t stream) {
  if (a.rays.n_rays == 0) return LP_OK;
  int rc;
  const int E = a.mlp.dims[0], CO = a.mlp.dims[a.mlp.n_layers], NB = sloop_nb(a);
#define LP_SL_FWD(EV, COV) rc = (NB == 1 && EV < 64) ? sloop_launch_fwd<EV, COV, (EV < 64 ? 1 : 2)>(a, stream) : sloop_launch_fwd<EV, COV, 2>(a, stream)
  if (E == 16) {
    if (CO == 16) LP_SL_FWD(16, 16); else LP_SL_FWD(16, 32);
  } else if (E == 32) {
    if (CO == 16) LP_SL_FWD(32, 16); else LP_SL_FWD(32, 32);
  } else {
    if (CO == 16) LP_SL_FWD(64, 16); else LP_SL_FWD(64, 32);
  }
#undef LP_SL_FWD
  if (rc) return rc;
  return check_launch("splat_mlp_fwd_loop");
}

int splatter_mlp_backward_loop(const LpSplatterArgs& a, hipStream_t stream) {
  if (a.rays.n_rays == 0) return LP_OK;
  int rc;
  if (sloop_bwd_shallow(a)) {
    if ((rc = g_relu_dump ? splatter_mlp_backward_loop_shallow_dump(a, stream) : splatter_mlp_backward_loop_shallow(a, stream))) return rc;
    return check_launch("splat_mlp_bwd_loop (two layers)");
  }
  if ((rc = g_relu_dump ? splatter_mlp_backward_loop_deep_dump(a, stream) : sloop_bwd_table_deep<false>(a, stream))) return rc;
  return check_launch("splat_mlp_bwd_loop");
}

// launch shape (include/lightplane_hip.h, lp_mlp_splatter_launch_shape)
void splatter_mlp_loop_shape(const LpSplatterArgs& a, int32_t* shape) {
  const int fw = sloop_fwd_waves(a);
  shape[1] = fw;
  shape[2] = sloop_segments(a, true, WAVES);
  shape[3] = sloop_bwd_shallow(a) ? 2 : SLOOP_MAX;
  shape[4] = sloop_nb(a);
  shape[5] = sloop_segments(a, false, fw);
}

int splatter_mlp_loop_dump_words(const LpSplatterArgs& a) { return sloop_dump_words(a); }

// what the MLP-Splatter's looped backward computes in (lp_build_info): the dX chains keep three limbs; dW per translation unit
const char* build_info_splatter_mlp() {
  return "{\"dx_limbs\": 3, \"dw\": "
#if LP_LOOP_DW_BF16
         "\"deeper than two layers / width 64: two-limb bf16 operands, v_mfma_f32_16x16x32_bf16; two-layer MLPs (two waves per SIMD): "
         "fp32 operands, v_mfma_f32_16x16x4_f32\"}";
#else
         "\"fp32 operands, v_mfma_f32_16x16x4_f32\"}";
#endif
}

}  // namespace lp
