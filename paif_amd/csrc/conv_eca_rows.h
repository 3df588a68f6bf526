// Interface between the ECA-block entry (fusion_kernels.hip: paif_eca_conv2_gated_fwd_f16) and the row-streaming conv2 kernels of
// conv_eca_rows.hip: fp16 NHWC-32 maps, plain fp16 weights.
#pragma once
#include <hip/hip_runtime.h>

namespace paif_eca_rows {

struct Args {
  const void* r;          // conv2's source: the UN-activated fp16 NHWC-32 map (also the block's residual)
  const void* wpk;        // conv2's fp16 weight pack [tap][ks][hi|lo][64 lanes][8 fp16]: the hi halves are used
  const float* in_prelu;  // 1 float: slope of the PReLU in front of conv2
  const float* prelu;     // 1 float: slope of the block's closing PReLU (GATED)
  const float* gate;      // [B][32] (GATED)
  float* partial;         // [paif_conv2d_blocks(B, H, W)][32] channel sums of conv2's fp32 result (POOL)
  void* out;              // fp16 NHWC-32 (GATED, STAGED)
  int B, H, W;
};

enum Mode { POOL = 0, GATED = 1, STAGED = 2 };   // STAGED: the test hook -- `out` = the PReLU'd operand rows, no conv result used

bool fits(int B, int H, int W);        // the hard limits: 32-bit byte offsets with the out-of-range marker above them
bool by_size_rule(int B, int H, int W);   // fits() and the sizes at which the row runs fill the chip
int env_switch();                      // PAIF_ECA_ROWS, read per call: -1 unset, 0 never, 1 wherever fits()
int launch(Mode m, const Args& a, hipStream_t st);

}  // namespace paif_eca_rows
