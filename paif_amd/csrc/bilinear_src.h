// The source index of F.interpolate(mode="bilinear", align_corners=False): output coordinate o of an axis scaled by
// `scale` = in / out reads input rows i0 and i1 with weights (1 - l1) and l1.  One copy for every kernel that samples or
// scatters through that map (seg_backward.hip: resize adjoint, upsample_ce, upsample_argmax; seg_criteria.hip), so that the
// forward value, the full-resolution gradient and its adjoint agree bit for bit on which pixels they touch.
#pragma once
#include <hip/hip_runtime.h>

namespace paif {

__device__ __forceinline__ void src_index(float scale, int o, int isz, int& i0, int& i1, float& l1) {
  float f = scale * ((float)o + 0.5f) - 0.5f;
  f = f < 0.f ? 0.f : f;
  i0 = (int)f;
  i1 = i0 + (i0 < isz - 1 ? 1 : 0);
  l1 = f - (float)i0;
}

}  // namespace paif
