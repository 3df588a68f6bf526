// U2Fusion baseline (reference fusion_model/U2Fusion.py:91-125): conv_1 2 -> 44, five dense layers 44 (i + 1) -> 44 whose outputs are
// appended to the concat, sub 264 -> 128 -> 64 -> 32 -> 1, every conv 3 x 3 with zero pad 1, LeakyReLU(0.2) after all but the last, tanh
// after the last.  Forward and the reverse pass (input gradients).  One launch per layer, nothing fused across layers.
//
// LAYOUT.  fp32 NHWC.  ONE slab cat[B][H][W][264] holds conv_1's map and the five dense maps in the reference's cat order: dense layer i
// reads channels [0, 44 (i + 1)) and writes [44 (i + 1), 44 (i + 2)); the concat is never built a second time.  s1[..][128], s2[..][64],
// s3[..][32] are the maps of sub.0 .. sub.2.  The gradient buffers use the same layouts.  44 = 11 channel quads: every slice starts at a
// multiple of 176 B and float4 accesses stay aligned.
//
// Layers 1..8 and their transposes run on the matrix core: the slab conv of conv_slab.h (the kernel, its operand pack and its plan are
// described there), 3 x 3, LeakyReLU(0.2).  The reverse pass stages dz = d * (taped > 0 ? 1 : 0.2) through the kernel's input mask and
// runs the same kernel on a second weight pack (taps flipped, ci / co swapped).
//
// conv_1, sub.3 and their transposes run on the vector unit, weights through the scalar cache.
//
// BORDER RULE.  Every conv zero-pads its own input: whatever is read outside the image is zero at every level (total halo 10).
// LEAKYRELU.  torch: x > 0 ? x : 0.2 * x; in reverse the branch comes from the taped OUTPUT (same sign), a pre-activation of exactly 0
// takes the 0.2 branch.  The bias is added LAST, after the conv sum.
// No atomics: every output element is owned by one lane, the summation order is fixed, and no launch reads channels it writes.
#include <math.h>

#include "conv_slab.h"

namespace {

using namespace paif_slab;

constexpr float SLOPE = 0.2f;
constexpr int G = 44;            // growth = channels of conv_1 and of every dense layer
constexpr int CAT = 6 * G;       // 264

// ---- the ten convs ---------------------------------------------------------------------------------------------------------------------
// layer 0: conv_1, 1..5: dense_layers.0..4, 6..8: sub.0..2, 9: sub.3.  Layers 1..8 run on the matrix core.
struct Layer {
  int cin, cout;
};
__host__ __device__ constexpr Layer layer_of(int l) {
  return l == 0 ? Layer{2, G} : l <= 5 ? Layer{G * l, G} : l == 6 ? Layer{CAT, 128} : l == 7 ? Layer{128, 64} : l == 8 ? Layer{64, 32} : Layer{32, 1};
}

__host__ __device__ constexpr Plan plan_of(int l, bool transposed) {
  return transposed ? plan_for(layer_of(l).cin, layer_of(l).cout, 9) : plan_for(layer_of(l).cout, layer_of(l).cin, 9);
}

// packed weights, offsets in floats (all multiples of 4)
constexpr int PK_STEM_W = 0;                    // [plane 2][tap 9][co 44]
constexpr int PK_STEM_B = 2 * 9 * G;            // [co 44]
constexpr int PK_HEAD_W = PK_STEM_B + G;        // [tap 9][ci 32]
constexpr int PK_HEAD_B = PK_HEAD_W + 9 * 32;   // [1], padded to 4
constexpr int PK_BIAS = PK_HEAD_B + 4;          // layers 1..8 one after the other
constexpr int PK_OPS = PK_BIAS + 5 * G + 128 + 64 + 32;
__host__ __device__ constexpr size_t bias_off(int l) {
  size_t o = PK_BIAS;
  for (int i = 1; i < l; ++i) o += layer_of(i).cout;
  return o;
}
__host__ __device__ constexpr size_t ops_off(int l, bool transposed) {   // forward packs of layers 1..8, then the transposed ones
  size_t o = PK_OPS;
  for (int t = 0; t < 2; ++t)
    for (int i = 1; i <= 8; ++i) {
      if (t == (int)transposed && i == l) return o;
      o += plan_of(i, t != 0).floats();
    }
  return o;
}
constexpr size_t PK_FLOATS = ops_off(8, true) + plan_of(8, true).floats();
static_assert(PK_OPS % 4 == 0 && PK_BIAS % 4 == 0 && PK_HEAD_W % 4 == 0, "float4 loads from the pack stay aligned");
static_assert(PK_HEAD_B == PK_HEAD_W + 9 * 32, "head32_*_k read the bias behind the weights");
static_assert(ops_off(8, true) == 1420836, "the operand packs stay where they are");
static_assert(PK_FLOATS == 1439268, "the pack's size is part of the ABI (paif_u2fusion_pack_floats)");

// ---- weight packing: conv_1 (layer 0), the biases of layers 1..8, sub.3 (layer 9); the operand packs are pack_ops of conv_slab.h ---------
__global__ void pack_small_k(const float* __restrict__ w, const float* __restrict__ b, int layer, float* __restrict__ pack) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (layer == 0) {
    if (i < 2 * 9 * G) {   // i = (plane * 9 + tap) * 44 + co
      const int co = i % G, pt = i / G, tap = pt % 9, c = pt / 9;
      pack[PK_STEM_W + i] = w[(co * 2 + c) * 9 + tap];
    }
    if (i < G) pack[PK_STEM_B + i] = b[i];
  } else if (layer == 9) {
    if (i < 9 * 32) pack[PK_HEAD_W + i] = w[(i & 31) * 9 + (i >> 5)];   // i = tap * 32 + ci
    if (i == 0) pack[PK_HEAD_B] = b[0];
  } else if (i < layer_of(layer).cout) {
    pack[bias_off(layer) + i] = b[i];
  }
}

// ---- conv_1: 2 -> 44, bias, LeakyReLU, into channels [0, 44) of cat.  One pixel per thread -----------------------------------------------
__global__ __launch_bounds__(256) void stem_fwd_k(const float* __restrict__ x1, size_t sb1, const float* __restrict__ x2, size_t sb2,
                                                  const float* __restrict__ pack, float* __restrict__ cat, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float acc[G];
#pragma unroll
  for (int c = 0; c < G; ++c) acc[c] = 0.f;
#pragma unroll 1   // 44 weights in scalar registers at a time
  for (int pt = 0; pt < 18; ++pt) {
    const int pl = pt / 9, tap = pt - 9 * pl;
    const float* __restrict__ src = pl ? x2 + b * sb2 : x1 + b * sb1;
    const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
    const float v = ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? src[(size_t)gy * W + gx] : 0.f;
    const float* __restrict__ wt = pack + PK_STEM_W + pt * G;
#pragma unroll
    for (int c = 0; c < G; ++c) acc[c] = fmaf(wt[c], v, acc[c]);
  }
  const float* __restrict__ bs = pack + PK_STEM_B;
  float* o = cat + i * CAT;
#pragma unroll
  for (int c = 0; c < G; c += 4)
    *reinterpret_cast<float4*>(o + c) = make_float4(leaky(acc[c] + bs[c], SLOPE), leaky(acc[c + 1] + bs[c + 1], SLOPE),
                                                    leaky(acc[c + 2] + bs[c + 2], SLOPE), leaky(acc[c + 3] + bs[c + 3], SLOPE));
}

// Reverse of conv_1: dz = d_cat[0:44] * mask; d_x[plane][p] = sum over tap, co of W[co][plane][tap] * dz[p - (tap - centre)][co]
__global__ __launch_bounds__(256) void stem_bwd_k(const float* __restrict__ pack, const float* __restrict__ cat, const float* __restrict__ dcat,
                                                  float* __restrict__ d1, float* __restrict__ d2, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y - (tap / 3 - 1), gx = x - (tap % 3 - 1);
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const size_t o = ((size_t)b * hw + (size_t)gy * W + gx) * CAT;
    const float* __restrict__ w1 = pack + PK_STEM_W + tap * G;
    const float* __restrict__ w2 = pack + PK_STEM_W + (9 + tap) * G;
#pragma unroll
    for (int c = 0; c < G; c += 4) {
      const float4 z = dleaky4(*reinterpret_cast<const float4*>(cat + o + c), *reinterpret_cast<const float4*>(dcat + o + c), SLOPE);
      s1 = fmaf(w1[c], z.x, s1), s1 = fmaf(w1[c + 1], z.y, s1), s1 = fmaf(w1[c + 2], z.z, s1), s1 = fmaf(w1[c + 3], z.w, s1);
      s2 = fmaf(w2[c], z.x, s2), s2 = fmaf(w2[c + 1], z.y, s2), s2 = fmaf(w2[c + 2], z.z, s2), s2 = fmaf(w2[c + 3], z.w, s2);
    }
  }
  d1[i] = s1;
  d2[i] = s2;
}

// sub.3 (32 -> 1, bias, tanh) and its reverse (dy = g * (1 - out^2)) are head32_fwd_k / head32_bwd_k<ACT_TANH> of conv_slab.h.

}  // namespace

extern "C" size_t paif_u2fusion_pack_floats(void) { return PK_FLOATS; }

extern "C" int paif_u2fusion_pack_conv(const float* w, const float* b, int layer, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && pack, PAIF_EINVAL, "u2fusion_pack_conv: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 9, PAIF_EINVAL, "u2fusion_pack_conv: layer %d outside [0, 9]", layer);
  const hipStream_t s = paif::as_stream(stream);
  hipLaunchKernelGGL(pack_small_k, dim3(4), dim3(256), 0, s, w, b, layer, pack);
  if (layer >= 1 && layer <= 8)
    for (int t = 0; t < 2; ++t)   // the pack starts as zeros (ops.u2fusion_pack): the padding beyond M and K is not written
      pack_ops(w, layer_of(layer).cout, layer_of(layer).cin, 0, plan_of(layer, t != 0), t, pack + ops_off(layer, t != 0), s);
  PAIF_LAUNCH_CHECK("u2fusion_pack_conv");
  return 0;
}

extern "C" int paif_u2fusion_stem_fwd(const float* x_over, size_t sb1, const float* x_under, size_t sb2, const float* pack, float* cat, int B, int H,
                                      int W, paif_stream_t stream) {
  PAIF_REQUIRE(x_over && x_under && pack && cat, PAIF_EINVAL, "u2fusion_stem_fwd: null pointer");
  PAIF_SLAB_SHAPE("u2fusion_stem_fwd", 1, "", 31);
  PAIF_REQUIRE((size_t)H * W <= sb1 && (size_t)H * W <= sb2, PAIF_EINVAL, "u2fusion_stem_fwd: batch stride smaller than a plane");
  hipLaunchKernelGGL(stem_fwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), x_over, sb1, x_under, sb2, pack, cat, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_stem_fwd");
  return 0;
}

extern "C" int paif_u2fusion_conv_fwd(const float* pack, int layer, const float* in, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && out, PAIF_EINVAL, "u2fusion_conv_fwd: null pointer");
  PAIF_REQUIRE(layer >= 1 && layer <= 8, PAIF_EINVAL, "u2fusion_conv_fwd: layer %d outside [1, 8]", layer);
  PAIF_REQUIRE((layer <= 5) == (in == out), PAIF_EINVAL, "u2fusion_conv_fwd: a dense layer works inside cat, a sub layer from one map to another");
  PAIF_SLAB_SHAPE("u2fusion_conv_fwd", 1, "", 31);
  PAIF_SLAB_TILES("u2fusion_conv_fwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, false);
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = in, a.out = out, a.wpk = pack + ops_off(layer, false), a.bias = pack + bias_off(layer), a.slope = SLOPE;
  a.in_cs = layer <= 6 ? CAT : y.cin, a.nq = y.cin / 4;
  a.out_cs = layer <= 5 ? CAT : y.cout, a.out_off = layer <= 5 ? G * layer : 0, a.out_n = y.cout;
  launch_conv<9, false, EPI_ACT>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("u2fusion_conv_fwd");
  return 0;
}

extern "C" int paif_u2fusion_head_fwd(const float* pack, const float* s3, float* fused, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && s3 && fused, PAIF_EINVAL, "u2fusion_head_fwd: null pointer");
  PAIF_SLAB_SHAPE("u2fusion_head_fwd", 1, "", 31);
  hipLaunchKernelGGL(head32_fwd_k<ACT_TANH>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack + PK_HEAD_W, 0.f, s3, fused,
                     H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_head_fwd");
  return 0;
}

extern "C" int paif_u2fusion_head_bwd(const float* pack, const float* fused, const float* d_fused, float* d_s3, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(pack && fused && d_fused && d_s3, PAIF_EINVAL, "u2fusion_head_bwd: null pointer");
  PAIF_SLAB_SHAPE("u2fusion_head_bwd", 1, "", 31);
  hipLaunchKernelGGL(head32_bwd_k<ACT_TANH>, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, paif::as_stream(stream), pack + PK_HEAD_W, 0.f, fused,
                     d_fused, d_s3, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_head_bwd");
  return 0;
}

extern "C" int paif_u2fusion_conv_bwd(const float* pack, int layer, const float* taped, const float* d_out, float* d_in, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(pack && taped && d_out && d_in, PAIF_EINVAL, "u2fusion_conv_bwd: null pointer");
  PAIF_REQUIRE(layer >= 1 && layer <= 8, PAIF_EINVAL, "u2fusion_conv_bwd: layer %d outside [1, 8]", layer);
  PAIF_REQUIRE(taped != d_out && taped != d_in, PAIF_EINVAL, "u2fusion_conv_bwd: the gradient maps must not alias the taped maps");
  PAIF_REQUIRE((layer <= 5) == (d_out == d_in), PAIF_EINVAL, "u2fusion_conv_bwd: a dense layer works inside d_cat, a sub layer from one map to another");
  PAIF_SLAB_SHAPE("u2fusion_conv_bwd", 1, "", 31);
  PAIF_SLAB_TILES("u2fusion_conv_bwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, true);
  const int off = layer <= 5 ? G * layer : 0, cs = layer <= 5 ? CAT : y.cout;   // where the layer's output lives
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = d_out + off, a.mask = taped + off, a.out = d_in, a.wpk = pack + ops_off(layer, true), a.slope = SLOPE;
  a.in_cs = cs, a.nq = y.cout / 4;
  a.out_cs = layer <= 6 ? CAT : y.cin, a.out_off = 0, a.out_n = y.cin;
  const dim3 grid = conv_grid(pl, B, tx, ty);
  if (layer <= 5) launch_conv<9, true, EPI_ADD>(pl.MB, grid, paif::as_stream(stream), a);   // reads slice `layer` of d_cat, adds below it
  else launch_conv<9, true, EPI_STORE>(pl.MB, grid, paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("u2fusion_conv_bwd");
  return 0;
}

extern "C" int paif_u2fusion_stem_bwd(const float* pack, const float* cat, const float* d_cat, float* d_x_over, float* d_x_under, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(pack && cat && d_cat && d_x_over && d_x_under, PAIF_EINVAL, "u2fusion_stem_bwd: null pointer");
  PAIF_SLAB_SHAPE("u2fusion_stem_bwd", 1, "", 31);
  hipLaunchKernelGGL(stem_bwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack, cat, d_cat, d_x_over, d_x_under, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_stem_bwd");
  return 0;
}
