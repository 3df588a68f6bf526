// SeAFusion baseline (reference fusion_model/SeaFusion.py:86-125).  Per stream (vis, inf): conv 3 x 3 1 -> 16 + LeakyReLU(0.2), RGBD(16, 32),
// RGBD(32, 48); decoder over cat(vis 48, inf 48): 3 x 3 convs 96 -> 64 -> 32 -> 16 with LeakyReLU(0.2) (the decoder's BatchNorm modules are
// never called by the reference's forward and do not exist here), 3 x 3 16 -> 1, tanh / 2 + 0.5.
// RGBD(C, Cout): x1 = LeakyReLU(0.2)(conv1 3 x 3 C -> C (x)), x2 = LeakyReLU(0.2)(conv2 3 x 3 2C -> C (cat(x, x1))),
// g = |convx(x)| + |convy(x)| (depthwise 3 x 3, no bias; the filters are PARAMETERS read from the pack, Sobel only at initialisation),
// out = LeakyReLU(0.1)(convdown 1 x 1 (cat(x, x1, x2)) + convup 1 x 1 (g)).
// Forward and the reverse pass (input gradients), 22 launches each, one per layer.
//
// LAYOUT.  fp32 NHWC.  Per stream slab1[B][H][W][64] and slab2[..][128]: a slab of an RGBD(C, .) holds x in [0, C), x1 in [C, 2C), x2 in
// [2C, 3C) and g in [3C, 4C), so conv2 reads [0, 2C), and the RGBD's tail is ONE 1 x 1 conv over all 4C channels with the weight
// [convdown.weight | convup.weight] and the bias convdown.bias + convup.bias.  RGBD1 writes [0, 32) of slab2; the two RGBD2 write enc[..][96]
// (vis [0, 48), inf [48, 96)), decode4's concat.  dec4 / dec3 / dec2: 64 / 32 / 16 channels.  sgn[B][H][W][C] (one byte per element)
// tapes sign(convx), sign(convy) of a block: the reverse pass takes abs' from it, bit for bit the forward's sign (abs'(0) = 0, as torch).
// The gradient buffers use the layouts of the maps.
//
// The 3 x 3 and 1 x 1 convs with 16 or more input channels run on the matrix core (conv_slab.h); the stems, the depthwise pair, the head
// and their transposes run on the vector unit.
//
// BORDER RULE.  Every conv zero-pads its own input (total halo 10).  LEAKYRELU.  x > 0 ? x : slope * x; in reverse the branch comes from
// the taped OUTPUT; exactly 0 takes the slope.  The bias is added LAST, after the conv sum.
// REVERSE ORDER per RGBD: the 1 x 1 transpose STORES all 4C channels of d_slab (input masked by the taped RGBD output, slope 0.1); the
// depthwise transpose reads [3C, 4C) and adds into [0, C); conv2's transpose reads [2C, 3C) and adds into [0, 2C); conv1's reads [C, 2C)
// and adds into [0, C).  No atomics, every output element is owned by one lane, and no launch reads channels it writes.
#include <math.h>
#include <stdint.h>

#include "conv_slab.h"

namespace {

using namespace paif_slab;

constexpr float SLOPE = 0.2f, SLOPE_RGBD = 0.1f;
constexpr int ENC = 96;

// block k = 2 * stream + r: RGBD r of stream (0 vis, 1 inf)
__host__ __device__ constexpr int blk_c(int k) { return 16 << (k & 1); }
__host__ __device__ constexpr int blk_cout(int k) { return (k & 1) ? 48 : 32; }

// matrix-core 3 x 3 layers: 2 k + {0 conv1, 1 conv2} of block k; 8, 9, 10: decode4, decode3, decode2
struct Layer {
  int cin, cout;
};
__host__ __device__ constexpr Layer layer_of(int l) {
  return l < 8 ? Layer{blk_c(l >> 1) * (1 + (l & 1)), blk_c(l >> 1)} : l == 8 ? Layer{ENC, 64} : l == 9 ? Layer{64, 32} : Layer{32, 16};
}
__host__ __device__ constexpr Plan plan_of(int l, bool transposed) {
  return transposed ? plan_for(layer_of(l).cin, layer_of(l).cout, 9) : plan_for(layer_of(l).cout, layer_of(l).cin, 9);
}
__host__ __device__ constexpr Plan tail_plan(int k, bool transposed) {
  return transposed ? plan_for(4 * blk_c(k), blk_cout(k), 1) : plan_for(blk_cout(k), 4 * blk_c(k), 1);
}

// packed weights, offsets in floats (all multiples of 4)
constexpr int PK_STEM = 0;                       // per stream [tap 9][co 16], then the bias [16]
constexpr int PK_HEAD_W = 2 * 160;               // [tap 9][ci 16]
constexpr int PK_HEAD_B = PK_HEAD_W + 144;       // [1], padded to 4
constexpr int PK_DW = PK_HEAD_B + 4;             // per block: convx [tap 9][C], convy [tap 9][C]
__host__ __device__ constexpr size_t dw_off(int k) {
  size_t o = PK_DW;
  for (int i = 0; i < k; ++i) o += 18 * blk_c(i);
  return o;
}
constexpr size_t PK_BIAS = dw_off(4);            // layers 0..10, then per block convdown.bias, convup.bias
__host__ __device__ constexpr size_t bias_off(int l) {
  size_t o = PK_BIAS;
  for (int i = 0; i < l; ++i) o += layer_of(i).cout;
  return o;
}
__host__ __device__ constexpr size_t tail_bias_off(int k, int up) {
  size_t o = bias_off(11);
  for (int i = 0; i < k; ++i) o += 2 * blk_cout(i);
  return o + (up ? blk_cout(k) : 0);
}
constexpr size_t PK_OPS = tail_bias_off(4, 0);
__host__ __device__ constexpr size_t ops_off(int l, bool transposed) {   // layers 0..10 forward, then transposed; l = 11: the end
  size_t o = PK_OPS;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 11; ++i) {
      if (t == (int)transposed && i == l) return o;
      o += plan_of(i, t != 0).floats();
    }
  return o;
}
__host__ __device__ constexpr size_t tail_ops_off(int k, bool transposed) {
  size_t o = ops_off(11, true);
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 4; ++i) {
      if (t == (int)transposed && i == k) return o;
      o += tail_plan(i, t != 0).floats();
    }
  return o;
}
constexpr size_t PK_FLOATS = tail_ops_off(4, true);
static_assert(PK_DW % 4 == 0 && PK_BIAS % 4 == 0 && PK_OPS % 4 == 0, "float4 loads from the pack stay aligned");

// ---- weight packing -----------------------------------------------------------------------------------------------------------------
// the vector-unit weights: [c][tap] -> [tap][c] (stem: c = co; head: c = ci; depthwise: c = channel), and a bias as it is
__global__ void pack_small_k(const float* __restrict__ w, int C, float* __restrict__ pw, const float* __restrict__ b, int nb, float* __restrict__ pb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (w && i < 9 * C) pw[i] = w[(i % C) * 9 + i / C];
  if (b && i < nb) pb[i] = b[i];
}

// ---- the stems: 1 -> 16, bias, LeakyReLU(0.2), into channels [0, 16) of slab1.  One pixel per thread, weights through the scalar cache ------
__global__ __launch_bounds__(256) void stem_fwd_k(const float* __restrict__ x, size_t sb, const float* __restrict__ pw, float* __restrict__ slab, int H,
                                                  int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), xx = (int)(i - b * hw - (size_t)y * W);
  const float* __restrict__ src = x + b * sb;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
#pragma unroll 1   // 16 weights in scalar registers at a time
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = xx + tap % 3 - 1;
    const float v =((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) ? src[(size_t)gy * W + gx] : 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = fmaf(pw[tap * 16 + c], v, acc[c]);
  }
  const float* __restrict__ bs = pw + 144;
  float* o = slab + i * 64;
#pragma unroll
  for (int c = 0; c < 16; c += 4)
    *reinterpret_cast<float4*>(o + c) = make_float4(leaky(acc[c] + bs[c], SLOPE), leaky(acc[c + 1] + bs[c + 1], SLOPE),
                                                    leaky(acc[c + 2] + bs[c + 2], SLOPE), leaky(acc[c + 3] + bs[c + 3], SLOPE));
}

// Reverse: dz = d_slab[0:16] * mask; d_x[p] = sum over tap, co of W[co][tap] * dz[p - (tap - centre)][co]
__global__ __launch_bounds__(256) void stem_bwd_k(const float* __restrict__ pw, const float* __restrict__ slab, const float* __restrict__ dslab,
                                                  float* __restrict__ dx, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y - (tap / 3 - 1), gx = x - (tap % 3 - 1);
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const size_t o = ((size_t)b * hw + (size_t)gy * W + gx) * 64;
    const float* __restrict__ wt = pw + tap * 16;
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
      const float4 z = dleaky4(*reinterpret_cast<const float4*>(slab + o + c), *reinterpret_cast<const float4*>(dslab + o + c), SLOPE);
      s = fmaf(wt[c], z.x, s), s = fmaf(wt[c + 1], z.y, s), s = fmaf(wt[c + 2], z.z, s), s = fmaf(wt[c + 3], z.w, s);
    }
  }
  dx[i] = s;
}

// ---- the depthwise pair: g = |convx(x)| + |convy(x)| of channels [0, C) into [3C, 4C) of the same slab; one thread per pixel and channel
// quad.  sgn: per element (sign(convx) + 1) | (sign(convy) + 1) << 2, four channels in one 32-bit store ------------------------------------
__device__ __forceinline__ unsigned sgn_code(float gx, float gy) {
  return (unsigned)((gx > 0.f) - (gx < 0.f) + 1) | ((unsigned)((gy > 0.f) - (gy < 0.f) + 1) << 2);
}
__global__ __launch_bounds__(256) void sobel_fwd_k(const float* __restrict__ pw, float* slab, uint8_t* __restrict__ sgn, int C, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int nq = C >> 2, cs = 4 * C;
  const size_t pix = i / nq;
  const int c = 4 * (int)(i - pix * nq);
  if (pix >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(pix / hw), y = (int)((pix - b * hw) / W), x = (int)(pix - b * hw - (size_t)y * W);
  float4 gx = make_float4(0.f, 0.f, 0.f, 0.f), gy = gx;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
    const float4 v = *reinterpret_cast<const float4*>(slab + ((size_t)b * hw + (size_t)yy * W + xx) * cs + c);
    const float4 wx = *reinterpret_cast<const float4*>(pw + tap * C + c), wy = *reinterpret_cast<const float4*>(pw + (9 + tap) * C + c);
    gx.x = fmaf(wx.x, v.x, gx.x), gx.y = fmaf(wx.y, v.y, gx.y), gx.z = fmaf(wx.z, v.z, gx.z), gx.w = fmaf(wx.w, v.w, gx.w);
    gy.x = fmaf(wy.x, v.x, gy.x), gy.y = fmaf(wy.y, v.y, gy.y), gy.z = fmaf(wy.z, v.z, gy.z), gy.w = fmaf(wy.w, v.w, gy.w);
  }
  *reinterpret_cast<float4*>(slab + pix * cs + 3 * C + c) =
      make_float4(fabsf(gx.x) + fabsf(gy.x), fabsf(gx.y) + fabsf(gy.y), fabsf(gx.z) + fabsf(gy.z), fabsf(gx.w) + fabsf(gy.w));
  *reinterpret_cast<unsigned*>(sgn + pix * C + c) =
      sgn_code(gx.x, gy.x) | (sgn_code(gx.y, gy.y) << 8) | (sgn_code(gx.z, gy.z) << 16) | (sgn_code(gx.w, gy.w) << 24);
}

// Reverse: d_x[p][c] += sum over tap of (wx[c][tap] * sx + wy[c][tap] * sy)[p - (tap - centre)] * d_g[p - (tap - centre)][c]: reads [3C, 4C)
// of d_slab, adds into [0, C)
__device__ __forceinline__ float sgn_term(float wx, float wy, float dg, unsigned code, float s) {
  const float sx = (float)((int)(code & 3u) - 1), sy = (float)((int)((code >> 2) & 3u) - 1);
  return fmaf(wy, dg * sy, fmaf(wx, dg * sx, s));
}
__global__ __launch_bounds__(256) void sobel_bwd_k(const float* __restrict__ pw, const uint8_t* __restrict__ sgn, float* dslab, int C, int H, int W,
                                                   size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  const int nq = C >> 2, cs = 4 * C;
  const size_t pix = i / nq;
  const int c = 4 * (int)(i - pix * nq);
  if (pix >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(pix / hw), y = (int)((pix - b * hw) / W), x = (int)(pix - b * hw - (size_t)y * W);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int yy = y - (tap / 3 - 1), xx = x - (tap % 3 - 1);
    if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
    const size_t o = (size_t)b * hw + (size_t)yy * W + xx;
    const float4 dg = *reinterpret_cast<const float4*>(dslab + o * cs + 3 * C + c);
    const unsigned code = *reinterpret_cast<const unsigned*>(sgn + o * C + c);
    const float4 wx = *reinterpret_cast<const float4*>(pw + tap * C + c), wy = *reinterpret_cast<const float4*>(pw + (9 + tap) * C + c);
    s.x = sgn_term(wx.x, wy.x, dg.x, code, s.x), s.y = sgn_term(wx.y, wy.y, dg.y, code >> 8, s.y);
    s.z = sgn_term(wx.z, wy.z, dg.z, code >> 16, s.z), s.w = sgn_term(wx.w, wy.w, dg.w, code >> 24, s.w);
  }
  float4* o = reinterpret_cast<float4*>(dslab + pix * cs + c);   // owned by this thread
  const float4 u = *o;
  *o = make_float4(u.x + s.x, u.y + s.y, u.z + s.z, u.w + s.w);
}

// ---- decode1: 16 -> 1, bias, tanh / 2 + 0.5.  One pixel per thread ------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_k(const float* __restrict__ pack, const float* __restrict__ dec2, float* __restrict__ out, int H, int W,
                                                  size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const float* __restrict__ src = dec2 + ((size_t)b * hw + (size_t)gy * W + gx) * 16;
    const float* __restrict__ wt = pack + PK_HEAD_W + tap * 16;
#pragma unroll
    for (int c = 0; c < 16; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(src + c);
      s = fmaf(wt[c], v.x, s), s = fmaf(wt[c + 1], v.y, s), s = fmaf(wt[c + 2], v.z, s), s = fmaf(wt[c + 3], v.w, s);
    }
  }
  out[i] = tanhf(s + pack[PK_HEAD_B]) * 0.5f + 0.5f;
}

// Reverse: with t = 2 f - 1 the taped tanh, dy = g * 0.5 * (1 - t^2); d_dec2[p][ci] = sum over tap of W[ci][tap] * dy[p - (tap - centre)].
// Four lanes per pixel, one channel quad each; WRITES d_dec2.
__global__ __launch_bounds__(256) void head_bwd_k(const float* __restrict__ pack, const float* __restrict__ out, const float* __restrict__ g,
                                                  float* __restrict__ ddec2, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int cq = threadIdx.x & 3;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y - (tap / 3 - 1), gx = x - (tap % 3 - 1);
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const size_t o = (size_t)b * hw + (size_t)gy * W + gx;
    const float t = 2.f * out[o] - 1.f, dy = g[o] * (0.5f * ((1.f - t) * (1.f + t)));
    const float4 wv = *reinterpret_cast<const float4*>(pack + PK_HEAD_W + tap * 16 + 4 * cq);
    s.x = fmaf(wv.x, dy, s.x), s.y = fmaf(wv.y, dy, s.y), s.z = fmaf(wv.z, dy, s.z), s.w = fmaf(wv.w, dy, s.w);
  }
  *reinterpret_cast<float4*>(ddec2 + i * 16 + 4 * cq) = s;
}

}  // namespace

extern "C" size_t paif_seafusion_pack_floats(void) { return PK_FLOATS; }

extern "C" int paif_seafusion_pack_conv(const float* w, const float* b, int conv, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && pack, PAIF_EINVAL, "seafusion_pack_conv: null pointer");
  PAIF_REQUIRE(conv >= 0 && conv <= 29, PAIF_EINVAL, "seafusion_pack_conv: conv %d outside [0, 29]", conv);
  const hipStream_t s = paif::as_stream(stream);
  const int st = conv / 13, j = conv % 13, r = (j - 1) / 6, t = (j - 1) % 6, k = 2 * st + r;   // conv < 26: stream, RGBD, member
  const bool depthwise = conv < 26 && j > 0 && (t == 3 || t == 4);
  PAIF_REQUIRE(depthwise == (b == nullptr), PAIF_EINVAL, "seafusion_pack_conv: a bias is expected for every conv but the depthwise ones");
  const dim3 g2(2), th(256);
  if (conv == 29) {
    hipLaunchKernelGGL(pack_small_k, g2, th, 0, s, w, 16, pack + PK_HEAD_W, b, 1, pack + PK_HEAD_B);
  } else if (conv >= 26 || (j > 0 && t < 2)) {   // a matrix-core 3 x 3
    const int l = conv >= 26 ? 8 + (conv - 26) : 2 * k + t;
    const Layer y = layer_of(l);
    hipLaunchKernelGGL(pack_small_k, g2, th, 0, s, (const float*)nullptr, 0, (float*)nullptr, b, y.cout, pack + bias_off(l));
    for (int tr = 0; tr < 2; ++tr) pack_ops(w, y.cout, y.cin, 0, plan_of(l, tr != 0), tr, pack + ops_off(l, tr != 0), s);
  } else if (j == 0) {
    hipLaunchKernelGGL(pack_small_k, g2, th, 0, s, w, 16, pack + PK_STEM + 160 * st, b, 16, pack + PK_STEM + 160 * st + 144);
  } else if (depthwise) {
    hipLaunchKernelGGL(pack_small_k, g2, th, 0, s, w, blk_c(k), pack + dw_off(k) + (t == 4 ? 9 * blk_c(k) : 0), (const float*)nullptr, 0, (float*)nullptr);
  } else {   // convdown: channels [0, 3C) of the tail's concat; convup: [3C, 4C)
    const int C = blk_c(k), up = t == 5;
    hipLaunchKernelGGL(pack_small_k, g2, th, 0, s, (const float*)nullptr, 0, (float*)nullptr, b, blk_cout(k), pack + tail_bias_off(k, up));
    for (int tr = 0; tr < 2; ++tr)
      pack_ops(w, blk_cout(k), up ? C : 3 * C, up ? 3 * C : 0, tail_plan(k, tr != 0), tr, pack + tail_ops_off(k, tr != 0), s);
  }
  PAIF_LAUNCH_CHECK("seafusion_pack_conv");
  return 0;
}

extern "C" int paif_seafusion_stem_fwd(const float* x, size_t sb, const float* pack, int stream_id, float* slab1, int B, int H, int W,
                                       paif_stream_t stream) {
  PAIF_REQUIRE(x && pack && slab1, PAIF_EINVAL, "seafusion_stem_fwd: null pointer");
  PAIF_REQUIRE(stream_id == 0 || stream_id == 1, PAIF_EINVAL, "seafusion_stem_fwd: stream %d is neither 0 (vis) nor 1 (inf)", stream_id);
  PAIF_SLAB_SHAPE("seafusion_stem_fwd", 1, "", 31);
  PAIF_REQUIRE((size_t)H * W <= sb, PAIF_EINVAL, "seafusion_stem_fwd: batch stride smaller than a plane");
  hipLaunchKernelGGL(stem_fwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), x, sb, pack + PK_STEM + 160 * stream_id,
                     slab1, H, W, n);
  PAIF_LAUNCH_CHECK("seafusion_stem_fwd");
  return 0;
}

extern "C" int paif_seafusion_conv_fwd(const float* pack, int layer, const float* in, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && out, PAIF_EINVAL, "seafusion_conv_fwd: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 10, PAIF_EINVAL, "seafusion_conv_fwd: layer %d outside [0, 10]", layer);
  PAIF_REQUIRE((layer < 8) == (in == out), PAIF_EINVAL, "seafusion_conv_fwd: a dense conv works inside its slab, a decoder conv from one map to another");
  PAIF_SLAB_SHAPE("seafusion_conv_fwd", 1, "", 31);
  PAIF_SLAB_TILES("seafusion_conv_fwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, false);
  const int C = y.cout;
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = in, a.out = out, a.wpk = pack + ops_off(layer, false), a.bias = pack + bias_off(layer), a.slope = SLOPE;
  a.in_cs = layer < 8 ? 4 * C : y.cin, a.nq = y.cin / 4;
  a.out_cs = layer < 8 ? 4 * C : y.cout, a.out_off = layer < 8 ? C * (1 + (layer & 1)) : 0, a.out_n = y.cout;
  launch_conv<9, false, EPI_ACT>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("seafusion_conv_fwd");
  return 0;
}

extern "C" int paif_seafusion_sobel_fwd(const float* pack, int block, float* slab, void* sgn, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab && sgn, PAIF_EINVAL, "seafusion_sobel_fwd: null pointer");
  PAIF_REQUIRE(block >= 0 && block <= 3, PAIF_EINVAL, "seafusion_sobel_fwd: block %d outside [0, 3]", block);
  PAIF_SLAB_SHAPE("seafusion_sobel_fwd", 1, "", 31);
  const int C = blk_c(block);
  const size_t work = n * (C / 4);
  hipLaunchKernelGGL(sobel_fwd_k, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack + dw_off(block), slab,
                     static_cast<uint8_t*>(sgn), C, H, W, n);
  PAIF_LAUNCH_CHECK("seafusion_sobel_fwd");
  return 0;
}

extern "C" int paif_seafusion_tail_fwd(const float* pack, int block, const float* slab, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab && out, PAIF_EINVAL, "seafusion_tail_fwd: null pointer");
  PAIF_REQUIRE(block >= 0 && block <= 3, PAIF_EINVAL, "seafusion_tail_fwd: block %d outside [0, 3]", block);
  PAIF_REQUIRE(slab != out, PAIF_EINVAL, "seafusion_tail_fwd: the output map must not be the block's own slab");
  PAIF_SLAB_SHAPE("seafusion_tail_fwd", 1, "", 31);
  PAIF_SLAB_TILES("seafusion_tail_fwd");
  const Plan pl = tail_plan(block, false);
  const int C = blk_c(block), r = block & 1;
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = slab, a.out = out, a.wpk = pack + tail_ops_off(block, false);
  a.bias = pack + tail_bias_off(block, 0), a.bias2 = pack + tail_bias_off(block, 1), a.slope = SLOPE_RGBD;
  a.in_cs = 4 * C, a.nq = C;
  a.out_cs = r ? ENC : 128, a.out_off = r ? 48 * (block >> 1) : 0, a.out_n = blk_cout(block);
  launch_conv<1, false, EPI_ACT>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("seafusion_tail_fwd");
  return 0;
}

extern "C" int paif_seafusion_head_fwd(const float* pack, const float* dec2, float* fused, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && dec2 && fused, PAIF_EINVAL, "seafusion_head_fwd: null pointer");
  PAIF_SLAB_SHAPE("seafusion_head_fwd", 1, "", 31);
  hipLaunchKernelGGL(head_fwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack, dec2, fused, H, W, n);
  PAIF_LAUNCH_CHECK("seafusion_head_fwd");
  return 0;
}

extern "C" int paif_seafusion_head_bwd(const float* pack, const float* fused, const float* d_fused, float* d_dec2, int B, int H, int W,
                                       paif_stream_t stream) {
  PAIF_REQUIRE(pack && fused && d_fused && d_dec2, PAIF_EINVAL, "seafusion_head_bwd: null pointer");
  PAIF_SLAB_SHAPE("seafusion_head_bwd", 1, "", 31);
  hipLaunchKernelGGL(head_bwd_k, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, paif::as_stream(stream), pack, fused, d_fused, d_dec2, H, W, n);
  PAIF_LAUNCH_CHECK("seafusion_head_bwd");
  return 0;
}

extern "C" int paif_seafusion_conv_bwd(const float* pack, int layer, const float* taped, const float* d_out, float* d_in, int B, int H, int W,
                                       paif_stream_t stream) {
  PAIF_REQUIRE(pack && taped && d_out && d_in, PAIF_EINVAL, "seafusion_conv_bwd: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 10, PAIF_EINVAL, "seafusion_conv_bwd: layer %d outside [0, 10]", layer);
  PAIF_REQUIRE(taped != d_out && taped != d_in, PAIF_EINVAL, "seafusion_conv_bwd: the gradient maps must not alias the taped maps");
  PAIF_REQUIRE((layer < 8) == (d_out == d_in), PAIF_EINVAL, "seafusion_conv_bwd: a dense conv works inside d_slab, a decoder conv from one map to another");
  PAIF_SLAB_SHAPE("seafusion_conv_bwd", 1, "", 31);
  PAIF_SLAB_TILES("seafusion_conv_bwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, true);
  const int C = y.cout, off = layer < 8 ? C * (1 + (layer & 1)) : 0, cs = layer < 8 ? 4 * C : y.cout;   // where the layer's output lives
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = d_out + off, a.mask = taped + off, a.out = d_in, a.wpk = pack + ops_off(layer, true), a.slope = SLOPE;
  a.in_cs = cs, a.nq = y.cout / 4;
  a.out_cs = layer < 8 ? 4 * C : y.cin, a.out_off = 0, a.out_n = y.cin;
  const dim3 grid = conv_grid(pl, B, tx, ty);
  if (layer < 8) launch_conv<9, true, EPI_ADD>(pl.MB, grid, paif::as_stream(stream), a);   // reads its own slice of d_slab, adds below it
  else launch_conv<9, true, EPI_STORE>(pl.MB, grid, paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("seafusion_conv_bwd");
  return 0;
}

extern "C" int paif_seafusion_tail_bwd(const float* pack, int block, const float* taped_out, const float* d_out, float* d_slab, int B, int H, int W,
                                       paif_stream_t stream) {
  PAIF_REQUIRE(pack && taped_out && d_out && d_slab, PAIF_EINVAL, "seafusion_tail_bwd: null pointer");
  PAIF_REQUIRE(block >= 0 && block <= 3, PAIF_EINVAL, "seafusion_tail_bwd: block %d outside [0, 3]", block);
  PAIF_REQUIRE(d_out != d_slab && taped_out != d_slab && taped_out != d_out, PAIF_EINVAL, "seafusion_tail_bwd: three different maps are expected");
  PAIF_SLAB_SHAPE("seafusion_tail_bwd", 1, "", 31);
  PAIF_SLAB_TILES("seafusion_tail_bwd");
  const Plan pl = tail_plan(block, true);
  const int C = blk_c(block), r = block & 1, off = r ? 48 * (block >> 1) : 0;
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = d_out + off, a.mask = taped_out + off, a.out = d_slab, a.wpk = pack + tail_ops_off(block, true), a.slope = SLOPE_RGBD;
  a.in_cs = r ? ENC : 128, a.nq = blk_cout(block) / 4;
  a.out_cs = 4 * C, a.out_off = 0, a.out_n = 4 * C;
  launch_conv<1, true, EPI_STORE>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("seafusion_tail_bwd");
  return 0;
}

extern "C" int paif_seafusion_sobel_bwd(const float* pack, int block, const void* sgn, float* d_slab, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && sgn && d_slab, PAIF_EINVAL, "seafusion_sobel_bwd: null pointer");
  PAIF_REQUIRE(block >= 0 && block <= 3, PAIF_EINVAL, "seafusion_sobel_bwd: block %d outside [0, 3]", block);
  PAIF_SLAB_SHAPE("seafusion_sobel_bwd", 1, "", 31);
  const int C = blk_c(block);
  const size_t work = n * (C / 4);
  hipLaunchKernelGGL(sobel_bwd_k, dim3((unsigned)((work + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack + dw_off(block),
                     static_cast<const uint8_t*>(sgn), d_slab, C, H, W, n);
  PAIF_LAUNCH_CHECK("seafusion_sobel_bwd");
  return 0;
}

extern "C" int paif_seafusion_stem_bwd(const float* pack, int stream_id, const float* slab1, const float* d_slab1, float* d_x, int B, int H, int W,
                                       paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab1 && d_slab1 && d_x, PAIF_EINVAL, "seafusion_stem_bwd: null pointer");
  PAIF_REQUIRE(stream_id == 0 || stream_id == 1, PAIF_EINVAL, "seafusion_stem_bwd: stream %d is neither 0 (vis) nor 1 (inf)", stream_id);
  PAIF_SLAB_SHAPE("seafusion_stem_bwd", 1, "", 31);
  hipLaunchKernelGGL(stem_bwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack + PK_STEM + 160 * stream_id, slab1,
                     d_slab1, d_x, H, W, n);
  PAIF_LAUNCH_CHECK("seafusion_stem_bwd");
  return 0;
}
