// The hand-designed fusion network of the reference (core/model_fusion_auto.py:118-188): Fusion_Network over two DRDB blocks.
//   conv1 3 x 3 2 -> 64 on cat(ir, vis), PReLU; DRDB1; DRDB2; conv2 3 x 3 64 -> 32, PReLU; conv21 3 x 3 32 -> 1, PReLU = f;
//   c = clamp(f, 0, 1); fused = (c - min c) / (max c - min c), min and max over the whole batch.
// DRDB(64, 32): x_k = ReLU(Dcov_k 3 x 3, dilation 2, pad 2 (cat(x, x_1 .. x_{k-1}))) for k = 1..5 (32 channels each), then
//   out = x + ReLU(conv 1 x 1 224 -> 64 (cat(x, x_1 .. x_5))).  ONE PReLU slope serves the three places; it is an argument (read on the host).
// Forward and the reverse pass (input gradients).  The clamp and the batch min / max normalisation, forward and reverse, are the plane
// kernels of object_glue.hip (paif_plane_clamp_minmax_*): f is taped BEFORE the clamp, every branch of the tail is read off it.
//
// LAYOUT.  fp32 NHWC.  One slab [B][H][W][224] per DRDB: x in [0, 64), x_k in [64 + 32 (k - 1), 64 + 32 k).  Dcov_k reads [0, 64 + 32 (k - 1))
// and writes the 32 channels behind them: the concats are channel ranges, nothing is copied, no launch reads channels it writes.  The
// 1 x 1 reads all 224 channels and writes x + r, r = ReLU(v + b), into [0, 64) of the NEXT map (DRDB2's slab, or the 64-channel map conv2
// reads); r itself is taped as r6 [B][H][W][64]: the reverse pass must not recover the branch from out - x (x + r can equal x in fp32).
// c2 [B][H][W][32] is conv2's map, f [B][H][W] conv21's.  Gradient buffers use the layouts of their maps.
//
// The 3 x 3 (dilated or not) and 1 x 1 convs with 32 or more input channels run on the matrix core (conv_slab.h); conv1, conv21 and their
// transposes run on the vector unit.  Summation order: chunks, taps, k ascending; no atomics; every output element is owned by one lane.
//
// REVERSE ORDER per DRDB: the 1 x 1 transpose STORES all 224 channels of d_slab (input d_out masked by the taped r6, slope 0), the residual
// then ADDS d_out onto [0, 64); Dcov_5 .. Dcov_1 transposed read their own 32 channels of d_slab (masked by the taped x_k) and ADD into
// the channels below.  [0, 64) of DRDB2's d_slab is DRDB1's d_out.
#include <math.h>
#include <stdint.h>

#include "conv_slab.h"

namespace {

using namespace paif_slab;

constexpr int SLAB = 224, CX = 64, GROW = 32;

// matrix-core layers: 6 * block + j, j = 0..4: Dcov_{j+1}, j = 5: the block's 1 x 1; 12: conv2
struct Layer {
  int cin, cout, taps;
};
__host__ __device__ constexpr Layer layer_of(int l) {
  return l == 12 ? Layer{CX, 32, 9} : (l % 6 == 5 ? Layer{SLAB, CX, 1} : Layer{CX + GROW * (l % 6), GROW, 9});
}
__host__ __device__ constexpr Plan plan_of(int l, bool transposed) {
  return transposed ? plan_for(layer_of(l).cin, layer_of(l).cout, layer_of(l).taps) : plan_for(layer_of(l).cout, layer_of(l).cin, layer_of(l).taps);
}

// packed weights, offsets in floats (all multiples of 4)
constexpr int PK_STEM_W = 0;                      // [tap 9][ci 2][co 64]
constexpr int PK_STEM_B = PK_STEM_W + 9 * 2 * 64;  // [64]
constexpr int PK_HEAD_W = PK_STEM_B + 64;         // [tap 9][ci 32]
constexpr int PK_HEAD_B = PK_HEAD_W + 9 * 32;     // [1], padded to 4
constexpr int PK_BIAS = PK_HEAD_B + 4;            // layers 0..12
__host__ __device__ constexpr size_t bias_off(int l) {
  size_t o = PK_BIAS;
  for (int i = 0; i < l; ++i) o += layer_of(i).cout;
  return o;
}
constexpr size_t PK_OPS = bias_off(13);
__host__ __device__ constexpr size_t ops_off(int l, bool transposed) {   // layers 0..12 forward, then transposed; l = 13: the end
  size_t o = PK_OPS;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 13; ++i) {
      if (t == (int)transposed && i == l) return o;
      o += plan_of(i, t != 0).floats();
    }
  return o;
}
constexpr size_t PK_FLOATS = ops_off(13, true);
static_assert(PK_HEAD_W % 4 == 0 && PK_BIAS % 4 == 0 && PK_OPS % 4 == 0, "float4 loads from the pack stay aligned");
static_assert(PK_HEAD_B == PK_HEAD_W + 9 * 32, "head32_*_k read the bias behind the weights");

// ---- weight packing -----------------------------------------------------------------------------------------------------------------
// a vector-unit weight [co][ci][tap] -> [tap][ci][co] (conv1: ci 2, co 64; conv21: ci 32, co 1), and a bias as it is
__global__ void pack_small_k(const float* __restrict__ w, int co, int ci, float* __restrict__ pw, const float* __restrict__ b, int nb,
                             float* __restrict__ pb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (w && i < 9 * ci * co) {
    const int c = i % co, k = (i / co) % ci, tap = i / (co * ci);
    pw[i] = w[((size_t)c * ci + k) * 9 + tap];
  }
  if (b && i < nb) pb[i] = b[i];
}

// ---- conv1: 2 -> 64, bias, PReLU, into channels [0, 64) of DRDB1's slab.  One pixel per thread, 16 output channels per blockIdx.y: the
// weights go through the scalar cache.  The two planes are read where they lie (no cat) ----------------------------------------------------
__global__ __launch_bounds__(256) void stem_fwd_k(const float* __restrict__ ir, size_t sb_ir, const float* __restrict__ vis, size_t sb_vis,
                                                  const float* __restrict__ pack, float slope, float* __restrict__ slab, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int c0 = 16 * blockIdx.y;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  const float* __restrict__ p0 = ir + b * sb_ir;
  const float* __restrict__ p1 = vis + b * sb_vis;
  const float* __restrict__ pw = pack + PK_STEM_W + c0;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
#pragma unroll 1   // 32 weights in scalar registers at a time
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
    const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    const float v0 = in ? p0[(size_t)gy * W + gx] : 0.f, v1 = in ? p1[(size_t)gy * W + gx] : 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = fmaf(pw[(tap * 2 + 1) * 64 + c], v1, fmaf(pw[tap * 2 * 64 + c], v0, acc[c]));
  }
  const float* __restrict__ bs = pack + PK_STEM_B + c0;
  float* o = slab + i * SLAB + c0;
#pragma unroll
  for (int c = 0; c < 16; c += 4)
    *reinterpret_cast<float4*>(o + c) = make_float4(leaky(acc[c] + bs[c], slope), leaky(acc[c + 1] + bs[c + 1], slope),
                                                    leaky(acc[c + 2] + bs[c + 2], slope), leaky(acc[c + 3] + bs[c + 3], slope));
}

// Reverse: dz = d_slab[0:64] through the PReLU (branch from the taped slab); d_plane[ci][p] = sum over tap, co of W[co][ci][tap] *
// dz[p - (tap - centre)][co].  One pixel per thread, both planes.
__global__ __launch_bounds__(256) void stem_bwd_k(const float* __restrict__ pack, float slope, const float* __restrict__ slab,
                                                  const float* __restrict__ dslab, float* __restrict__ d_ir, float* __restrict__ d_vis, int H, int W,
                                                  size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s0 = 0.f, s1 = 0.f;
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y - (tap / 3 - 1), gx = x - (tap % 3 - 1);
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const size_t o = ((size_t)b * hw + (size_t)gy * W + gx) * SLAB;
    const float* __restrict__ w0 = pack + PK_STEM_W + tap * 2 * 64;
    const float* __restrict__ w1 = w0 + 64;
#pragma unroll 4
    for (int c = 0; c < CX; c += 4) {
      const float4 z = dleaky4(*reinterpret_cast<const float4*>(slab + o + c), *reinterpret_cast<const float4*>(dslab + o + c), slope);
      s0 = fmaf(w0[c], z.x, s0), s0 = fmaf(w0[c + 1], z.y, s0), s0 = fmaf(w0[c + 2], z.z, s0), s0 = fmaf(w0[c + 3], z.w, s0);
      s1 = fmaf(w1[c], z.x, s1), s1 = fmaf(w1[c + 1], z.y, s1), s1 = fmaf(w1[c + 2], z.z, s1), s1 = fmaf(w1[c + 3], z.w, s1);
    }
  }
  d_ir[i] = s0;
  d_vis[i] = s1;
}

// conv21 (32 -> 1, bias, PReLU -> f, BEFORE the clamp) and its reverse (branch from the taped f) are head32_fwd_k / head32_bwd_k<ACT_LEAKY>
// of conv_slab.h.

// ---- the residual of a DRDB in reverse: d_slab[0:64] += d_out.  Sixteen lanes per pixel, one channel quad each ---------------------------
__global__ __launch_bounds__(256) void resid_add_k(const float* __restrict__ d_out, int cs, float* __restrict__ dslab, size_t n) {
  const size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int c = 4 * (threadIdx.x & 15);
  if (i >= n) return;
  const float4 g = *reinterpret_cast<const float4*>(d_out + i * cs + c);
  float4* o = reinterpret_cast<float4*>(dslab + i * SLAB + c);   // owned by this lane
  const float4 u = *o;
  *o = make_float4(u.x + g.x, u.y + g.y, u.z + g.z, u.w + g.w);
}

// the dilation-2 3 x 3 forms
template <bool MASK, int EPI>
void launch_dil2(int MB, dim3 grid, hipStream_t s, const ConvArgs& a) {
  if (MB == 4) hipLaunchKernelGGL((conv_k<9, 4, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL_NONE, 2>), grid, dim3(256), 0, s, a);
  else if (MB == 3) hipLaunchKernelGGL((conv_k<9, 3, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL_NONE, 2>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_k<9, 2, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL_NONE, 2>), grid, dim3(256), 0, s, a);
}

}  // namespace

extern "C" size_t paif_drdb_pack_floats(void) { return PK_FLOATS; }

extern "C" int paif_drdb_pack_conv(const float* w, const float* b, int conv, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && pack, PAIF_EINVAL, "drdb_pack_conv: null pointer");
  PAIF_REQUIRE(conv >= 0 && conv <= 14, PAIF_EINVAL, "drdb_pack_conv: conv %d outside [0, 14]", conv);
  const hipStream_t s = paif::as_stream(stream);
  const dim3 th(256);
  if (conv == 0) {
    hipLaunchKernelGGL(pack_small_k, dim3(5), th, 0, s, w, 64, 2, pack + PK_STEM_W, b, 64, pack + PK_STEM_B);
  } else if (conv == 14) {
    hipLaunchKernelGGL(pack_small_k, dim3(2), th, 0, s, w, 1, 32, pack + PK_HEAD_W, b, 1, pack + PK_HEAD_B);
  } else {
    const int l = conv - 1;
    const Layer y = layer_of(l);
    hipLaunchKernelGGL(pack_small_k, dim3(1), th, 0, s, (const float*)nullptr, 0, 0, (float*)nullptr, b, y.cout, pack + bias_off(l));
    for (int tr = 0; tr < 2; ++tr) pack_ops(w, y.cout, y.cin, 0, plan_of(l, tr != 0), tr, pack + ops_off(l, tr != 0), s);
  }
  PAIF_LAUNCH_CHECK("drdb_pack_conv");
  return 0;
}

#define DRDB_BLOCK(name) PAIF_REQUIRE(block == 0 || block == 1, PAIF_EINVAL, name ": block %d is neither 0 (DRDB1) nor 1 (DRDB2)", block)
#define DRDB_SLOPE(name) PAIF_REQUIRE(slope >= 0.f, PAIF_EINVAL, name ": the PReLU slope %g is negative (the branch is read off the taped output)", (double)slope)

extern "C" int paif_drdb_stem_fwd(const float* ir, size_t sb_ir, const float* vis, size_t sb_vis, const float* pack, float slope, float* slab,
                                  int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(ir && vis && pack && slab, PAIF_EINVAL, "drdb_stem_fwd: null pointer");
  DRDB_SLOPE("drdb_stem_fwd");
  PAIF_SLAB_SHAPE("drdb_stem_fwd", 1, "", 31);
  PAIF_REQUIRE((size_t)H * W <= sb_ir && (size_t)H * W <= sb_vis, PAIF_EINVAL, "drdb_stem_fwd: batch stride smaller than a plane");
  hipLaunchKernelGGL(stem_fwd_k, dim3((unsigned)((n + 255) / 256), 4), dim3(256), 0, paif::as_stream(stream), ir, sb_ir, vis, sb_vis, pack, slope,
                     slab, H, W, n);
  PAIF_LAUNCH_CHECK("drdb_stem_fwd");
  return 0;
}

extern "C" int paif_drdb_dcov_fwd(const float* pack, int block, int k, float* slab, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab, PAIF_EINVAL, "drdb_dcov_fwd: null pointer");
  DRDB_BLOCK("drdb_dcov_fwd");
  PAIF_REQUIRE(k >= 1 && k <= 5, PAIF_EINVAL, "drdb_dcov_fwd: Dcov%d does not exist", k);
  PAIF_SLAB_SHAPE("drdb_dcov_fwd", 1, "", 31);
  PAIF_SLAB_TILES("drdb_dcov_fwd");
  const int l = 6 * block + k - 1;
  const Layer y = layer_of(l);
  const Plan pl = plan_of(l, false);
  ConvArgs a = conv_args(pl, H, W, tx, ty);   // slope 0: ReLU
  a.in = slab, a.out = slab, a.wpk = pack + ops_off(l, false), a.bias = pack + bias_off(l);
  a.in_cs = SLAB, a.nq = y.cin / 4;
  a.out_cs = SLAB, a.out_off = y.cin, a.out_n = GROW;
  launch_dil2<false, EPI_ACT>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("drdb_dcov_fwd");
  return 0;
}

extern "C" int paif_drdb_tail_fwd(const float* pack, int block, const float* slab, float* out, int out_cs, float* r6, int B, int H, int W,
                                  paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab && out && r6, PAIF_EINVAL, "drdb_tail_fwd: null pointer");
  DRDB_BLOCK("drdb_tail_fwd");
  PAIF_REQUIRE(out_cs == SLAB || out_cs == CX, PAIF_EINVAL, "drdb_tail_fwd: the output is a 224-channel slab or a 64-channel map, not %d", out_cs);
  PAIF_REQUIRE(slab != out && slab != r6 && out != r6, PAIF_EINVAL, "drdb_tail_fwd: three different maps are expected");
  PAIF_SLAB_SHAPE("drdb_tail_fwd", 1, "", 31);
  PAIF_SLAB_TILES("drdb_tail_fwd");
  const int l = 6 * block + 5;
  const Plan pl = plan_of(l, false);
  ConvArgs a = conv_args(pl, H, W, tx, ty);   // slope 0: ReLU
  a.in = slab, a.out = out, a.wpk = pack + ops_off(l, false), a.bias = pack + bias_off(l);
  a.in_cs = SLAB, a.nq = SLAB / 4;
  a.out_cs = out_cs, a.out_off = 0, a.out_n = CX;
  a.avg = r6, a.avg_cs = CX, a.avg_off = 0;
  static_assert(plan_of(5, false).MB == 4 && plan_of(5, false).groups == 1, "64 output channels in one group");
  hipLaunchKernelGGL((conv_k<1, 4, false, EPI_RES>), dim3((unsigned)(tx * ty * B), 1), dim3(256), 0, paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("drdb_tail_fwd");
  return 0;
}

extern "C" int paif_drdb_conv2_fwd(const float* pack, float slope, const float* in, float* c2, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && c2 && in != c2, PAIF_EINVAL, "drdb_conv2_fwd: null or aliased pointer");
  DRDB_SLOPE("drdb_conv2_fwd");
  PAIF_SLAB_SHAPE("drdb_conv2_fwd", 1, "", 31);
  PAIF_SLAB_TILES("drdb_conv2_fwd");
  const Plan pl = plan_of(12, false);
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = in, a.out = c2, a.wpk = pack + ops_off(12, false), a.bias = pack + bias_off(12), a.slope = slope;
  a.in_cs = CX, a.nq = CX / 4;
  a.out_cs = 32, a.out_off = 0, a.out_n = 32;
  launch_conv<9, false, EPI_ACT>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("drdb_conv2_fwd");
  return 0;
}

extern "C" int paif_drdb_head_fwd(const float* pack, float slope, const float* c2, float* f, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && c2 && f, PAIF_EINVAL, "drdb_head_fwd: null pointer");
  DRDB_SLOPE("drdb_head_fwd");
  PAIF_SLAB_SHAPE("drdb_head_fwd", 1, "", 31);
  hipLaunchKernelGGL(head32_fwd_k<ACT_LEAKY>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack + PK_HEAD_W, slope, c2, f,
                     H, W, n);
  PAIF_LAUNCH_CHECK("drdb_head_fwd");
  return 0;
}

extern "C" int paif_drdb_head_bwd(const float* pack, float slope, const float* f, const float* d_f, float* d_c2, int B, int H, int W,
                                  paif_stream_t stream) {
  PAIF_REQUIRE(pack && f && d_f && d_c2, PAIF_EINVAL, "drdb_head_bwd: null pointer");
  DRDB_SLOPE("drdb_head_bwd");
  PAIF_SLAB_SHAPE("drdb_head_bwd", 1, "", 31);
  hipLaunchKernelGGL(head32_bwd_k<ACT_LEAKY>, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, paif::as_stream(stream), pack + PK_HEAD_W, slope, f, d_f,
                     d_c2, H, W, n);
  PAIF_LAUNCH_CHECK("drdb_head_bwd");
  return 0;
}

extern "C" int paif_drdb_conv2_bwd(const float* pack, float slope, const float* c2, const float* d_c2, float* d_in, int B, int H, int W,
                                   paif_stream_t stream) {
  PAIF_REQUIRE(pack && c2 && d_c2 && d_in, PAIF_EINVAL, "drdb_conv2_bwd: null pointer");
  PAIF_REQUIRE(c2 != d_c2 && c2 != d_in && d_c2 != d_in, PAIF_EINVAL, "drdb_conv2_bwd: three different maps are expected");
  DRDB_SLOPE("drdb_conv2_bwd");
  PAIF_SLAB_SHAPE("drdb_conv2_bwd", 1, "", 31);
  PAIF_SLAB_TILES("drdb_conv2_bwd");
  const Plan pl = plan_of(12, true);
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = d_c2, a.mask = c2, a.out = d_in, a.wpk = pack + ops_off(12, true), a.slope = slope;
  a.in_cs = 32, a.nq = 8;
  a.out_cs = CX, a.out_off = 0, a.out_n = CX;
  launch_conv<9, true, EPI_STORE>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("drdb_conv2_bwd");
  return 0;
}

extern "C" int paif_drdb_tail_bwd(const float* pack, int block, const float* r6, const float* d_out, int d_out_cs, float* d_slab, int B, int H, int W,
                                  paif_stream_t stream) {
  PAIF_REQUIRE(pack && r6 && d_out && d_slab, PAIF_EINVAL, "drdb_tail_bwd: null pointer");
  DRDB_BLOCK("drdb_tail_bwd");
  PAIF_REQUIRE(d_out_cs == SLAB || d_out_cs == CX, PAIF_EINVAL, "drdb_tail_bwd: d_out is [0, 64) of a 224-channel slab or a 64-channel map, not %d",
               d_out_cs);
  PAIF_REQUIRE(d_out != d_slab && r6 != d_slab && r6 != d_out, PAIF_EINVAL, "drdb_tail_bwd: three different maps are expected");
  PAIF_SLAB_SHAPE("drdb_tail_bwd", 1, "", 31);
  PAIF_SLAB_TILES("drdb_tail_bwd");
  const int l = 6 * block + 5;
  const Plan pl = plan_of(l, true);
  const hipStream_t s = paif::as_stream(stream);
  ConvArgs a = conv_args(pl, H, W, tx, ty);   // slope 0: ReLU
  a.in = d_out, a.mask = r6, a.out = d_slab, a.wpk = pack + ops_off(l, true);
  a.in_cs = d_out_cs, a.mask_cs = CX, a.in_scale = 1.f, a.nq = CX / 4;   // the mask has its own stride: the scaled staging, at scale 1
  a.out_cs = SLAB, a.out_off = 0, a.out_n = SLAB;
  static_assert(plan_of(5, true).MB == 3 && plan_of(5, true).groups == 5, "224 output channels: five groups of three blocks, one block of padding");
  hipLaunchKernelGGL((conv_k<1, 3, true, EPI_STORE, ACT_LEAKY, false, XIN_SCALED>), conv_grid(pl, B, tx, ty), dim3(256), 0, s, a);
  PAIF_LAUNCH_CHECK("drdb_tail_bwd(conv)");
  hipLaunchKernelGGL(resid_add_k, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, s, d_out, d_out_cs, d_slab, n);
  PAIF_LAUNCH_CHECK("drdb_tail_bwd(residual)");
  return 0;
}

extern "C" int paif_drdb_dcov_bwd(const float* pack, int block, int k, const float* slab, float* d_slab, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab && d_slab && slab != d_slab, PAIF_EINVAL, "drdb_dcov_bwd: null or aliased pointer");
  DRDB_BLOCK("drdb_dcov_bwd");
  PAIF_REQUIRE(k >= 1 && k <= 5, PAIF_EINVAL, "drdb_dcov_bwd: Dcov%d does not exist", k);
  PAIF_SLAB_SHAPE("drdb_dcov_bwd", 1, "", 31);
  PAIF_SLAB_TILES("drdb_dcov_bwd");
  const int l = 6 * block + k - 1;
  const Layer y = layer_of(l);
  const Plan pl = plan_of(l, true);
  ConvArgs a = conv_args(pl, H, W, tx, ty);   // slope 0: ReLU
  a.in = d_slab + y.cin, a.mask = slab + y.cin, a.out = d_slab, a.wpk = pack + ops_off(l, true);
  a.in_cs = SLAB, a.nq = GROW / 4;
  a.out_cs = SLAB, a.out_off = 0, a.out_n = y.cin;
  PAIF_REQUIRE(pl.MB >= 3, PAIF_EINVAL, "drdb_dcov_bwd: unexpected plan");
  launch_dil2<true, EPI_ADD>(pl.MB, conv_grid(pl, B, tx, ty), paif::as_stream(stream), a);   // reads its own slice, adds below it
  PAIF_LAUNCH_CHECK("drdb_dcov_bwd");
  return 0;
}

extern "C" int paif_drdb_stem_bwd(const float* pack, float slope, const float* slab, const float* d_slab, float* d_ir, float* d_vis, int B, int H,
                                  int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && slab && d_slab && d_ir && d_vis, PAIF_EINVAL, "drdb_stem_bwd: null pointer");
  DRDB_SLOPE("drdb_stem_bwd");
  PAIF_SLAB_SHAPE("drdb_stem_bwd", 1, "", 31);
  hipLaunchKernelGGL(stem_bwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack, slope, slab, d_slab, d_ir, d_vis, H,
                     W, n);
  PAIF_LAUNCH_CHECK("drdb_stem_bwd");
  return 0;
}
