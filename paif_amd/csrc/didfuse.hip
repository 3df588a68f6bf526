// DIDFuse baseline (reference fusion_model/AUIF.py, class DID).  Per stream s (0: x_over / AE_Encoder1, 1: x_under / AE_Encoder2):
// f1 = PReLU(BN(conv 3 x 3 1 -> 64 of the REFLECTION-padded plane)), f2 = PReLU(BN(conv 3 x 3 64 -> 64, zero pad 1 (f1))),
// fB = tanh(BN(conv 64 -> 64 (f2))), fD = tanh(BN(conv 64 -> 64 (f2))).  The four maps are averaged over the streams; the decoder is
// Out1 = PReLU(BN(conv 128 -> 64 (F_b | F_d))), Out2 = PReLU(BN(conv 128 -> 64 (Out1 | F_2))),
// fused = sigmoid(BN(conv 3 x 3 128 -> 1 of the reflection-padded (Out2 | F_1))).  Every BatchNorm is the eval-mode one and every PReLU has
// one slope.  Forward and the reverse pass (input gradients), ten launches each.
//
// BATCHNORM is folded into the pack by the pack kernel, in fp32 on the device: scale = gamma * rsqrt(var + eps), the packed weight is
// W * scale[co] (forward and transposed operand packs alike), the epilogue bias is beta + (bias - mean) * scale.  No kernel applies a
// BatchNorm at run time.
//
// LAYOUT.  fp32 NHWC.  enc[s][B][H][W][256] = f1 | f2 | fB | fD of stream s; bd[..][128] = F_b | F_d; d1[..][128] = Out1 | F_2;
// d2[..][128] = Out2 | F_1: every concat the decoder reads exists once.  The means are written by the SECOND stream's launches (the pair
// epilogue of conv_slab.h, and the same in the stem): the launch that stores a quad of stream 1 reads stream 0's quad at the same place
// and stores 0.5 (a + b) into the decoder slab.  Gradient buffers: d_d2, d_d1, d_bd [..][128] as their maps; dg [..][128] = d_f1 | d_f2 of
// one stream (d_fB | d_fD = 0.5 d_bd is never stored: the 0.5 is the input scale of cov34's transpose).
//
// MATRIX CORE (conv_slab.h, conv_k<9, 4, ...>): cov2 per stream (64 -> 64), cov3 + cov4 per stream as ONE 64 -> 128 conv (the two weights
// side by side on M), cov5, cov6 (128 -> 64), and their transposes.  VECTOR UNIT: cov1 and cov7 (reflection padding) and their transposes.
//
// REVERSE ORDER.  head' WRITES d_d2; cov6' (mask Out2) WRITES d_d1; cov5' (mask Out1) WRITES d_bd; then per stream: cov34' (tanh mask from
// fB | fD, input scale 0.5) WRITES dg[64:128); cov2' (input dg[64:128) + 0.5 d_d1[64:128), mask f2) WRITES dg[0:64); the stem's transpose
// (input dg[0:64) + 0.5 d_d2[64:128), mask f1) WRITES d_x.  No atomics, no memset, every output element is owned by one lane, no launch
// reads channels it writes, nothing is recomputed.  PReLU'(0) = slope (the branch comes from the taped output: slopes >= 0 only, which the
// module checks when it builds the pack).
#include <math.h>
#include <stdint.h>

#include "conv_slab.h"

namespace {

using namespace paif_slab;

constexpr int ENC = 256, DEC = 128, CH = 64;

// matrix-core layers: 2 s + {0 cov2, 1 cov3 | cov4} of stream s; 4 cov5; 5 cov6
struct Layer {
  int cin, cout;
};
__host__ __device__ constexpr Layer layer_of(int l) { return l < 4 ? Layer{CH, (l & 1) ? 2 * CH : CH} : Layer{2 * CH, CH}; }
__host__ __device__ constexpr Plan plan_of(int l, bool transposed) {
  return transposed ? plan_for(layer_of(l).cin, layer_of(l).cout, 9) : plan_for(layer_of(l).cout, layer_of(l).cin, 9);
}
static_assert(plan_of(0, false).MB == 4 && plan_of(1, false).MB == 4 && plan_of(1, false).groups == 2 && plan_of(4, true).groups == 2 &&
                  plan_of(1, true).MB == 4 && plan_of(1, true).groups == 1,
              "every launch is the MB = 4 form");

// packed weights, offsets in floats (all multiples of 4)
constexpr size_t PK_STEM = 0;                          // per stream [tap 9][co 64] scaled, then the shift [64]
constexpr size_t PK_HEAD_W = 2 * 640;                  // [tap 9][ci 128] scaled
constexpr size_t PK_HEAD_B = PK_HEAD_W + 9 * DEC;      // the shift [1], padded to 4
constexpr size_t PK_BIAS = PK_HEAD_B + 4;              // the shifts of layers 0..5
__host__ __device__ constexpr size_t bias_off(int l) {
  size_t o = PK_BIAS;
  for (int i = 0; i < l; ++i) o += layer_of(i).cout;
  return o;
}
constexpr size_t PK_FOLD = bias_off(6);                // per layer the scaled weight [cout][cin][9] (cov3's rows, then cov4's)
__host__ __device__ constexpr size_t fold_off(int l) {
  size_t o = PK_FOLD;
  for (int i = 0; i < l; ++i) o += (size_t)layer_of(i).cout * layer_of(i).cin * 9;
  return o;
}
constexpr size_t PK_OPS = fold_off(6);
__host__ __device__ constexpr size_t ops_off(int l, bool transposed) {   // layers 0..5 forward, then transposed; l = 6: the end
  size_t o = PK_OPS;
  for (int t = 0; t < 2; ++t)
    for (int i = 0; i < 6; ++i) {
      if (t == (int)transposed && i == l) return o;
      o += plan_of(i, t != 0).floats();
    }
  return o;
}
constexpr size_t PK_FLOATS = ops_off(6, true);
static_assert(PK_HEAD_W % 4 == 0 && PK_BIAS % 4 == 0 && PK_FOLD % 4 == 0 && PK_OPS % 4 == 0, "float4 loads from the pack stay aligned");

// ---- weight packing: the BatchNorm fold ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float bn_scale(const float* __restrict__ g, const float* __restrict__ var, float eps, int c) {
  return g[c] * rsqrtf(var[c] + eps);
}
// w [co][per] -> dw [co][per] * scale[co] (transposed = 0) or dw [per][co] (transposed = 1: the vector-unit layouts [tap][c]);
// shift [co] = beta + (b - mean) * scale
__global__ void fold_k(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ g, const float* __restrict__ be,
                       const float* __restrict__ mu, const float* __restrict__ var, float eps, int co, int per, int transposed,
                       float* __restrict__ dw, float* __restrict__ shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < co * per) {
    const int c = i / per, r = i - c * per;
    dw[transposed ? r * co + c : i] = w[i] * bn_scale(g, var, eps, c);
  }
  if (i < co) shift[i] = be[i] + (b[i] - mu[i]) * bn_scale(g, var, eps, i);
}
// cov7: one output channel, w [1][128][9] -> [tap][ci] * scale
__global__ void fold_head_k(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ g, const float* __restrict__ be,
                            const float* __restrict__ mu, const float* __restrict__ var, float eps, float* __restrict__ dw,
                            float* __restrict__ shift) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const float sc = bn_scale(g, var, eps, 0);
  if (i < 9 * DEC) dw[(i % 9) * DEC + i / 9] = w[i] * sc;
  if (i == 0) shift[0] = be[0] + (b[0] - mu[0]) * sc;
}

// ---- reflection padding by one: the index a tap reads, and its transpose -----------------------------------------------------------------
__device__ __forceinline__ int reflect1(int y, int H) { return y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y); }
// The output rows q whose tap d (-1, 0, 1) reads input row y, i.e. reflect1(q + d) = y: y - d where that is a row, and the rows whose
// read left the plane and came back -- q = 0 with d = -1 reads row 1, q = H - 1 with d = +1 reads row H - 2.  At most two.
__device__ __forceinline__ int readers(int y, int d, int H, int q[2]) {
  int n = 0;
  const int s = y - d;
  if ((unsigned)s < (unsigned)H) q[n++] = s;
  if (d == -1 && y == 1) q[n++] = 0;
  if (d == 1 && y == H - 2) q[n++] = H - 1;
  return n;
}
__device__ __forceinline__ float sum16(float v) {   // over the 16 lanes of a pixel, a fixed order
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  return v;
}

// ---- cov1: reflect, 1 -> 64, shift, PReLU, into channels [0, 64) of enc.  16 lanes per pixel, one channel quad each.  PAIR (stream 1):
// 0.5 (f1 of stream 0 + own) goes to channels [64, 128) of d2 ----------------------------------------------------------------------------
template <bool PAIR>
__global__ __launch_bounds__(256) void stem_fwd_k(const float* __restrict__ x, size_t sb, const float* __restrict__ pw, float slope,
                                                  float* __restrict__ enc, const float* __restrict__ enc0, float* __restrict__ d2, int H, int W,
                                                  size_t n) {
  const size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int c = 4 * (threadIdx.x & 15);
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), xx = (int)(i - b * hw - (size_t)y * W);
  const float* __restrict__ src = x + b * sb;
  float4 s = *reinterpret_cast<const float4*>(pw + 9 * CH + c);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const float v = src[(size_t)reflect1(y + tap / 3 - 1, H) * W + reflect1(xx + tap % 3 - 1, W)];
    const float4 wv = *reinterpret_cast<const float4*>(pw + tap * CH + c);
    s.x = fmaf(wv.x, v, s.x), s.y = fmaf(wv.y, v, s.y), s.z = fmaf(wv.z, v, s.z), s.w = fmaf(wv.w, v, s.w);
  }
  const float4 f = make_float4(leaky(s.x, slope), leaky(s.y, slope), leaky(s.z, slope), leaky(s.w, slope));
  *reinterpret_cast<float4*>(enc + i * ENC + c) = f;
  if constexpr (PAIR) {
    const float4 u = *reinterpret_cast<const float4*>(enc0 + i * ENC + c);
    *reinterpret_cast<float4*>(d2 + i * DEC + CH + c) = make_float4(0.5f * (u.x + f.x), 0.5f * (u.y + f.y), 0.5f * (u.z + f.z), 0.5f * (u.w + f.w));
  }
}

// Reverse: dz[q] = PReLU'(f1[q]) * (dg[q][0:64) + 0.5 d_d2[q][64:128)); d_x[p] = sum over taps and over the output pixels q whose
// reflected read of that tap hits p of W[.][tap] . dz[q].  16 lanes per pixel, one channel quad each, then the sum over the 16.
__global__ __launch_bounds__(256) void stem_bwd_k(const float* __restrict__ pw, float slope, const float* __restrict__ enc, const float* __restrict__ dg,
                                                  const float* __restrict__ dd2, float* __restrict__ dx, int H, int W, size_t n) {
  const size_t i0 = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const size_t i = i0 < n ? i0 : n - 1;   // every lane stays for the shuffles
  const int c = 4 * (threadIdx.x & 15);
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    int qy[2], qx[2];
    const int ny = readers(y, tap / 3 - 1, H, qy), nx = readers(x, tap % 3 - 1, W, qx);
    const float4 wv = *reinterpret_cast<const float4*>(pw + tap * CH + c);
    for (int a = 0; a < ny; ++a)
      for (int e = 0; e < nx; ++e) {
        const size_t o = (size_t)b * hw + (size_t)qy[a] * W + qx[e];
        const float4 g = *reinterpret_cast<const float4*>(dg + o * DEC + c), u = *reinterpret_cast<const float4*>(dd2 + o * DEC + CH + c);
        const float4 z = dleaky4(*reinterpret_cast<const float4*>(enc + o * ENC + c),
                                 make_float4(fmaf(0.5f, u.x, g.x), fmaf(0.5f, u.y, g.y), fmaf(0.5f, u.z, g.z), fmaf(0.5f, u.w, g.w)), slope);
        s = fmaf(wv.x, z.x, s), s = fmaf(wv.y, z.y, s), s = fmaf(wv.z, z.z, s), s = fmaf(wv.w, z.w, s);
      }
  }
  s = sum16(s);
  if (i0 < n && c == 0) dx[i] = s;
}

// ---- cov7: reflect, 128 -> 1, shift, sigmoid.  16 lanes per pixel, the channel quads cq and cq + 16 each, then the sum over the 16 ---------
__global__ __launch_bounds__(256) void head_fwd_k(const float* __restrict__ pack, const float* __restrict__ d2, float* __restrict__ out, int H, int W,
                                                  size_t n) {
  const size_t i0 = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const size_t i = i0 < n ? i0 : n - 1;
  const int c = 4 * (threadIdx.x & 15);
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const float* __restrict__ src = d2 + ((size_t)b * hw + (size_t)reflect1(y + tap / 3 - 1, H) * W + reflect1(x + tap % 3 - 1, W)) * DEC;
    const float* __restrict__ wt = pack + PK_HEAD_W + tap * DEC;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float4 v = *reinterpret_cast<const float4*>(src + CH * h + c), wv = *reinterpret_cast<const float4*>(wt + CH * h + c);
      s = fmaf(wv.x, v.x, s), s = fmaf(wv.y, v.y, s), s = fmaf(wv.z, v.z, s), s = fmaf(wv.w, v.w, s);
    }
  }
  s = sum16(s);
  if (i0 < n && c == 0) out[i] = 1.f / (1.f + expf(-(s + pack[PK_HEAD_B])));
}

// Reverse: dz = d * f * (1 - f) off the taped plane; per pixel the nine sums T[tap] of dz over the output pixels whose reflected read of
// that tap hits the pixel, once; then d_d2[p][ci] = sum over taps of W[ci][tap] * T[tap].  16 lanes per pixel, two channel quads each;
// WRITES all 128 channels of d_d2.
__global__ __launch_bounds__(256) void head_bwd_k(const float* __restrict__ pack, const float* __restrict__ out, const float* __restrict__ g,
                                                  float* __restrict__ dd2, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int c = 4 * (threadIdx.x & 15);
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float4 s0 = make_float4(0.f, 0.f, 0.f, 0.f), s1 = s0;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    int qy[2], qx[2];
    const int ny = readers(y, tap / 3 - 1, H, qy), nx = readers(x, tap % 3 - 1, W, qx);
    float T = 0.f;
    for (int a = 0; a < ny; ++a)
      for (int e = 0; e < nx; ++e) {
        const size_t o = (size_t)b * hw + (size_t)qy[a] * W + qx[e];
        const float f = out[o];
        T = fmaf(g[o], f * (1.f - f), T);
      }
    const float* __restrict__ wt = pack + PK_HEAD_W + tap * DEC;
    const float4 w0 = *reinterpret_cast<const float4*>(wt + c), w1 = *reinterpret_cast<const float4*>(wt + CH + c);
    s0.x = fmaf(w0.x, T, s0.x), s0.y = fmaf(w0.y, T, s0.y), s0.z = fmaf(w0.z, T, s0.z), s0.w = fmaf(w0.w, T, s0.w);
    s1.x = fmaf(w1.x, T, s1.x), s1.y = fmaf(w1.y, T, s1.y), s1.z = fmaf(w1.z, T, s1.z), s1.w = fmaf(w1.w, T, s1.w);
  }
  *reinterpret_cast<float4*>(dd2 + i * DEC + c) = s0;
  *reinterpret_cast<float4*>(dd2 + i * DEC + CH + c) = s1;
}

}  // namespace

extern "C" size_t paif_didfuse_pack_floats(void) { return PK_FLOATS; }

extern "C" int paif_didfuse_pack_conv(const float* w, const float* b, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                                      const float* bn_var, float eps, int conv, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && bn_weight && bn_bias && bn_mean && bn_var && pack, PAIF_EINVAL, "didfuse_pack_conv: null pointer");
  PAIF_REQUIRE(conv >= 0 && conv <= 10, PAIF_EINVAL, "didfuse_pack_conv: conv %d outside [0, 10]", conv);
  PAIF_REQUIRE(eps >= 0.f, PAIF_EINVAL, "didfuse_pack_conv: negative eps");
  const hipStream_t s = paif::as_stream(stream);
  const dim3 th(256);
  if (conv == 10) {
    hipLaunchKernelGGL(fold_head_k, dim3((9 * DEC + 255) / 256), th, 0, s, w, b, bn_weight, bn_bias, bn_mean, bn_var, eps, pack + PK_HEAD_W,
                       pack + PK_HEAD_B);
  } else if (conv < 8 && conv % 4 == 0) {
    float* pw = pack + PK_STEM + 640 * (conv / 4);
    hipLaunchKernelGGL(fold_k, dim3((9 * CH + 255) / 256), th, 0, s, w, b, bn_weight, bn_bias, bn_mean, bn_var, eps, CH, 9, 1, pw, pw + 9 * CH);
  } else {
    // cov2 -> layer 2 s; cov3, cov4 -> rows [0, 64), [64, 128) of layer 2 s + 1; cov5, cov6 -> 4, 5
    const int j = conv % 4, l = conv >= 8 ? conv - 4 : 2 * (conv / 4) + (j > 1), row = j == 3 && conv < 8 ? CH : 0;
    const Layer y = layer_of(l);
    const int per = y.cin * 9;
    hipLaunchKernelGGL(fold_k, dim3((unsigned)((CH * per + 255) / 256)), th, 0, s, w, b, bn_weight, bn_bias, bn_mean, bn_var, eps, CH, per, 0,
                       pack + fold_off(l) + (size_t)row * per, pack + bias_off(l) + row);
    // the operand packs read the layer's whole folded weight: for cov3 | cov4 the later call of the two completes them
    for (int tr = 0; tr < 2; ++tr) pack_ops(pack + fold_off(l), y.cout, y.cin, 0, plan_of(l, tr != 0), tr, pack + ops_off(l, tr != 0), s);
  }
  PAIF_LAUNCH_CHECK("didfuse_pack_conv");
  return 0;
}

#define DID_WHY " (reflection padding needs H, W >= 2)"   // cov1 and cov7 reflect: every entry point refuses a plane they could not take

extern "C" int paif_didfuse_stem_fwd(const float* x, size_t sb, const float* pack, int stream_id, float slope, float* enc, const float* enc0,
                                     float* d2, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(x && pack && enc, PAIF_EINVAL, "didfuse_stem_fwd: null pointer");
  PAIF_REQUIRE(stream_id == 0 || stream_id == 1, PAIF_EINVAL, "didfuse_stem_fwd: stream %d is neither 0 (x_over) nor 1 (x_under)", stream_id);
  PAIF_REQUIRE((stream_id == 1) == (enc0 != nullptr) && (stream_id == 1) == (d2 != nullptr), PAIF_EINVAL,
               "didfuse_stem_fwd: stream 1, and only stream 1, takes stream 0's enc and the slab d2 for the mean");
  PAIF_REQUIRE(enc0 != enc, PAIF_EINVAL, "didfuse_stem_fwd: the two streams' maps must differ");
  PAIF_SLAB_SHAPE("didfuse_stem_fwd", 2, DID_WHY, 31);
  PAIF_REQUIRE((size_t)H * W <= sb, PAIF_EINVAL, "didfuse_stem_fwd: batch stride smaller than a plane");
  const dim3 grid((unsigned)((n + 15) / 16)), th(256);
  const float* pw = pack + PK_STEM + 640 * stream_id;
  if (stream_id) hipLaunchKernelGGL(stem_fwd_k<true>, grid, th, 0, paif::as_stream(stream), x, sb, pw, slope, enc, enc0, d2, H, W, n);
  else hipLaunchKernelGGL(stem_fwd_k<false>, grid, th, 0, paif::as_stream(stream), x, sb, pw, slope, enc, enc0, d2, H, W, n);
  PAIF_LAUNCH_CHECK("didfuse_stem_fwd");
  return 0;
}

extern "C" int paif_didfuse_conv_fwd(const float* pack, int layer, float slope, const float* in, float* out, const float* pair, float* avg, int B,
                                     int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && out, PAIF_EINVAL, "didfuse_conv_fwd: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 5, PAIF_EINVAL, "didfuse_conv_fwd: layer %d outside [0, 5]", layer);
  PAIF_REQUIRE((layer < 4) == (in == out), PAIF_EINVAL, "didfuse_conv_fwd: an encoder conv works inside enc, a decoder conv from one slab to another");
  const bool paired = layer == 2 || layer == 3;
  PAIF_REQUIRE(paired == (pair != nullptr) && paired == (avg != nullptr), PAIF_EINVAL,
               "didfuse_conv_fwd: the layers of stream 1, and only they, take stream 0's enc and the slab of the mean");
  PAIF_REQUIRE(!paired || (pair != out && avg != out && (const float*)avg != pair), PAIF_EINVAL,
               "didfuse_conv_fwd: three different maps are expected");
  PAIF_SLAB_SHAPE("didfuse_conv_fwd", 2, DID_WHY, 31);
  PAIF_SLAB_TILES("didfuse_conv_fwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, false);
  const bool wide = layer < 4 && (layer & 1);   // cov3 | cov4
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.wpk = pack + ops_off(layer, false), a.bias = pack + bias_off(layer), a.slope = slope, a.out = out;
  if (layer < 4) {
    a.in = in + (wide ? CH : 0), a.in_cs = ENC, a.out_cs = ENC, a.out_off = wide ? 2 * CH : CH;
  } else {
    a.in = in, a.in_cs = DEC, a.out_cs = DEC, a.out_off = 0;
  }
  a.nq = y.cin / 4, a.out_n = y.cout;
  a.pair = pair, a.avg = avg, a.avg_cs = DEC, a.avg_off = wide ? 0 : CH;   // F_b | F_d fill bd, F_2 is [64, 128) of d1
  const dim3 grid = conv_grid(pl, B, tx, ty);
  const hipStream_t s = paif::as_stream(stream);
  if (wide && paired) launch_conv4<false, EPI_ACT, ACT_TANH, true, XIN_PLAIN>(grid, s, a);
  else if (wide) launch_conv4<false, EPI_ACT, ACT_TANH, false, XIN_PLAIN>(grid, s, a);
  else if (paired) launch_conv4<false, EPI_ACT, ACT_LEAKY, true, XIN_PLAIN>(grid, s, a);
  else launch_conv4<false, EPI_ACT, ACT_LEAKY, false, XIN_PLAIN>(grid, s, a);
  PAIF_LAUNCH_CHECK("didfuse_conv_fwd");
  return 0;
}

extern "C" int paif_didfuse_head_fwd(const float* pack, const float* d2, float* fused, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && d2 && fused, PAIF_EINVAL, "didfuse_head_fwd: null pointer");
  PAIF_SLAB_SHAPE("didfuse_head_fwd", 2, DID_WHY, 31);
  hipLaunchKernelGGL(head_fwd_k, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, paif::as_stream(stream), pack, d2, fused, H, W, n);
  PAIF_LAUNCH_CHECK("didfuse_head_fwd");
  return 0;
}

extern "C" int paif_didfuse_head_bwd(const float* pack, const float* fused, const float* d_fused, float* d_d2, int B, int H, int W,
                                     paif_stream_t stream) {
  PAIF_REQUIRE(pack && fused && d_fused && d_d2, PAIF_EINVAL, "didfuse_head_bwd: null pointer");
  PAIF_SLAB_SHAPE("didfuse_head_bwd", 2, DID_WHY, 31);
  hipLaunchKernelGGL(head_bwd_k, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, paif::as_stream(stream), pack, fused, d_fused, d_d2, H, W, n);
  PAIF_LAUNCH_CHECK("didfuse_head_bwd");
  return 0;
}

extern "C" int paif_didfuse_conv_bwd(const float* pack, int layer, float slope, const float* taped, const float* d_out, float* d_in,
                                     const float* d_skip, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && taped && d_out && d_in, PAIF_EINVAL, "didfuse_conv_bwd: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 5, PAIF_EINVAL, "didfuse_conv_bwd: layer %d outside [0, 5]", layer);
  const bool cov2 = layer < 4 && !(layer & 1), cov34 = layer < 4 && (layer & 1);
  PAIF_REQUIRE(taped != d_out && taped != d_in && taped != d_skip, PAIF_EINVAL, "didfuse_conv_bwd: the gradient maps must not alias the taped maps");
  PAIF_REQUIRE(cov2 == (d_out == d_in), PAIF_EINVAL, "didfuse_conv_bwd: cov2's transpose works inside dg, every other one from one map to another");
  PAIF_REQUIRE(cov2 == (d_skip != nullptr), PAIF_EINVAL, "didfuse_conv_bwd: cov2's transpose, and only it, takes d_d1 for the mean's transpose");
  PAIF_REQUIRE(d_skip != d_in, PAIF_EINVAL, "didfuse_conv_bwd: d_d1 must not be the map that is written");
  PAIF_SLAB_SHAPE("didfuse_conv_bwd", 2, DID_WHY, 31);
  PAIF_SLAB_TILES("didfuse_conv_bwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, true);
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.wpk = pack + ops_off(layer, true), a.slope = slope, a.out = d_in;
  a.nq = y.cout / 4, a.in_cs = DEC, a.out_cs = DEC, a.out_n = y.cin;
  const dim3 grid = conv_grid(pl, B, tx, ty);
  const hipStream_t s = paif::as_stream(stream);
  if (cov34) {          // d_bd (all 128), tanh' from fB | fD, the mean's 0.5 -> dg[64:128)
    a.in = d_out, a.mask = taped + 2 * CH, a.mask_cs = ENC, a.in_scale = 0.5f, a.out_off = CH;
    launch_conv4<true, EPI_STORE, ACT_TANH, false, XIN_SCALED>(grid, s, a);
  } else if (cov2) {    // dg[64:128) + 0.5 d_d1[64:128), PReLU' from f2 -> dg[0:64)
    a.in = d_out + CH, a.in2 = d_skip + CH, a.mask = taped + CH, a.mask_cs = ENC, a.in_scale = 1.f, a.in2_scale = 0.5f, a.out_off = 0;
    launch_conv4<true, EPI_STORE, ACT_LEAKY, false, XIN_SUM>(grid, s, a);
  } else {              // cov6': d_d2[0:64), mask Out2 -> d_d1; cov5': d_d1[0:64), mask Out1 -> d_bd
    a.in = d_out, a.mask = taped, a.out_off = 0;
    launch_conv4<true, EPI_STORE, ACT_LEAKY, false, XIN_PLAIN>(grid, s, a);
  }
  PAIF_LAUNCH_CHECK("didfuse_conv_bwd");
  return 0;
}

extern "C" int paif_didfuse_stem_bwd(const float* pack, int stream_id, float slope, const float* enc, const float* dg, const float* d_d2, float* d_x,
                                     int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && enc && dg && d_d2 && d_x, PAIF_EINVAL, "didfuse_stem_bwd: null pointer");
  PAIF_REQUIRE(stream_id == 0 || stream_id == 1, PAIF_EINVAL, "didfuse_stem_bwd: stream %d is neither 0 (x_over) nor 1 (x_under)", stream_id);
  PAIF_SLAB_SHAPE("didfuse_stem_bwd", 2, DID_WHY, 31);
  hipLaunchKernelGGL(stem_bwd_k, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, paif::as_stream(stream), pack + PK_STEM + 640 * stream_id, slope, enc,
                     dg, d_d2, d_x, H, W, n);
  PAIF_LAUNCH_CHECK("didfuse_stem_bwd");
  return 0;
}
