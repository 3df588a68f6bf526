// U2Fusion baseline (reference fusion_model/U2Fusion.py:91-125): conv_1 2 -> 44, five dense layers 44 (i + 1) -> 44 whose outputs are
// appended to the concat, sub 264 -> 128 -> 64 -> 32 -> 1, every conv 3 x 3 with zero pad 1, LeakyReLU(0.2) after all but the last, tanh
// after the last.  Forward and the reverse pass (input gradients).  One launch per layer, nothing fused across layers.
//
// LAYOUT.  fp32 NHWC.  ONE slab cat[B][H][W][264] holds conv_1's map and the five dense maps in the reference's cat order: dense layer i
// reads channels [0, 44 (i + 1)) and writes [44 (i + 1), 44 (i + 2)); the concat is never built a second time.  s1[..][128], s2[..][64],
// s3[..][32] are the maps of sub.0 .. sub.2.  The gradient buffers use the same layouts.  44 = 11 channel quads: every slice starts at a
// multiple of 176 B and float4 accesses stay aligned.
//
// THE MATRIX-CORE CONV (conv_k).  A 3 x 3, pad 1 implicit GEMM on v_mfma_f32_16x16x4_f32 (exact f32, a k-ordered fmaf chain) in the
// operand arrangement of sdnet.hip: output CHANNELS on M, 16 PIXELS of one image row on N; the D operand of lane l is channels
// 4 (l >> 4) .. + 3 of pixel l & 15, one float4 of the NHWC map, and the B operand of four consecutive instructions is one float4 of the
// input map (instruction j takes channel 4 k + j for its k).  A workgroup of four waves owns a 16 x 16 pixel tile (four rows per wave) and
// MB blocks of 16 output channels (blockIdx.y selects the group of MB blocks): 4 MB accumulators of four VGPRs per lane.  The weights do
// not fit in registers and the input tile does not fit in LDS, so the kernel loops over CHUNKS of 16 input channels: per chunk it stages
// the tile + halo 1 (quad-plane image of sdnet.hip, 21 KB) and the chunk's weights in operand order (9 taps x MB x 1 KB), then per tap
// reads four pixel float4 and MB weight float4 for 16 MB instructions.  Channel counts that are no multiple of 16 are padded with zeros
// in the staged tile and in the weight pack (K side), with zero weight rows and masked stores (M side); the maps themselves stay exact.
// Parameters: the input slab (pointer at its first channel, channel stride, quads), the output slab (pointer, channel stride, channel
// offset, channel count), an input mask (the reverse pass stages dz = d * (taped > 0 ? 1 : 0.2)), and the epilogue: bias + LeakyReLU
// store, plain store, or read-add-write.  The transposed convs of the reverse pass are the same kernel on a second weight pack (taps
// flipped, ci / co swapped).
//
// conv_1, sub.3 and their transposes run on the vector unit, weights through the scalar cache.
//
// BORDER RULE.  Every conv zero-pads its own input: whatever is read outside the image is zero at every level (total halo 10).
// LEAKYRELU.  torch: x > 0 ? x : 0.2 * x; in reverse the branch comes from the taped OUTPUT (same sign), a pre-activation of exactly 0
// takes the 0.2 branch.  The bias is added LAST, after the conv sum.
// No atomics: every output element is owned by one lane, the summation order is fixed, and no launch reads channels it writes.
#include <math.h>

#include "paif_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

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

// One operand pack of conv_k: M output channels in `groups` groups of MB blocks of 16, K input channels in `chunks` chunks of 16.
struct Plan {
  int M, K, MB, groups, chunks;
  __host__ __device__ constexpr size_t floats() const { return (size_t)groups * chunks * 9 * MB * 256; }
};
// MB: the fewest padded blocks among 4 and 3 (a tie takes 4); 2 for 32 channels.
__host__ __device__ constexpr Plan plan_of(int l, bool transposed) {
  const Layer y = layer_of(l);
  const int M = transposed ? y.cin : y.cout, K = transposed ? y.cout : y.cin, blocks = (M + 15) / 16;
  const int MB = blocks <= 2 ? 2 : ((blocks + 3) / 4) * 4 <= ((blocks + 2) / 3) * 3 ? 4 : 3;
  return Plan{M, K, MB, (blocks + MB - 1) / MB, (K + 15) / 16};
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

// ---- weight packing -----------------------------------------------------------------------------------------------------------------
// Operand order of conv_k: [group][chunk][tap][block mb][lane][j]; A[m = lane & 15][k = lane >> 4] of instruction j is the weight of
// output channel 16 (group * MB + mb) + (lane & 15) and input channel 16 chunk + 4 (lane >> 4) + j.  Forward: W[m][k][tap]; transposed:
// W[k][m][8 - tap].  Zero beyond M and K.
__global__ void pack_ops_k(const float* __restrict__ w, int cin, Plan pl, int transposed, float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pl.floats()) return;
  const int j = i & 3, lane = (i >> 2) & 63;
  size_t r = i >> 8;
  const int mb = r % pl.MB;
  r /= pl.MB;
  const int tap = r % 9;
  r /= 9;
  const int c = r % pl.chunks, g = r / pl.chunks;
  const int m = 16 * (g * pl.MB + mb) + (lane & 15), k = 16 * c + 4 * (lane >> 4) + j;
  float v = 0.f;
  if (m < pl.M && k < pl.K) v = transposed ? w[((size_t)k * cin + m) * 9 + 8 - tap] : w[((size_t)m * cin + k) * 9 + tap];
  dst[i] = v;
}

// conv_1 (layer 0), the biases of layers 1..8, sub.3 (layer 9)
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

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }
__device__ __forceinline__ float dleaky(float out, float g) { return out > 0.f ? g : SLOPE * g; }
__device__ __forceinline__ float4 dleaky4(float4 f, float4 v) { return make_float4(dleaky(f.x, v.x), dleaky(f.y, v.y), dleaky(f.z, v.z), dleaky(f.w, v.w)); }

// ---- the matrix-core conv -----------------------------------------------------------------------------------------------------------------
constexpr int DT = 16;                 // tile edge: 4 waves x 4 rows of 16 pixels
constexpr int DP = DT + 2;             // + halo 1
constexpr int QS = 336;                // quad stride in float4: DP * DP = 324 rounded up to a multiple of 16 (256 B)
static_assert(QS >= DP * DP && QS % 16 == 0, "quad planes start at the same LDS bank");

enum { EPI_ACT = 0, EPI_STORE = 1, EPI_ADD = 2 };

struct ConvArgs {
  const float* in;     // first channel of the input slice; pixel stride in_cs floats, nq channel quads
  const float* mask;   // MASK: the taped map of the same slice (same stride)
  float* out;          // first channel of the output map; pixel stride out_cs; channels [out_off, out_off + out_n) are written
  const float* wpk;    // operand pack of this conv
  const float* bias;   // EPI_ACT
  int in_cs, nq, out_cs, out_off, out_n, chunks, H, W, tx, ty;
};

template <int MB, bool MASK, int EPI>
__global__ __launch_bounds__(256, 2) void conv_k(const ConvArgs a) {
  __shared__ float4 s_x[4 * QS];
  __shared__ float4 s_w[9 * MB * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, p = lane & 15;
  const int H = a.H, W = a.W;
  const int b = blockIdx.x / (a.tx * a.ty), rem = blockIdx.x - b * a.tx * a.ty, by = rem / a.tx, bx = rem - by * a.tx;
  const int y0 = by * DT, x0 = bx * DT, r0 = 4 * wave;
  const size_t img = (size_t)b * H * W;
  const float4* __restrict__ wg = reinterpret_cast<const float4*>(a.wpk) + (size_t)blockIdx.y * a.chunks * (9 * MB * 64);

  f32x4 acc[MB][4];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[mb][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < a.chunks; ++c) {
    if (c) __syncthreads();   // the previous chunk has been read
    for (int e = tid; e < DP * DP * 4; e += 256) {
      const int sq = e & 3, pix = e >> 2, ly = pix / DP, lx = pix - ly * DP, gy = y0 - 1 + ly, gx = x0 - 1 + lx, gq = 4 * c + sq;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W && gq < a.nq) {
        const size_t o = (img + (size_t)gy * W + gx) * a.in_cs + 4 * gq;
        v = *reinterpret_cast<const float4*>(a.in + o);
        if constexpr (MASK) v = dleaky4(*reinterpret_cast<const float4*>(a.mask + o), v);
      }
      s_x[sq * QS + pix] = v;
    }
    const float4* __restrict__ wc = wg + (size_t)c * (9 * MB * 64);
    for (int e = tid; e < 9 * MB * 64; e += 256) s_w[e] = wc[e];
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      float4 xv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = s_x[q * QS + (r0 + r + tap / 3) * DP + p + tap % 3];
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        const float4 wv = s_w[(tap * MB + mb) * 64 + lane];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mb][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv[r].x, acc[mb][r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mb][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv[r].y, acc[mb][r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mb][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv[r].z, acc[mb][r], 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[mb][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv[r].w, acc[mb][r], 0, 0, 0);
      }
    }
  }

  const int gx = x0 + p;
  if (gx >= W) return;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int co = 16 * ((int)blockIdx.y * MB + mb) + 4 * q;   // out_n is a multiple of 4: a quad is written whole or not at all
    if (co >= a.out_n) continue;
    float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EPI == EPI_ACT) bs = *reinterpret_cast<const float4*>(a.bias + co);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gy = y0 + r0 + r;
      if (gy >= H) continue;
      float4* o = reinterpret_cast<float4*>(a.out + (img + (size_t)gy * W + gx) * a.out_cs + a.out_off + co);   // owned by this lane
      const f32x4 v = acc[mb][r];
      if constexpr (EPI == EPI_ACT) {
        *o = make_float4(leaky(v[0] + bs.x), leaky(v[1] + bs.y), leaky(v[2] + bs.z), leaky(v[3] + bs.w));
      } else if constexpr (EPI == EPI_STORE) {
        *o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        const float4 u = *o;
        *o = make_float4(u.x + v[0], u.y + v[1], u.z + v[2], u.w + v[3]);
      }
    }
  }
}

template <bool MASK, int EPI>
void launch_conv(int MB, dim3 grid, hipStream_t s, const ConvArgs& a) {
  if (MB == 4) hipLaunchKernelGGL((conv_k<4, MASK, EPI>), grid, dim3(256), 0, s, a);
  else if (MB == 3) hipLaunchKernelGGL((conv_k<3, MASK, EPI>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_k<2, MASK, EPI>), grid, dim3(256), 0, s, a);
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
    *reinterpret_cast<float4*>(o + c) = make_float4(leaky(acc[c] + bs[c]), leaky(acc[c + 1] + bs[c + 1]), leaky(acc[c + 2] + bs[c + 2]),
                                                    leaky(acc[c + 3] + bs[c + 3]));
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
      const float4 z = dleaky4(*reinterpret_cast<const float4*>(cat + o + c), *reinterpret_cast<const float4*>(dcat + o + c));
      s1 = fmaf(w1[c], z.x, s1), s1 = fmaf(w1[c + 1], z.y, s1), s1 = fmaf(w1[c + 2], z.z, s1), s1 = fmaf(w1[c + 3], z.w, s1);
      s2 = fmaf(w2[c], z.x, s2), s2 = fmaf(w2[c + 1], z.y, s2), s2 = fmaf(w2[c + 2], z.z, s2), s2 = fmaf(w2[c + 3], z.w, s2);
    }
  }
  d1[i] = s1;
  d2[i] = s2;
}

// ---- sub.3: 32 -> 1, bias, tanh.  One pixel per thread -------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_k(const float* __restrict__ pack, const float* __restrict__ s3, float* __restrict__ out, int H, int W,
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
    const float* __restrict__ src = s3 + ((size_t)b * hw + (size_t)gy * W + gx) * 32;
    const float* __restrict__ wt = pack + PK_HEAD_W + tap * 32;
#pragma unroll
    for (int c = 0; c < 32; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(src + c);
      s = fmaf(wt[c], v.x, s), s = fmaf(wt[c + 1], v.y, s), s = fmaf(wt[c + 2], v.z, s), s = fmaf(wt[c + 3], v.w, s);
    }
  }
  out[i] = tanhf(s + pack[PK_HEAD_B]);
}

// Reverse of sub.3: dy = g * (1 - out^2); d_s3[p][ci] = sum over tap of W[0][ci][tap] * dy[p - (tap - centre)].  Eight lanes per pixel, one
// channel quad each; WRITES d_s3.
__global__ __launch_bounds__(256) void head_bwd_k(const float* __restrict__ pack, const float* __restrict__ out, const float* __restrict__ g,
                                                  float* __restrict__ ds3, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 32 + (threadIdx.x >> 3);
  const int cq = threadIdx.x & 7;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y - (tap / 3 - 1), gx = x - (tap % 3 - 1);
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const size_t o = (size_t)b * hw + (size_t)gy * W + gx;
    const float f = out[o], dy = g[o] * ((1.f - f) * (1.f + f));
    const float4 wv = *reinterpret_cast<const float4*>(pack + PK_HEAD_W + tap * 32 + 4 * cq);
    s.x = fmaf(wv.x, dy, s.x), s.y = fmaf(wv.y, dy, s.y), s.z = fmaf(wv.z, dy, s.z), s.w = fmaf(wv.w, dy, s.w);
  }
  *reinterpret_cast<float4*>(ds3 + i * 32 + 4 * cq) = s;
}

}  // namespace

extern "C" size_t paif_u2fusion_pack_floats(void) { return PK_FLOATS; }

extern "C" int paif_u2fusion_pack_conv(const float* w, const float* b, int layer, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && pack, PAIF_EINVAL, "u2fusion_pack_conv: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 9, PAIF_EINVAL, "u2fusion_pack_conv: layer %d outside [0, 9]", layer);
  const hipStream_t s = paif::as_stream(stream);
  hipLaunchKernelGGL(pack_small_k, dim3(4), dim3(256), 0, s, w, b, layer, pack);
  if (layer >= 1 && layer <= 8)
    for (int t = 0; t < 2; ++t) {
      const Plan pl = plan_of(layer, t != 0);
      hipLaunchKernelGGL(pack_ops_k, dim3((unsigned)((pl.floats() + 255) / 256)), dim3(256), 0, s, w, layer_of(layer).cin, pl, t, pack + ops_off(layer, t != 0));
    }
  PAIF_LAUNCH_CHECK("u2fusion_pack_conv");
  return 0;
}

#define U2F_SHAPE(name)                                                                                   \
  PAIF_REQUIRE(B >= 1 && H >= 1 && W >= 1, PAIF_EINVAL, name ": bad shape %d x %d x %d", B, H, W);          \
  PAIF_REQUIRE((size_t)B* H* W < ((size_t)1 << 31), PAIF_EINVAL, name ": more than 2^31 pixels");           \
  const size_t n = (size_t)B * H * W;                                                                       \
  (void)n
#define U2F_TILES(name)                                                                                   \
  const int tx = (W + DT - 1) / DT, ty = (H + DT - 1) / DT;                                                 \
  PAIF_REQUIRE((size_t)tx* ty* B < ((size_t)1 << 31), PAIF_EINVAL, name ": too many tiles")

extern "C" int paif_u2fusion_stem_fwd(const float* x_over, size_t sb1, const float* x_under, size_t sb2, const float* pack, float* cat, int B, int H,
                                      int W, paif_stream_t stream) {
  PAIF_REQUIRE(x_over && x_under && pack && cat, PAIF_EINVAL, "u2fusion_stem_fwd: null pointer");
  U2F_SHAPE("u2fusion_stem_fwd");
  PAIF_REQUIRE((size_t)H * W <= sb1 && (size_t)H * W <= sb2, PAIF_EINVAL, "u2fusion_stem_fwd: batch stride smaller than a plane");
  hipLaunchKernelGGL(stem_fwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), x_over, sb1, x_under, sb2, pack, cat, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_stem_fwd");
  return 0;
}

extern "C" int paif_u2fusion_conv_fwd(const float* pack, int layer, const float* in, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && out, PAIF_EINVAL, "u2fusion_conv_fwd: null pointer");
  PAIF_REQUIRE(layer >= 1 && layer <= 8, PAIF_EINVAL, "u2fusion_conv_fwd: layer %d outside [1, 8]", layer);
  PAIF_REQUIRE((layer <= 5) == (in == out), PAIF_EINVAL, "u2fusion_conv_fwd: a dense layer works inside cat, a sub layer from one map to another");
  U2F_SHAPE("u2fusion_conv_fwd");
  U2F_TILES("u2fusion_conv_fwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, false);
  ConvArgs a;
  a.in = in, a.mask = nullptr, a.out = out, a.wpk = pack + ops_off(layer, false), a.bias = pack + bias_off(layer);
  a.in_cs = layer <= 6 ? CAT : y.cin, a.nq = y.cin / 4;
  a.out_cs = layer <= 5 ? CAT : y.cout, a.out_off = layer <= 5 ? G * layer : 0, a.out_n = y.cout;
  a.chunks = pl.chunks, a.H = H, a.W = W, a.tx = tx, a.ty = ty;
  launch_conv<false, EPI_ACT>(pl.MB, dim3((unsigned)(tx * ty * B), (unsigned)pl.groups), paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("u2fusion_conv_fwd");
  return 0;
}

extern "C" int paif_u2fusion_head_fwd(const float* pack, const float* s3, float* fused, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && s3 && fused, PAIF_EINVAL, "u2fusion_head_fwd: null pointer");
  U2F_SHAPE("u2fusion_head_fwd");
  hipLaunchKernelGGL(head_fwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack, s3, fused, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_head_fwd");
  return 0;
}

extern "C" int paif_u2fusion_head_bwd(const float* pack, const float* fused, const float* d_fused, float* d_s3, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(pack && fused && d_fused && d_s3, PAIF_EINVAL, "u2fusion_head_bwd: null pointer");
  U2F_SHAPE("u2fusion_head_bwd");
  hipLaunchKernelGGL(head_bwd_k, dim3((unsigned)((n + 31) / 32)), dim3(256), 0, paif::as_stream(stream), pack, fused, d_fused, d_s3, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_head_bwd");
  return 0;
}

extern "C" int paif_u2fusion_conv_bwd(const float* pack, int layer, const float* taped, const float* d_out, float* d_in, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(pack && taped && d_out && d_in, PAIF_EINVAL, "u2fusion_conv_bwd: null pointer");
  PAIF_REQUIRE(layer >= 1 && layer <= 8, PAIF_EINVAL, "u2fusion_conv_bwd: layer %d outside [1, 8]", layer);
  PAIF_REQUIRE(taped != d_out && taped != d_in, PAIF_EINVAL, "u2fusion_conv_bwd: the gradient maps must not alias the taped maps");
  PAIF_REQUIRE((layer <= 5) == (d_out == d_in), PAIF_EINVAL, "u2fusion_conv_bwd: a dense layer works inside d_cat, a sub layer from one map to another");
  U2F_SHAPE("u2fusion_conv_bwd");
  U2F_TILES("u2fusion_conv_bwd");
  const Layer y = layer_of(layer);
  const Plan pl = plan_of(layer, true);
  const int off = layer <= 5 ? G * layer : 0, cs = layer <= 5 ? CAT : y.cout;   // where the layer's output lives
  ConvArgs a;
  a.in = d_out + off, a.mask = taped + off, a.out = d_in, a.wpk = pack + ops_off(layer, true), a.bias = nullptr;
  a.in_cs = cs, a.nq = y.cout / 4;
  a.out_cs = layer <= 6 ? CAT : y.cin, a.out_off = 0, a.out_n = y.cin;
  a.chunks = pl.chunks, a.H = H, a.W = W, a.tx = tx, a.ty = ty;
  const dim3 grid((unsigned)(tx * ty * B), (unsigned)pl.groups);
  if (layer <= 5) launch_conv<true, EPI_ADD>(pl.MB, grid, paif::as_stream(stream), a);   // reads slice `layer` of d_cat, adds below it
  else launch_conv<true, EPI_STORE>(pl.MB, grid, paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("u2fusion_conv_bwd");
  return 0;
}

extern "C" int paif_u2fusion_stem_bwd(const float* pack, const float* cat, const float* d_cat, float* d_x_over, float* d_x_under, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(pack && cat && d_cat && d_x_over && d_x_under, PAIF_EINVAL, "u2fusion_stem_bwd: null pointer");
  U2F_SHAPE("u2fusion_stem_bwd");
  hipLaunchKernelGGL(stem_bwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack, cat, d_cat, d_x_over, d_x_under, H, W, n);
  PAIF_LAUNCH_CHECK("u2fusion_stem_bwd");
  return 0;
}
