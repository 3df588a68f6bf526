// SDNet baseline (reference fusion_model/SDNet.py): two four-layer dense encoders of 16-channel maps and a 128 -> 1 fuse, forward and
// the reverse pass (input gradients).  One launch per layer, both encoders ("streams") in every launch: blockIdx.y is the stream.
//
// LAYOUT.  Feature maps are NHWC with 16 fp32 channels (64 B per pixel) in ONE allocation [stream 0/1][level 0..3][B][H][W][16]; the
// gradient maps use the same layout.  Level l of stream s is conv(l+1)(s+1) of the reference: x11 .. x14, x21 .. x24.
//
// ARITHMETIC.  fp32 throughout.  Every dense conv has 16 output channels and 16 * L input channels: on v_mfma_f32_16x16x4_f32 (exact
// f32, a k-ordered fmaf chain) one instruction is a [16 x 4] x [4 x 16] product.  The kernels put the 16 CHANNELS of the result on the
// M side and 16 PIXELS of one image row on the N side: the D operand of lane l is then channels 4 * (l >> 4) .. + 3 of pixel l & 15, one
// float4 of the NHWC map, and the B operand (pixel l & 15, k = l >> 4) of four consecutive instructions is one float4 of the input map
// when instruction j takes channel 4 * k + j for its k.  The weights are packed in that operand order (pack_k) and stay in registers:
// 36 * L VGPRs per lane, loaded once per workgroup.
//
// LDS IMAGE of a 16-channel tile: [channel quad q 0..3][row][pixel] float4, quad stride QS (a multiple of 256 B).  A wave's ds_read_b128
// of 16 consecutive pixels x 4 quads is then conflict-free for any pixel shift (each 16-lane group reads 256 contiguous bytes, and the
// quads start at the same bank).
//
// BORDER RULE.  Every conv zero-pads its own input: the staged tiles are zero outside the image at every level (total halo 2 + 1 + 1 + 1).
//
// LEAKYRELU.  torch: x > 0 ? x : 0.01 * x, gradient x > 0 ? g : 0.01 * g (a pre-activation of exactly 0 takes the negative branch).  The
// output has the sign of the pre-activation, so the reverse pass takes the branch from the taped OUTPUT (out > 0); nothing is recomputed.
//
// The bias is added LAST, after the conv sum (see reconet.hip: a sum started from the bias rounds every addition at its magnitude).
//
// REVERSE PASS.  fuse_bwd WRITES all eight gradient maps; dense_bwd<L> (L = 3, 2, 1) reads level L and adds to the levels below it -- a
// gather, every pixel owned by one lane, plain read-add-write: no atomics, fixed summation order, and no launch reads a map it writes.
#include <math.h>

#include "paif_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr float SLOPE = 0.01f;

// packed weights (pack_k), offsets in floats
constexpr int PK_STEM_W = 0;       // [stream][tap 25][co 16]
constexpr int PK_STEM_B = 800;     // [stream][co 16]
constexpr int PK_FUSE_W = 832;     // [stream][level][c 16] = the reference's cat order
constexpr int PK_FUSE_B = 960;
constexpr int PK_DENSE_B = 1024;   // [L - 1][stream][co 16]
constexpr int PK_FWD = 1152;       // per L: [stream][source level s < L][tap 9][lane 64][j 4], forward operand order
constexpr int PK_OPS = 2 * 2304 * 6;   // floats of one operand set (L = 1, 2, 3)
constexpr int PK_BWD = PK_FWD + PK_OPS;
constexpr int PK_FLOATS = PK_BWD + PK_OPS;
__host__ __device__ constexpr int dense_off(int L) { return 2 * 2304 * ((L - 1) * L / 2); }

// ---- weight packing -----------------------------------------------------------------------------------------------------------------
// layer 0: stem (w [16,1,5,5]), 1..3: dense L (w [16,16L,3,3]), 4: fuse (w [1,128,1,1], stream ignored)
__global__ void pack_k(const float* __restrict__ w, const float* __restrict__ b, int layer, int st, float* __restrict__ pack) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (layer == 0) {
    if (i < 400) pack[PK_STEM_W + st * 400 + i] = w[(i & 15) * 25 + (i >> 4)];   // i = tap * 16 + co
    if (i < 16) pack[PK_STEM_B + st * 16 + i] = b[i];
  } else if (layer == 4) {
    if (i < 128) pack[PK_FUSE_W + i] = w[i];
    if (i == 0) pack[PK_FUSE_B] = b[0];
  } else {
    const int L = layer, n = L * 2304;
    if (i < 16) pack[PK_DENSE_B + ((L - 1) * 2 + st) * 16 + i] = b[i];
    if (i >= n) return;
    const int j = i & 3, lane = (i >> 2) & 63, tap = (i >> 8) % 9, s = (i >> 8) / 9, q = lane >> 4, r = lane & 15, cin = 16 * L;
    // forward: A[co = r][k = q] of instruction j is W[r][16 s + 4 q + j][tap]; reverse: A[ci = r][k = q] is W[4 q + j][16 s + r][tap]
    pack[PK_FWD + dense_off(L) + st * n + i] = w[((size_t)r * cin + 16 * s + 4 * q + j) * 9 + tap];
    pack[PK_BWD + dense_off(L) + st * n + i] = w[((size_t)(4 * q + j) * cin + 16 * s + r) * 9 + tap];
  }
}

__device__ __forceinline__ float leaky(float v) { return v > 0.f ? v : SLOPE * v; }
__device__ __forceinline__ float dleaky(float out, float g) { return out > 0.f ? g : SLOPE * g; }

// ---- stem: 5 x 5, 1 -> 16, pad 2, bias, LeakyReLU (SDNet.py:9-10, :34, :39) -------------------------------------------------------------
constexpr int SW = 32, SH = 8;            // tile: one pixel per thread
constexpr int SPW = SW + 4, SPH = SH + 4;   // + halo 2

__global__ __launch_bounds__(256) void stem_fwd_k(const float* __restrict__ x1, size_t sb1, const float* __restrict__ x2, size_t sb2,
                                                  const float* __restrict__ pack, float* __restrict__ feat, size_t lvl, int H, int W, int tx,
                                                  int ty) {
  __shared__ float s_p[SPH * SPW];
  const int tid = threadIdx.x, st = blockIdx.y;
  const int b = blockIdx.x / (tx * ty), rem = blockIdx.x - b * tx * ty, by = rem / tx, bx = rem - by * tx;
  const int y0 = by * SH, x0 = bx * SW;
  const float* p = st ? x2 + b * sb2 : x1 + b * sb1;
  for (int e = tid; e < SPH * SPW; e += 256) {
    const int ly = e / SPW, lx = e - ly * SPW, gy = y0 - 2 + ly, gx = x0 - 2 + lx;
    const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    s_p[e] = in ? p[(size_t)gy * W + gx] : 0.f;
  }
  __syncthreads();
  const int ly = tid >> 5, lx = tid & 31, gy = y0 + ly, gx = x0 + lx;
  const float* __restrict__ wt = pack + PK_STEM_W + st * 400;
  float acc[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) acc[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 25; ++k) {
    const float v = s_p[(ly + k / 5) * SPW + lx + k % 5];
#pragma unroll
    for (int c = 0; c < 16; ++c) acc[c] = fmaf(wt[k * 16 + c], v, acc[c]);
  }
  if (gy >= H || gx >= W) return;
  const float* __restrict__ bs = pack + PK_STEM_B + st * 16;
  float* o = feat + (size_t)st * 4 * lvl + (((size_t)b * H + gy) * W + gx) * 16;
#pragma unroll
  for (int c = 0; c < 16; c += 4)
    *reinterpret_cast<float4*>(o + c) = make_float4(leaky(acc[c] + bs[c]), leaky(acc[c + 1] + bs[c + 1]), leaky(acc[c + 2] + bs[c + 2]),
                                                    leaky(acc[c + 3] + bs[c + 3]));
}

// ---- dense convs on the matrix core --------------------------------------------------------------------------------------------------
constexpr int DT = 16;                 // tile edge: 4 waves x 4 rows of 16 pixels
constexpr int DP = DT + 2;             // + halo 1
constexpr int QS = 336;                // quad stride in float4: DP * DP = 324 rounded up to a multiple of 16 (256 B)
static_assert(QS >= DP * DP && QS % 16 == 0, "quad planes start at the same LDS bank");

// Stage the tile + halo 1 of one 16-channel NHWC map into the quad-plane image; zero outside the image.  mask (optional): the map whose
// sign selects the LeakyReLU branch (the reverse pass stages dz = d_out * (out > 0 ? 1 : 0.01)).
template <bool MASK>
__device__ __forceinline__ void stage_tile(float4* __restrict__ img, const float* __restrict__ map, const float* __restrict__ out, int y0, int x0, int H,
                                           int W, int tid) {
  for (int e = tid; e < DP * DP * 4; e += 256) {
    const int q = e & 3, pix = e >> 2, ly = pix / DP, lx = pix - ly * DP, gy = y0 - 1 + ly, gx = x0 - 1 + lx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
      const size_t o = ((size_t)gy * W + gx) * 16 + 4 * q;
      v = *reinterpret_cast<const float4*>(map + o);
      if constexpr (MASK) {
        const float4 f = *reinterpret_cast<const float4*>(out + o);
        v = make_float4(dleaky(f.x, v.x), dleaky(f.y, v.y), dleaky(f.z, v.z), dleaky(f.w, v.w));
      }
    }
    img[q * QS + pix] = v;
  }
}

// 3 x 3, pad 1, over the virtual concat of levels 0 .. L-1 -> level L, bias, LeakyReLU (SDNet.py:12-19, :35-37, :40-42)
template <int L>
__global__ __launch_bounds__(256, 2) void dense_fwd_k(const float* __restrict__ pack, float* __restrict__ feat, size_t lvl, int H, int W, int tx, int ty) {
  __shared__ float4 s_x[L * 4 * QS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, st = blockIdx.y, q = lane >> 4, p = lane & 15;
  const int b = blockIdx.x / (tx * ty), rem = blockIdx.x - b * tx * ty, by = rem / tx, bx = rem - by * tx;
  const int y0 = by * DT, x0 = bx * DT;
  float* base = feat + (size_t)st * 4 * lvl + (size_t)b * H * W * 16;   // level 0 of this stream and image

  const float4* __restrict__ wp = reinterpret_cast<const float4*>(pack + PK_FWD + dense_off(L) + st * L * 2304) + lane;
  float4 w[L * 9];
#pragma unroll
  for (int i = 0; i < L * 9; ++i) w[i] = wp[i * 64];

#pragma unroll
  for (int s = 0; s < L; ++s) stage_tile<false>(s_x + s * 4 * QS, base + s * lvl, nullptr, y0, x0, H, W, tid);
  __syncthreads();

  f32x4 acc[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) acc[r] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int r0 = 4 * wave;
#pragma unroll
  for (int s = 0; s < L; ++s)
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) {
      float4 xv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = s_x[(s * 4 + q) * QS + (r0 + r + tap / 3) * DP + p + tap % 3];
      const float4 wv = w[s * 9 + tap];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, xv[r].x, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, xv[r].y, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, xv[r].z, acc[r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, xv[r].w, acc[r], 0, 0, 0);
    }

  const float4 bs = *reinterpret_cast<const float4*>(pack + PK_DENSE_B + ((L - 1) * 2 + st) * 16 + 4 * q);
  const int gx = x0 + p;
  if (gx >= W) return;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int gy = y0 + r0 + r;
    if (gy >= H) continue;
    *reinterpret_cast<float4*>(base + L * lvl + ((size_t)gy * W + gx) * 16 + 4 * q) =
        make_float4(leaky(acc[r][0] + bs.x), leaky(acc[r][1] + bs.y), leaky(acc[r][2] + bs.z), leaky(acc[r][3] + bs.w));
  }
}

// Reverse of dense_fwd_k<L>: dz = dfeat[L] * (feat[L] > 0 ? 1 : 0.01) on the tile + halo 1, then for every source level s < L
//   dfeat[s][p][ci] += sum over tap, co of W_L[co][16 s + ci][tap] * dz[p - (tap - centre)][co]      (M = ci, N = 16 pixels, K = 144)
template <int L>
__global__ __launch_bounds__(256, 2) void dense_bwd_k(const float* __restrict__ pack, const float* __restrict__ feat, float* __restrict__ dfeat,
                                                      size_t lvl, int H, int W, int tx, int ty) {
  __shared__ float4 s_z[4 * QS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, st = blockIdx.y, q = lane >> 4, p = lane & 15;
  const int b = blockIdx.x / (tx * ty), rem = blockIdx.x - b * tx * ty, by = rem / tx, bx = rem - by * tx;
  const int y0 = by * DT, x0 = bx * DT;
  const size_t off = (size_t)st * 4 * lvl + (size_t)b * H * W * 16;

  const float4* __restrict__ wp = reinterpret_cast<const float4*>(pack + PK_BWD + dense_off(L) + st * L * 2304) + lane;
  float4 w[L * 9];
#pragma unroll
  for (int i = 0; i < L * 9; ++i) w[i] = wp[i * 64];

  stage_tile<true>(s_z, dfeat + off + L * lvl, feat + off + L * lvl, y0, x0, H, W, tid);
  __syncthreads();

  f32x4 acc[L][4];
#pragma unroll
  for (int s = 0; s < L; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[s][r] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int r0 = 4 * wave;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    float4 zv[4];   // the output pixel p - (tap - centre) read this pixel through tap
#pragma unroll
    for (int r = 0; r < 4; ++r) zv[r] = s_z[q * QS + (r0 + r + 2 - tap / 3) * DP + p + 2 - tap % 3];
#pragma unroll
    for (int s = 0; s < L; ++s) {
      const float4 wv = w[s * 9 + tap];
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[s][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.x, zv[r].x, acc[s][r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[s][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.y, zv[r].y, acc[s][r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[s][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.z, zv[r].z, acc[s][r], 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[s][r] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv.w, zv[r].w, acc[s][r], 0, 0, 0);
    }
  }

  const int gx = x0 + p;
  if (gx >= W) return;
#pragma unroll
  for (int s = 0; s < L; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gy = y0 + r0 + r;
      if (gy >= H) continue;
      float4* o = reinterpret_cast<float4*>(dfeat + off + s * lvl + ((size_t)gy * W + gx) * 16 + 4 * q);   // owned by this lane
      const float4 v = *o;
      *o = make_float4(v.x + acc[s][r][0], v.y + acc[s][r][1], v.z + acc[s][r][2], v.w + acc[s][r][3]);
    }
}

// ---- fuse: 1 x 1 over the eight maps, 128 -> 1, bias, tanh (SDNet.py:21, :44).  Four lanes per pixel, one channel quad each -------------
__global__ __launch_bounds__(256) void fuse_fwd_k(const float* __restrict__ pack, const float* __restrict__ feat, size_t lvl, float* __restrict__ out,
                                                  size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int q = threadIdx.x & 3;
  const size_t pix = i < n ? i : n - 1;   // every lane takes part in the shuffles
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 v = *reinterpret_cast<const float4*>(feat + k * lvl + pix * 16 + 4 * q);
    const float4 wv = *reinterpret_cast<const float4*>(pack + PK_FUSE_W + k * 16 + 4 * q);
    s += (wv.x * v.x + wv.y * v.y) + (wv.z * v.z + wv.w * v.w);
  }
  s += __shfl_xor(s, 1);
  s += __shfl_xor(s, 2);
  if (q == 0 && i < n) out[i] = tanhf(s + pack[PK_FUSE_B]);
}

// dy = g * (1 - out^2); WRITES the eight gradient maps as w_fuse[k * 16 + c] * dy
__global__ __launch_bounds__(256) void fuse_bwd_k(const float* __restrict__ pack, const float* __restrict__ out, const float* __restrict__ g,
                                                  float* __restrict__ dfeat, size_t lvl, size_t n) {
  const size_t i = (size_t)blockIdx.x * 64 + (threadIdx.x >> 2);
  const int q = threadIdx.x & 3;
  if (i >= n) return;
  const float o = out[i], dy = g[i] * ((1.f - o) * (1.f + o));
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float4 wv = *reinterpret_cast<const float4*>(pack + PK_FUSE_W + k * 16 + 4 * q);
    *reinterpret_cast<float4*>(dfeat + k * lvl + i * 16 + 4 * q) = make_float4(wv.x * dy, wv.y * dy, wv.z * dy, wv.w * dy);
  }
}

// ---- stem, reverse: dz0 = dfeat[0] * mask; d_plane[p] = sum over tap, co of w[co][tap] * dz0[p - (tap - centre)][co] --------------------
constexpr int SQS = 448;   // quad stride in float4: SPH * SPW = 432 rounded up to a multiple of 16
static_assert(SQS >= SPH * SPW && SQS % 16 == 0, "quad planes start at the same LDS bank");

__global__ __launch_bounds__(256) void stem_bwd_k(const float* __restrict__ pack, const float* __restrict__ feat, const float* __restrict__ dfeat, size_t lvl,
                                                  float* __restrict__ d1, float* __restrict__ d2, int H, int W, int tx, int ty) {
  __shared__ float4 s_z[4 * SQS];
  const int tid = threadIdx.x, st = blockIdx.y;
  const int b = blockIdx.x / (tx * ty), rem = blockIdx.x - b * tx * ty, by = rem / tx, bx = rem - by * tx;
  const int y0 = by * SH, x0 = bx * SW;
  const size_t off = (size_t)st * 4 * lvl + (size_t)b * H * W * 16;
  for (int e = tid; e < SPH * SPW * 4; e += 256) {
    const int q = e & 3, pix = e >> 2, ly = pix / SPW, lx = pix - ly * SPW, gy = y0 - 2 + ly, gx = x0 - 2 + lx;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W) {
      const size_t o = off + ((size_t)gy * W + gx) * 16 + 4 * q;
      const float4 f = *reinterpret_cast<const float4*>(feat + o), g = *reinterpret_cast<const float4*>(dfeat + o);
      v = make_float4(dleaky(f.x, g.x), dleaky(f.y, g.y), dleaky(f.z, g.z), dleaky(f.w, g.w));
    }
    s_z[q * SQS + pix] = v;
  }
  __syncthreads();
  const int ly = tid >> 5, lx = tid & 31, gy = y0 + ly, gx = x0 + lx;
  const float* __restrict__ wt = pack + PK_STEM_W + st * 400;
  float s[4] = {0.f, 0.f, 0.f, 0.f};   // one partial sum per channel quad
#pragma unroll
  for (int k = 0; k < 25; ++k) {
    const int pix = (ly + 4 - k / 5) * SPW + lx + 4 - k % 5;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 z = s_z[q * SQS + pix];
      const float* wk = wt + k * 16 + 4 * q;
      s[q] = fmaf(wk[0], z.x, s[q]);
      s[q] = fmaf(wk[1], z.y, s[q]);
      s[q] = fmaf(wk[2], z.z, s[q]);
      s[q] = fmaf(wk[3], z.w, s[q]);
    }
  }
  if (gy >= H || gx >= W) return;
  (st ? d2 : d1)[((size_t)b * H + gy) * W + gx] = (s[0] + s[1]) + (s[2] + s[3]);
}

}  // namespace

extern "C" size_t paif_sdnet_pack_floats(void) { return (size_t)PK_FLOATS; }

extern "C" int paif_sdnet_pack_conv(const float* w, const float* b, int layer, int stream_index, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && pack, PAIF_EINVAL, "sdnet_pack_conv: null pointer");
  PAIF_REQUIRE(layer >= 0 && layer <= 4, PAIF_EINVAL, "sdnet_pack_conv: layer %d outside [0, 4]", layer);
  PAIF_REQUIRE(stream_index == 0 || stream_index == 1, PAIF_EINVAL, "sdnet_pack_conv: encoder %d outside [0, 1]", stream_index);
  const int n = layer == 0 ? 400 : layer == 4 ? 128 : layer * 2304;
  hipLaunchKernelGGL(pack_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), w, b, layer, stream_index, pack);
  PAIF_LAUNCH_CHECK("sdnet_pack_conv");
  return 0;
}

#define SDNET_SHAPE(name)                                                                                  \
  PAIF_REQUIRE(B >= 1 && H >= 1 && W >= 1, PAIF_EINVAL, name ": bad shape %d x %d x %d", B, H, W);           \
  PAIF_REQUIRE((size_t)B* H* W < ((size_t)1 << 31), PAIF_EINVAL, name ": more than 2^31 pixels");            \
  const size_t lvl = (size_t)B * H * W * 16; /* floats of one level of one encoder */                        \
  (void)lvl
#define SDNET_TILES(name, TW, TH)                                                                          \
  const int tx = (W + TW - 1) / TW, ty = (H + TH - 1) / TH;                                                  \
  PAIF_REQUIRE((size_t)tx* ty* B < ((size_t)1 << 31), PAIF_EINVAL, name ": too many tiles");                 \
  const dim3 grid((unsigned)(tx * ty * B), 2)

extern "C" int paif_sdnet_stem_fwd(const float* x1, size_t sb1, const float* x2, size_t sb2, const float* pack, float* feat, int B, int H, int W,
                                   paif_stream_t stream) {
  PAIF_REQUIRE(x1 && x2 && pack && feat, PAIF_EINVAL, "sdnet_stem_fwd: null pointer");
  SDNET_SHAPE("sdnet_stem_fwd");
  PAIF_REQUIRE((size_t)H * W <= sb1 && (size_t)H * W <= sb2, PAIF_EINVAL, "sdnet_stem_fwd: batch stride smaller than a plane");
  SDNET_TILES("sdnet_stem_fwd", SW, SH);
  hipLaunchKernelGGL(stem_fwd_k, grid, dim3(256), 0, paif::as_stream(stream), x1, sb1, x2, sb2, pack, feat, lvl, H, W, tx, ty);
  PAIF_LAUNCH_CHECK("sdnet_stem_fwd");
  return 0;
}

extern "C" int paif_sdnet_dense_fwd(const float* pack, float* feat, int level, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && feat, PAIF_EINVAL, "sdnet_dense_fwd: null pointer");
  PAIF_REQUIRE(level >= 1 && level <= 3, PAIF_EINVAL, "sdnet_dense_fwd: level %d outside [1, 3]", level);
  SDNET_SHAPE("sdnet_dense_fwd");
  SDNET_TILES("sdnet_dense_fwd", DT, DT);
  const hipStream_t s = paif::as_stream(stream);
  if (level == 1) hipLaunchKernelGGL(dense_fwd_k<1>, grid, dim3(256), 0, s, pack, feat, lvl, H, W, tx, ty);
  else if (level == 2) hipLaunchKernelGGL(dense_fwd_k<2>, grid, dim3(256), 0, s, pack, feat, lvl, H, W, tx, ty);
  else hipLaunchKernelGGL(dense_fwd_k<3>, grid, dim3(256), 0, s, pack, feat, lvl, H, W, tx, ty);
  PAIF_LAUNCH_CHECK("sdnet_dense_fwd");
  return 0;
}

extern "C" int paif_sdnet_fuse_fwd(const float* pack, const float* feat, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && feat && out, PAIF_EINVAL, "sdnet_fuse_fwd: null pointer");
  SDNET_SHAPE("sdnet_fuse_fwd");
  const size_t n = (size_t)B * H * W;
  hipLaunchKernelGGL(fuse_fwd_k, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, paif::as_stream(stream), pack, feat, lvl, out, n);
  PAIF_LAUNCH_CHECK("sdnet_fuse_fwd");
  return 0;
}

extern "C" int paif_sdnet_fuse_bwd(const float* pack, const float* out, const float* d_out, float* dfeat, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && out && d_out && dfeat, PAIF_EINVAL, "sdnet_fuse_bwd: null pointer");
  SDNET_SHAPE("sdnet_fuse_bwd");
  const size_t n = (size_t)B * H * W;
  hipLaunchKernelGGL(fuse_bwd_k, dim3((unsigned)((n + 63) / 64)), dim3(256), 0, paif::as_stream(stream), pack, out, d_out, dfeat, lvl, n);
  PAIF_LAUNCH_CHECK("sdnet_fuse_bwd");
  return 0;
}

extern "C" int paif_sdnet_dense_bwd(const float* pack, const float* feat, float* dfeat, int level, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && feat && dfeat, PAIF_EINVAL, "sdnet_dense_bwd: null pointer");
  PAIF_REQUIRE(feat != dfeat, PAIF_EINVAL, "sdnet_dense_bwd: the gradient maps must not alias the taped maps");
  PAIF_REQUIRE(level >= 1 && level <= 3, PAIF_EINVAL, "sdnet_dense_bwd: level %d outside [1, 3]", level);
  SDNET_SHAPE("sdnet_dense_bwd");
  SDNET_TILES("sdnet_dense_bwd", DT, DT);
  const hipStream_t s = paif::as_stream(stream);
  if (level == 1) hipLaunchKernelGGL(dense_bwd_k<1>, grid, dim3(256), 0, s, pack, feat, dfeat, lvl, H, W, tx, ty);
  else if (level == 2) hipLaunchKernelGGL(dense_bwd_k<2>, grid, dim3(256), 0, s, pack, feat, dfeat, lvl, H, W, tx, ty);
  else hipLaunchKernelGGL(dense_bwd_k<3>, grid, dim3(256), 0, s, pack, feat, dfeat, lvl, H, W, tx, ty);
  PAIF_LAUNCH_CHECK("sdnet_dense_bwd");
  return 0;
}

extern "C" int paif_sdnet_stem_bwd(const float* pack, const float* feat, const float* dfeat, float* d_x1, float* d_x2, int B, int H, int W,
                                   paif_stream_t stream) {
  PAIF_REQUIRE(pack && feat && dfeat && d_x1 && d_x2, PAIF_EINVAL, "sdnet_stem_bwd: null pointer");
  SDNET_SHAPE("sdnet_stem_bwd");
  SDNET_TILES("sdnet_stem_bwd", SW, SH);
  hipLaunchKernelGGL(stem_bwd_k, grid, dim3(256), 0, paif::as_stream(stream), pack, feat, dfeat, lvl, d_x1, d_x2, H, W, tx, ty);
  PAIF_LAUNCH_CHECK("sdnet_stem_bwd");
  return 0;
}
