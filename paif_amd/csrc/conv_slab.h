// The SLAB CONV: an exact-fp32 implicit GEMM on v_mfma_f32_16x16x4_f32 over a slice of an NHWC concat slab, shaped by template / argument
// (u2fusion.hip, seafusion.hip, didfuse.hip, bffusion.hip and drdb.hip all run on it; their shared host scaffolding is at the end):
//   * TAPS: 9 (3 x 3, zero pad 1) or 1 (1 x 1: no halo is staged);
//   * MB in {1, 2, 3, 4} blocks of 16 output channels per workgroup (plan_for(): a 16-channel output spends no instruction on zeros);
//   * the LeakyReLU slope is an argument: of the store epilogue (EPI_ACT) or of the input mask (MASK);
//   * EPI_ACT adds up to two biases (a 1 x 1 over two weight matrices side by side sums both convs' biases);
//   * ACT: the activation of the store epilogue and of the input mask is LeakyReLU (the default) or tanh (mask 1 - taped^2);
//   * PAIR: the epilogue also reads the quad another map holds at the same place and stores the mean of the two into a third map;
//   * XIN: the masked staging scales its input (1), and adds a scaled second input before the mask (2); the mask has its own stride;
//   * REFL: REFL_STAGE stages the halo by REFLECTION (row -1 takes row 1, row H takes row H - 2: ReflectionPad2d(1) in front of the conv);
//     REFL_RING is the transpose's half of that: the zero-pad conv evaluated on the (H + 2) x (W + 2) grid, the input read one pixel up
//     and left, the output a ring map [B][H + 2][W + 2][out_cs] that a fold pass adds back onto the plane (bffusion.hip: fold_k).
//   * DIL: the dilation of the 3 x 3 taps, 1 or 2 (zero pad DIL): the staged tile has a halo of DIL (20 x 20 pixels at 2; with MB = 4
//     the static LDS is 4 * 400 + 9 * 4 * 64 float4 = 62464 B of the 64 KB), tap t reads at + DIL (t / 3) rows and + DIL (t % 3) columns;
//   * EPI_RES (1 x 1 only): the residual AFTER the activation, out = x + act(v + b) with x the first channels of the INPUT map at the same
//     pixel; act(v + b) itself goes to `avg` (the tape of the branch: x + r can equal x in fp32 for a small positive r).
//   ReLU is LeakyReLU at slope 0, epilogue and mask alike (a negative input stores -0, which every consumer treats as 0).
// The last five default to what the header did before them: an instantiation that does not name them compiles to the same code.
// Output CHANNELS on M, 16 PIXELS of one image row on N; the D operand of lane l is channels
// 4 (l >> 4) .. + 3 of pixel l & 15, one float4 of the NHWC map, and the B operand of four consecutive instructions is one float4 of the
// input map.  A workgroup of four waves owns a 16 x 16 pixel tile (four rows per wave) and MB blocks of 16 output channels (blockIdx.y
// selects the group of MB blocks).  Per CHUNK of 16 input channels it stages the tile (+ halo 1 for 9 taps; what lies outside the image
// is zero) as four quad planes and the chunk's weights in operand order (TAPS x MB x 1 KB), then per tap reads four pixel float4 and MB
// weight float4 for 16 MB instructions, k ascending: a fixed summation order.  Every output quad is owned by one lane: no atomics.
// A launch must not read channels it writes (EPI_ADD reads and writes its OWN quad only).
// Channel counts: K and M are padded with zeros to multiples of 16 in the staged tile, the pack and the stores (out_n a multiple of 4).
#pragma once
#include "paif_common.h"

namespace paif_slab {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DT = 16;   // tile edge: 4 waves x 4 rows of 16 pixels

enum { EPI_ACT = 0, EPI_STORE = 1, EPI_ADD = 2, EPI_RES = 3 };
enum { ACT_LEAKY = 0, ACT_TANH = 1 };
enum { XIN_PLAIN = 0, XIN_SCALED = 1, XIN_SUM = 2 };
enum { REFL_NONE = 0, REFL_STAGE = 1, REFL_RING = 2 };

// One operand pack: M output channels in `groups` groups of MB blocks of 16, K input channels in `chunks` chunks of 16, `taps` taps.
struct Plan {
  int M, K, MB, groups, chunks, taps;
  __host__ __device__ constexpr size_t floats() const { return (size_t)groups * chunks * taps * MB * 256; }
};
// MB: all blocks in one group up to 4; beyond, the fewest padded blocks among 4 and 3 (a tie takes 4).
__host__ __device__ constexpr Plan plan_for(int M, int K, int taps) {
  const int blocks = (M + 15) / 16;
  const int MB = blocks <= 4 ? blocks : ((blocks + 3) / 4) * 4 <= ((blocks + 2) / 3) * 3 ? 4 : 3;
  return Plan{M, K, MB, (blocks + MB - 1) / MB, (K + 15) / 16, taps};
}

// Operand order: [group][chunk][tap][block mb][lane][j]; A[m = lane & 15][k = lane >> 4] of instruction j is the weight of output channel
// m = 16 (group * MB + mb) + (lane & 15) and input channel k = 16 chunk + 4 (lane >> 4) + j.  `w` is a conv weight [co][n][taps] whose n
// input channels sit at [off, off + n) of the conv's concat (several weights side by side fill one pack).  Forward (M = co, K = concat):
// W[m][k - off][tap]; transposed (M = concat, K = co): W[k][m - off][taps - 1 - tap].  Elements outside [off, off + n) are left alone
// (the pack starts as zeros).
static __global__ void pack_ops_k(const float* __restrict__ w, int co, int n, int off, Plan pl, int transposed, float* __restrict__ dst) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= pl.floats()) return;
  const int j = i & 3, lane = (i >> 2) & 63;
  size_t r = i >> 8;
  const int mb = r % pl.MB;
  r /= pl.MB;
  const int tap = r % pl.taps;
  r /= pl.taps;
  const int c = r % pl.chunks, g = r / pl.chunks;
  const int m = 16 * (g * pl.MB + mb) + (lane & 15), k = 16 * c + 4 * (lane >> 4) + j;
  if (transposed) {
    if (m >= off && m < off + n && k < co) dst[i] = w[((size_t)k * n + (m - off)) * pl.taps + pl.taps - 1 - tap];
  } else {
    if (k >= off && k < off + n && m < co) dst[i] = w[((size_t)m * n + (k - off)) * pl.taps + tap];
  }
}

// reflection padding by one: the row a read at y takes (y in [-1, H]; H >= 2)
__device__ __forceinline__ int refl1(int y, int H) { return y < 0 ? -y : (y >= H ? 2 * H - 2 - y : y); }

__device__ __forceinline__ float leaky(float v, float s) { return v > 0.f ? v : s * v; }
// the branch is read off the taped OUTPUT (same sign as the pre-activation; exactly 0 takes the slope, as torch)
__device__ __forceinline__ float dleaky(float out, float g, float s) { return out > 0.f ? g : s * g; }
__device__ __forceinline__ float4 dleaky4(float4 f, float4 v, float s) {
  return make_float4(dleaky(f.x, v.x, s), dleaky(f.y, v.y, s), dleaky(f.z, v.z, s), dleaky(f.w, v.w, s));
}

// tanh' off the taped OUTPUT t: 1 - t^2, as (1 - t)(1 + t)
__device__ __forceinline__ float dtanh(float t, float g) { return g * ((1.f - t) * (1.f + t)); }
__device__ __forceinline__ float4 dtanh4(float4 t, float4 v) { return make_float4(dtanh(t.x, v.x), dtanh(t.y, v.y), dtanh(t.z, v.z), dtanh(t.w, v.w)); }
template <int ACT>
__device__ __forceinline__ float act_of(float v, float s) {
  if constexpr (ACT == ACT_TANH) return tanhf(v);
  else return leaky(v, s);
}

struct ConvArgs {
  const float* in;      // first channel of the input slice; pixel stride in_cs floats, nq channel quads
  const float* mask;    // MASK: the taped map of the same slice (same stride)
  float* out;           // first channel of the output map; pixel stride out_cs; channels [out_off, out_off + out_n) are written
  const float* wpk;     // operand pack of this conv
  const float* bias;    // EPI_ACT, EPI_RES
  const float* bias2;   // EPI_ACT: a second bias, or null
  float slope;          // LeakyReLU slope: of the stored map (EPI_ACT), of the taped map behind the input (MASK)
  int in_cs, nq, out_cs, out_off, out_n, chunks, H, W, tx, ty;
  // PAIR: `pair` is laid out as `out` (same stride and offset); 0.5 (own + pair) goes to channels [avg_off, avg_off + out_n) of `avg`
  // EPI_RES: act(v + b) goes to channels [avg_off, avg_off + out_n) of `avg`; the residual is channels [0, out_n) of `in`
  const float* pair = nullptr;
  float* avg = nullptr;
  int avg_cs = 0, avg_off = 0;
  // XIN: staged value = mask(in_scale * in [+ in2_scale * in2]); in2 has the stride of in, the mask its own (XIN_PLAIN: in_cs)
  const float* in2 = nullptr;
  float in_scale = 1.f, in2_scale = 1.f;
  int mask_cs = 0;
};

template <int TAPS, int MB, bool MASK, int EPI, int ACT = ACT_LEAKY, bool PAIR = false, int XIN = XIN_PLAIN, int REFL = REFL_NONE, int DIL = 1>
__global__ __launch_bounds__(256, 2) void conv_k(const ConvArgs a) {
  static_assert(TAPS == 9 || TAPS == 1, "3 x 3 or 1 x 1");
  static_assert(!PAIR || EPI == EPI_ACT, "the pair store belongs to the activation epilogue");
  static_assert(XIN == XIN_PLAIN || MASK, "the extended staging is the masked one");
  static_assert(REFL == REFL_NONE || (TAPS == 9 && !PAIR && XIN == XIN_PLAIN), "reflection belongs to the plain 3 x 3 forms");
  static_assert(DIL == 1 || (DIL == 2 && TAPS == 9 && REFL == REFL_NONE), "dilation 2 belongs to the zero-padded 3 x 3 forms");
  static_assert(EPI != EPI_RES || (TAPS == 1 && !MASK && !PAIR), "the residual epilogue belongs to the forward 1 x 1");
  constexpr int HALO = TAPS == 9 ? DIL : 0, DP = DT + 2 * HALO;
  constexpr int QS = (DP * DP + 15) / 16 * 16;   // quad stride in float4, a multiple of 256 B: quad planes start at the same LDS bank
  __shared__ float4 s_x[4 * QS];
  __shared__ float4 s_w[TAPS * MB * 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, q = lane >> 4, p = lane & 15;
  const int H = a.H, W = a.W;                                                          // the INPUT plane
  constexpr int RING = REFL == REFL_RING ? 1 : 0;
  const int Ho = H + 2 * RING, Wo = W + 2 * RING;                                       // the output grid (tx, ty tile it)
  const int b = blockIdx.x / (a.tx * a.ty), rem = blockIdx.x - b * a.tx * a.ty, by = rem / a.tx, bx = rem - by * a.tx;
  const int y0 = by * DT, x0 = bx * DT, r0 = 4 * wave;
  const size_t img = (size_t)b * H * W, imgo = RING ? (size_t)b * Ho * Wo : img;
  const float4* __restrict__ wg = reinterpret_cast<const float4*>(a.wpk) + (size_t)blockIdx.y * a.chunks * (TAPS * MB * 64);

  f32x4 acc[MB][4];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[mb][r] = f32x4{0.f, 0.f, 0.f, 0.f};

  for (int c = 0; c < a.chunks; ++c) {
    if (c) __syncthreads();   // the previous chunk has been read
    for (int e = tid; e < DP * DP * 4; e += 256) {
      const int sq = e & 3, pix = e >> 2, ly = pix / DP, lx = pix - ly * DP, gq = 4 * c + sq;
      int gy = y0 - HALO - RING + ly, gx = x0 - HALO - RING + lx;
      if constexpr (REFL == REFL_STAGE) gy = refl1(gy, H), gx = refl1(gx, W);   // rows past H + 1 may leave the plane again: zero
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if ((unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W && gq < a.nq) {
        const size_t o = (img + (size_t)gy * W + gx) * a.in_cs + 4 * gq;
        v = *reinterpret_cast<const float4*>(a.in + o);
        if constexpr (XIN != XIN_PLAIN) {
          v = make_float4(a.in_scale * v.x, a.in_scale * v.y, a.in_scale * v.z, a.in_scale * v.w);
          if constexpr (XIN == XIN_SUM) {
            const float4 u = *reinterpret_cast<const float4*>(a.in2 + o);
            v = make_float4(fmaf(a.in2_scale, u.x, v.x), fmaf(a.in2_scale, u.y, v.y), fmaf(a.in2_scale, u.z, v.z), fmaf(a.in2_scale, u.w, v.w));
          }
        }
        if constexpr (MASK) {
          const size_t om = XIN == XIN_PLAIN ? o : (img + (size_t)gy * W + gx) * a.mask_cs + 4 * gq;
          const float4 f = *reinterpret_cast<const float4*>(a.mask + om);
          if constexpr (ACT == ACT_TANH) v = dtanh4(f, v);
          else v = dleaky4(f, v, a.slope);
        }
      }
      s_x[sq * QS + pix] = v;
    }
    const float4* __restrict__ wc = wg + (size_t)c * (TAPS * MB * 64);
    for (int e = tid; e < TAPS * MB * 64; e += 256) s_w[e] = wc[e];
    __syncthreads();
#pragma unroll
    for (int tap = 0; tap < TAPS; ++tap) {
      float4 xv[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) xv[r] = s_x[q * QS + (r0 + r + (HALO ? DIL * (tap / 3) : 0)) * DP + p + (HALO ? DIL * (tap % 3) : 0)];
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
  if (gx >= Wo) return;
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int co = 16 * ((int)blockIdx.y * MB + mb) + 4 * q;   // out_n is a multiple of 4: a quad is written whole or not at all
    if (co >= a.out_n) continue;
    float4 bs = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (EPI == EPI_ACT || EPI == EPI_RES) {
      bs = *reinterpret_cast<const float4*>(a.bias + co);
      if (a.bias2) {
        const float4 b2 = *reinterpret_cast<const float4*>(a.bias2 + co);
        bs = make_float4(bs.x + b2.x, bs.y + b2.y, bs.z + b2.z, bs.w + b2.w);
      }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int gy = y0 + r0 + r;
      if (gy >= Ho) continue;
      const size_t px = imgo + (size_t)gy * Wo + gx;
      float4* o = reinterpret_cast<float4*>(a.out + px * a.out_cs + a.out_off + co);   // owned by this lane
      const f32x4 v = acc[mb][r];
      if constexpr (EPI == EPI_ACT) {
        const float4 f = make_float4(act_of<ACT>(v[0] + bs.x, a.slope), act_of<ACT>(v[1] + bs.y, a.slope), act_of<ACT>(v[2] + bs.z, a.slope),
                                     act_of<ACT>(v[3] + bs.w, a.slope));
        *o = f;
        if constexpr (PAIR) {   // the other stream's quad at this place was stored by an earlier launch; the mean's quad is this lane's too
          const float4 u = *reinterpret_cast<const float4*>(a.pair + px * a.out_cs + a.out_off + co);
          *reinterpret_cast<float4*>(a.avg + px * a.avg_cs + a.avg_off + co) =
              make_float4(0.5f * (u.x + f.x), 0.5f * (u.y + f.y), 0.5f * (u.z + f.z), 0.5f * (u.w + f.w));
        }
      } else if constexpr (EPI == EPI_RES) {   // the input map is not the output map: its quad is read, never written, by this launch
        const float4 f = make_float4(act_of<ACT>(v[0] + bs.x, a.slope), act_of<ACT>(v[1] + bs.y, a.slope), act_of<ACT>(v[2] + bs.z, a.slope),
                                     act_of<ACT>(v[3] + bs.w, a.slope));
        const float4 u = *reinterpret_cast<const float4*>(a.in + px * a.in_cs + co);
        *reinterpret_cast<float4*>(a.avg + px * a.avg_cs + a.avg_off + co) = f;
        *o = make_float4(u.x + f.x, u.y + f.y, u.z + f.z, u.w + f.w);
      } else if constexpr (EPI == EPI_STORE) {
        *o = make_float4(v[0], v[1], v[2], v[3]);
      } else {
        const float4 u = *o;
        *o = make_float4(u.x + v[0], u.y + v[1], u.z + v[2], u.w + v[3]);
      }
    }
  }
}

template <int TAPS, bool MASK, int EPI>
void launch_conv(int MB, dim3 grid, hipStream_t s, const ConvArgs& a) {
  if (MB == 4) hipLaunchKernelGGL((conv_k<TAPS, 4, MASK, EPI>), grid, dim3(256), 0, s, a);
  else if (MB == 3) hipLaunchKernelGGL((conv_k<TAPS, 3, MASK, EPI>), grid, dim3(256), 0, s, a);
  else if (MB == 2) hipLaunchKernelGGL((conv_k<TAPS, 2, MASK, EPI>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_k<TAPS, 1, MASK, EPI>), grid, dim3(256), 0, s, a);
}
// the 3 x 3 forms with reflection: REFL_STAGE (forward) or REFL_RING (transposed, onto the ring map)
template <bool MASK, int EPI, int REFL>
void launch_conv_r(int MB, dim3 grid, hipStream_t s, const ConvArgs& a) {
  if (MB == 4) hipLaunchKernelGGL((conv_k<9, 4, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL>), grid, dim3(256), 0, s, a);
  else if (MB == 3) hipLaunchKernelGGL((conv_k<9, 3, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL>), grid, dim3(256), 0, s, a);
  else if (MB == 2) hipLaunchKernelGGL((conv_k<9, 2, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((conv_k<9, 1, MASK, EPI, ACT_LEAKY, false, XIN_PLAIN, REFL>), grid, dim3(256), 0, s, a);
}
// the 3 x 3, MB = 4 form with the later template parameters named
template <bool MASK, int EPI, int ACT, bool PAIR, int XIN>
void launch_conv4(dim3 grid, hipStream_t s, const ConvArgs& a) {
  hipLaunchKernelGGL((conv_k<9, 4, MASK, EPI, ACT, PAIR, XIN>), grid, dim3(256), 0, s, a);
}

// ---- host scaffolding of the networks on the slab conv ----------------------------------------------------------------------------------
inline void pack_ops(const float* w, int co, int n, int off, const Plan& pl, int transposed, float* dst, hipStream_t s) {
  hipLaunchKernelGGL(pack_ops_k, dim3((unsigned)((pl.floats() + 255) / 256)), dim3(256), 0, s, w, co, n, off, pl, transposed, dst);
}
// What every launch fills the same way: the plane, its tiling, the plan's chunks.  Pointers start null, the slope 0, the scales 1: a call
// site names the pointers, strides, offsets and slope its form reads.
inline ConvArgs conv_args(const Plan& pl, int H, int W, int tx, int ty) {
  ConvArgs a{};
  a.chunks = pl.chunks, a.H = H, a.W = W, a.tx = tx, a.ty = ty;
  return a;
}
inline dim3 conv_grid(const Plan& pl, int B, int tx, int ty) { return dim3((unsigned)(tx * ty * B), (unsigned)pl.groups); }

// ---- a 3 x 3, zero pad 1, 32 -> 1 head on the vector unit (U2Fusion's sub.3 with tanh, DRDB's conv21 with PReLU).  hp: the weights
// [tap 9][ci 32] through the scalar cache, then the bias; tap ascending, channel quad ascending.  One pixel per thread --------------------
template <int ACT>
__global__ __launch_bounds__(256) void head32_fwd_k(const float* __restrict__ hp, float slope, const float* __restrict__ in, float* __restrict__ out,
                                                    int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s = 0.f;
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const float* __restrict__ src = in + ((size_t)b * hw + (size_t)gy * W + gx) * 32;
    const float* __restrict__ wt = hp + tap * 32;
#pragma unroll
    for (int c = 0; c < 32; c += 4) {
      const float4 v = *reinterpret_cast<const float4*>(src + c);
      s = fmaf(wt[c], v.x, s), s = fmaf(wt[c + 1], v.y, s), s = fmaf(wt[c + 2], v.z, s), s = fmaf(wt[c + 3], v.w, s);
    }
  }
  out[i] = act_of<ACT>(s + hp[9 * 32], slope);
}
// Reverse: dy = g through the activation's derivative off the taped OUTPUT; d_in[p][ci] = sum over tap of W[ci][tap] * dy[p - (tap - centre)].
// Eight lanes per pixel, one channel quad each; WRITES d_in.
template <int ACT>
__global__ __launch_bounds__(256) void head32_bwd_k(const float* __restrict__ hp, float slope, const float* __restrict__ out, const float* __restrict__ g,
                                                    float* __restrict__ din, int H, int W, size_t n) {
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
    const float dy = ACT == ACT_TANH ? dtanh(out[o], g[o]) : dleaky(out[o], g[o], slope);
    const float4 wv = *reinterpret_cast<const float4*>(hp + tap * 32 + 4 * cq);
    s.x = fmaf(wv.x, dy, s.x), s.y = fmaf(wv.y, dy, s.y), s.z = fmaf(wv.z, dy, s.z), s.w = fmaf(wv.w, dy, s.w);
  }
  *reinterpret_cast<float4*>(din + i * 32 + 4 * cq) = s;
}

}  // namespace paif_slab

// ---- the shape checks of an entry point with B, H, W in scope: an image of at least min_hw x min_hw (`why` is what the message says about
// a minimum above 1), fewer than 2^cap pixels; defines n = B H W.  PAIF_SLAB_TILES defines the tiling tx, ty of the slab conv ------------
#define PAIF_SLAB_SHAPE(name, min_hw, why, cap)                                                                    \
  PAIF_REQUIRE(B >= 1 && H >= min_hw && W >= min_hw, PAIF_EINVAL, name ": bad shape %d x %d x %d" why, B, H, W);     \
  PAIF_REQUIRE((size_t)B* H* W < ((size_t)1 << cap), PAIF_EINVAL, name ": more than 2^" #cap " pixels");             \
  const size_t n = (size_t)B * H * W;                                                                              \
  (void)n
#define PAIF_SLAB_TILES(name)                                                                                      \
  const int tx = (W + paif_slab::DT - 1) / paif_slab::DT, ty = (H + paif_slab::DT - 1) / paif_slab::DT;              \
  PAIF_REQUIRE((size_t)tx* ty* B < ((size_t)1 << 31), PAIF_EINVAL, name ": too many tiles")
