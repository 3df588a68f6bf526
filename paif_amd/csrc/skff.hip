// SKFF, the selective-kernel feature fusion block of the reference (core/model_fusion_auto.py:190-224, the same class in operations_m.py),
// and what Fusion_Network2 (:227-260) needs beyond the DRDB entry points of drdb.hip.
//   SKFF(64, n, reduction, bias), d = max(int(64 / reduction), 4), inputs X_0 .. X_{n-1} [B][H][W][64]:
//     S[b][c] = mean over pixels of sum_h X_h;  z = W1 S + b1 (d values);  Z = PReLU(z);  A_h = W2_h Z + b2_h (64 values each);
//     a[b][.][c] = softmax over h of A_h[b][c];  V = sum_h a[b][h][c] X_h.
//   Reverse, given dV: da[b][h][c] = sum over pixels of dV X_h;  dA_h = a_h (da_h - sum_k a_k da_k);  dZ = sum_h W2_h^T dA_h;
//     dz = dZ where z > 0, slope dZ otherwise (exactly 0 takes the slope, as torch);  dS = W1^T dz;  dX_h = a_h dV + dS / (H W).
//   Fusion_Network2: x = PReLU(conv1(cat(ir, vis))); f1 = DRDB1(x); v1 = skff([f1, conv3 1x1 64 -> 64 (out1)]); f2 = DRDB2(v1);
//     v2 = skff2([f2, conv4 1x1 128 -> 64 (out2)]); f = PReLU(conv2 3x3 64 -> 1 (v2)); fused = (f - min f) / (max f - min f), min and max
//     over the whole batch, NO clamp.  conv1, DRDB1 and DRDB2 are the paif_drdb_* entry points.
//
// LAYOUT.  fp32 NHWC.  Every SKFF input has its own pixel stride (a map may be the first 64 channels of a 224-channel slab); V is written
// with its own pixel stride and channel offset (skff writes into [0, 64) of DRDB2's slab); dV is read with its own stride ([0, 64) of
// DRDB2's d_slab).  a [B][n][64], z [B][d] (the tape of the gate: the PReLU branch is read off z, so any slope is allowed in the gate),
// dS [B][64].  The gate's pack: W1 [d][64], b1 [d], W2 [n][64][d], b2 [n][64] (zeros where the module has no bias).
//
// LAUNCHES.  Forward: pool (per workgroup the sum of SK_PIX pixels of one image over the n inputs -> partial [B][blocks][64]), gate (one
// workgroup per image: the partials in block order in double, the two small products and the softmax in double, stored fp32), apply.
// Reverse: reduce (partial [B][blocks][n][64] of da), gate-reverse (-> dS), apply-reverse.  Sixteen lanes per pixel, one channel quad
// (float4) per lane; inside a workgroup the sixteen pixel rows meet in LDS in a fixed tree.  No atomics: every output element is owned
// by one lane, every sum has one order.  No allocation, no host synchronisation: capturable.
//
// The 1 x 1 convs conv3 / conv4 run on the slab conv (conv_slab.h) at slope 1 -- LeakyReLU at slope 1 is the identity, so the epilogue
// adds the bias and nothing else; their transposes are EPI_STORE on transposed packs.  The 64 -> 1 head and its reverse run on the
// vector unit; the reverse reads the PReLU branch off the taped f, so that slope must be >= 0.
#include <math.h>
#include <stdint.h>

#include "conv_slab.h"

namespace {

using namespace paif_slab;

constexpr int CX = 64;         // the width SKFF is built for
constexpr int SK_PIX = 512;    // pixels per pool / reduce / apply workgroup: B = 8 at 480 x 640 gives 4800 workgroups, ~19 per CU
constexpr int SK_ROWS = 16;    // pixel rows of a workgroup: 256 lanes = 16 rows x 16 channel quads
constexpr int SK_MAXN = 3, SK_MAXD = 64;

struct SkIn {
  const float* x[SK_MAXN];
  int cs[SK_MAXN];
};
struct SkOut {
  float* x[SK_MAXN];
};

__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }
__device__ __forceinline__ float4 fma4(float4 a, float4 b, float4 c) {
  return make_float4(fmaf(a.x, b.x, c.x), fmaf(a.y, b.y, c.y), fmaf(a.z, b.z, c.z), fmaf(a.w, b.w, c.w));
}
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// the sixteen rows of sm (one float4 per lane) into row 0: rows r and r + 8, then + 4, + 2, + 1.  Ends behind a barrier.
__device__ __forceinline__ void rows_to_row0(float4* sm, int tid) {
  __syncthreads();
#pragma unroll
  for (int st = 128; st >= 16; st >>= 1) {
    if (tid < st) sm[tid] = add4(sm[tid], sm[tid + st]);
    __syncthreads();
  }
}

// the pixels [p0, p1) of image blockIdx.y that workgroup blockIdx.x owns
__device__ __forceinline__ void block_span(size_t hw, size_t& p0, size_t& p1) {
  p0 = (size_t)blockIdx.x * SK_PIX;
  p1 = p0 + SK_PIX < hw ? p0 + SK_PIX : hw;
}

// ---- pool: partial[b][block][64] = sum over the block's pixels of (X_0 + .. + X_{n-1}) -----------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void pool_k(const SkIn in, float* __restrict__ partial, size_t hw) {
  __shared__ float4 sm[256];
  const int tid = threadIdx.x, q = tid & 15, r = tid >> 4, b = blockIdx.y;
  size_t p0, p1;
  block_span(hw, p0, p1);
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t px = p0 + r; px < p1; px += SK_ROWS) {
    const size_t o = (size_t)b * hw + px;
    float4 v = ld4(in.x[0] + o * in.cs[0] + 4 * q);
#pragma unroll
    for (int h = 1; h < N; ++h) v = add4(v, ld4(in.x[h] + o * in.cs[h] + 4 * q));
    acc = add4(acc, v);
  }
  sm[tid] = acc;
  rows_to_row0(sm, tid);
  if (tid < 16) *reinterpret_cast<float4*>(partial + ((size_t)b * gridDim.x + blockIdx.x) * CX + 4 * tid) = sm[tid];
}

// per image: out[c] (c < count, in LDS) = the partials' element c summed over the blocks in block order, in double.  Four lanes per
// element take a quarter of the blocks each, a contiguous run in ascending order; the four runs are added in ascending order.
__device__ __forceinline__ void finish_partials(const float* __restrict__ partial, int nblk, int count, double* s_part, double* out, int tid) {
  const int per = (nblk + 3) / 4;
  for (int e = tid; e < 4 * count; e += 256) {
    const int c = e % count, part = e / count;
    const int k0 = part * per, k1 = k0 + per < nblk ? k0 + per : nblk;
    double s = 0.0;
    for (int k = k0; k < k1; ++k) s += (double)partial[(size_t)k * count + c];
    s_part[e] = s;
  }
  __syncthreads();
  for (int c = tid; c < count; c += 256) out[c] = ((s_part[c] + s_part[count + c]) + s_part[2 * count + c]) + s_part[3 * count + c];
  __syncthreads();
}

// pack offsets (floats) of the gate's parameters
struct SkPack {
  int w1, b1, w2, b2, floats;
};
__host__ __device__ inline SkPack sk_pack(int n, int d) {
  SkPack p;
  p.w1 = 0, p.b1 = d * CX, p.w2 = p.b1 + d, p.b2 = p.w2 + n * CX * d, p.floats = p.b2 + n * CX;
  return p;
}

// ---- gate: one workgroup per image ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_k(const float* __restrict__ partial, int nblk, const float* __restrict__ pack, float slope, int n, int d,
                                              double inv_hw, float* __restrict__ a, float* __restrict__ z) {
  __shared__ double s_part[4 * CX], s_S[CX], s_Z[SK_MAXD], s_A[SK_MAXN * CX];
  const int tid = threadIdx.x, b = blockIdx.x;
  const SkPack pk = sk_pack(n, d);
  finish_partials(partial + (size_t)b * nblk * CX, nblk, CX, s_part, s_S, tid);
  if (tid < d) {
    double s = (double)pack[pk.b1 + tid];
    const float* __restrict__ w = pack + pk.w1 + tid * CX;
    for (int c = 0; c < CX; ++c) s += (double)w[c] * (s_S[c] * inv_hw);
    const float zf = (float)s;       // the taped value decides the branch, forward and reverse alike
    z[(size_t)b * d + tid] = zf;
    s_Z[tid] = zf > 0.f ? (double)zf : (double)slope * (double)zf;
  }
  __syncthreads();
  if (tid < n * CX) {
    double s = (double)pack[pk.b2 + tid];
    const float* __restrict__ w = pack + pk.w2 + (size_t)tid * d;
    for (int j = 0; j < d; ++j) s += (double)w[j] * s_Z[j];
    s_A[tid] = s;
  }
  __syncthreads();
  if (tid < CX) {
    double m = s_A[tid];
    for (int h = 1; h < n; ++h) m = fmax(m, s_A[h * CX + tid]);
    double e[SK_MAXN], sum = 0.0;
    for (int h = 0; h < n; ++h) e[h] = exp(s_A[h * CX + tid] - m), sum += e[h];
    for (int h = 0; h < n; ++h) a[((size_t)b * n + h) * CX + tid] = (float)(e[h] / sum);
  }
}

// ---- apply: V = sum_h a_h X_h ---------------------------------------------------------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void apply_k(const SkIn in, const float* __restrict__ a, float* __restrict__ v, int v_cs, int v_off, size_t hw) {
  const int tid = threadIdx.x, q = tid & 15, r = tid >> 4, b = blockIdx.y;
  size_t p0, p1;
  block_span(hw, p0, p1);
  float4 w[N];
#pragma unroll
  for (int h = 0; h < N; ++h) w[h] = ld4(a + ((size_t)b * N + h) * CX + 4 * q);
  for (size_t px = p0 + r; px < p1; px += SK_ROWS) {
    const size_t o = (size_t)b * hw + px;
    const float4 x0 = ld4(in.x[0] + o * in.cs[0] + 4 * q);
    float4 s = make_float4(w[0].x * x0.x, w[0].y * x0.y, w[0].z * x0.z, w[0].w * x0.w);
#pragma unroll
    for (int h = 1; h < N; ++h) s = fma4(w[h], ld4(in.x[h] + o * in.cs[h] + 4 * q), s);
    *reinterpret_cast<float4*>(v + o * v_cs + v_off + 4 * q) = s;   // owned by this lane
  }
}

// ---- reduce: partial[b][block][h][64] = sum over the block's pixels of dV X_h ---------------------------------------------------------------
template <int N>
__global__ __launch_bounds__(256) void reduce_k(const SkIn in, const float* __restrict__ dv, int dv_cs, float* __restrict__ partial, size_t hw) {
  __shared__ float4 sm[256];
  const int tid = threadIdx.x, q = tid & 15, r = tid >> 4, b = blockIdx.y;
  size_t p0, p1;
  block_span(hw, p0, p1);
  float4 acc[N];
#pragma unroll
  for (int h = 0; h < N; ++h) acc[h] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t px = p0 + r; px < p1; px += SK_ROWS) {
    const size_t o = (size_t)b * hw + px;
    const float4 g = ld4(dv + o * dv_cs + 4 * q);
#pragma unroll
    for (int h = 0; h < N; ++h) acc[h] = fma4(g, ld4(in.x[h] + o * in.cs[h] + 4 * q), acc[h]);
  }
  float* dst = partial + ((size_t)b * gridDim.x + blockIdx.x) * (N * CX);
#pragma unroll
  for (int h = 0; h < N; ++h) {
    if (h) __syncthreads();   // row 0 of the previous input has been read
    sm[tid] = acc[h];
    rows_to_row0(sm, tid);
    if (tid < 16) *reinterpret_cast<float4*>(dst + h * CX + 4 * tid) = sm[tid];
  }
}

// ---- gate-reverse: one workgroup per image -> dS[b][64] --------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_bwd_k(const float* __restrict__ partial, int nblk, const float* __restrict__ pack, float slope, int n, int d,
                                                  const float* __restrict__ a, const float* __restrict__ z, float* __restrict__ d_s) {
  __shared__ double s_part[4 * SK_MAXN * CX], s_da[SK_MAXN * CX], s_dA[SK_MAXN * CX], s_dz[SK_MAXD];
  const int tid = threadIdx.x, b = blockIdx.x;
  const SkPack pk = sk_pack(n, d);
  finish_partials(partial + (size_t)b * nblk * n * CX, nblk, n * CX, s_part, s_da, tid);
  if (tid < CX) {
    double dot = 0.0;
    for (int h = 0; h < n; ++h) dot += (double)a[((size_t)b * n + h) * CX + tid] * s_da[h * CX + tid];
    for (int h = 0; h < n; ++h) s_dA[h * CX + tid] = (double)a[((size_t)b * n + h) * CX + tid] * (s_da[h * CX + tid] - dot);
  }
  __syncthreads();
  if (tid < d) {
    double s = 0.0;
    for (int h = 0; h < n; ++h) {
      const float* __restrict__ w = pack + pk.w2 + (size_t)h * CX * d + tid;
      for (int c = 0; c < CX; ++c) s += (double)w[(size_t)c * d] * s_dA[h * CX + c];
    }
    s_dz[tid] = z[(size_t)b * d + tid] > 0.f ? s : (double)slope * s;
  }
  __syncthreads();
  if (tid < CX) {
    double s = 0.0;
    for (int j = 0; j < d; ++j) s += (double)pack[pk.w1 + j * CX + tid] * s_dz[j];
    d_s[(size_t)b * CX + tid] = (float)s;
  }
}

// ---- apply-reverse: dX_h = a_h dV + dS / (H W); an input whose gradient is not wanted has a null pointer --------------------------------------
template <int N>
__global__ __launch_bounds__(256) void apply_bwd_k(const float* __restrict__ dv, int dv_cs, const float* __restrict__ a, const float* __restrict__ d_s,
                                                   float inv_hw, const SkOut out, size_t hw) {
  const int tid = threadIdx.x, q = tid & 15, r = tid >> 4, b = blockIdx.y;
  size_t p0, p1;
  block_span(hw, p0, p1);
  float4 w[N];
#pragma unroll
  for (int h = 0; h < N; ++h) w[h] = ld4(a + ((size_t)b * N + h) * CX + 4 * q);
  float4 s = ld4(d_s + (size_t)b * CX + 4 * q);
  s = make_float4(s.x * inv_hw, s.y * inv_hw, s.z * inv_hw, s.w * inv_hw);
  for (size_t px = p0 + r; px < p1; px += SK_ROWS) {
    const size_t o = (size_t)b * hw + px;
    const float4 g = ld4(dv + o * dv_cs + 4 * q);
#pragma unroll
    for (int h = 0; h < N; ++h)
      if (out.x[h]) *reinterpret_cast<float4*>(out.x[h] + o * CX + 4 * q) = fma4(w[h], g, s);   // owned by this lane
  }
}

// ---- Fusion_Network2's own pack: conv3 and conv4 (operand packs forward and transposed, bias), the head ---------------------------------------
constexpr Plan G_FWD[2] = {plan_for(CX, 64, 1), plan_for(CX, 128, 1)};
constexpr Plan G_BWD[2] = {plan_for(64, CX, 1), plan_for(128, CX, 1)};
constexpr int GUIDE_CIN[2] = {64, 128};
constexpr size_t FK_HEAD_W = 0;                          // [tap 9][ci 64]
constexpr size_t FK_HEAD_B = FK_HEAD_W + 9 * CX;         // [1], padded to 4
constexpr size_t FK_BIAS = FK_HEAD_B + 4;                // conv3 [64], conv4 [64]
constexpr size_t FK_OPS = FK_BIAS + 2 * CX;
constexpr size_t guide_ops(int which, bool transposed) {   // which = 2: the end
  size_t o = FK_OPS;
  for (int i = 0; i < 2; ++i)
    for (int t = 0; t < 2; ++t) {
      if (i == which && t == (int)transposed) return o;
      o += (t ? G_BWD[i] : G_FWD[i]).floats();
    }
  return o;
}
constexpr size_t FK_FLOATS = guide_ops(2, false);
static_assert(FK_BIAS % 4 == 0 && FK_OPS % 4 == 0, "float4 loads from the pack stay aligned");
static_assert(G_FWD[0].MB == 4 && G_FWD[0].groups == 1 && G_FWD[1].MB == 4 && G_FWD[1].groups == 1, "64 output channels in one group");
static_assert(G_BWD[0].MB == 4 && G_BWD[0].groups == 1 && G_BWD[1].MB == 4 && G_BWD[1].groups == 2, "conv4 transposed: two groups of 64");

// the head's weight [1][64][3][3] -> [tap][ci]; a bias as it is
__global__ void pack_head_k(const float* __restrict__ w, float* __restrict__ pw, const float* __restrict__ b, int nb, float* __restrict__ pb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (w && i < 9 * CX) pw[i] = w[(i % CX) * 9 + i / CX];
  if (i < nb) pb[i] = b[i];
}

// ---- conv2: 3 x 3, zero pad 1, 64 -> 1, bias, PReLU -> f.  One pixel per thread; the weights go through the scalar cache; tap ascending,
// channel quad ascending -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head64_fwd_k(const float* __restrict__ hp, float slope, const float* __restrict__ in, float* __restrict__ out,
                                                    int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float s = 0.f;
#pragma unroll 1
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y + tap / 3 - 1, gx = x + tap % 3 - 1;
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const float* __restrict__ src = in + ((size_t)b * hw + (size_t)gy * W + gx) * CX;
    const float* __restrict__ wt = hp + tap * CX;
#pragma unroll
    for (int c = 0; c < CX; c += 4) {
      const float4 v = ld4(src + c);
      s = fmaf(wt[c], v.x, s), s = fmaf(wt[c + 1], v.y, s), s = fmaf(wt[c + 2], v.z, s), s = fmaf(wt[c + 3], v.w, s);
    }
  }
  out[i] = leaky(s + hp[9 * CX], slope);
}
// Reverse: dy = g through the PReLU (branch off the taped f); d_in[p][ci] = sum over tap of W[ci][tap] * dy[p - (tap - centre)].  Sixteen
// lanes per pixel, one channel quad each; WRITES d_in.
__global__ __launch_bounds__(256) void head64_bwd_k(const float* __restrict__ hp, float slope, const float* __restrict__ f, const float* __restrict__ g,
                                                    float* __restrict__ din, int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * 16 + (threadIdx.x >> 4);
  const int cq = threadIdx.x & 15;
  if (i >= n) return;
  const size_t hw = (size_t)H * W;
  const int b = (int)(i / hw), y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) {
    const int gy = y - (tap / 3 - 1), gx = x - (tap % 3 - 1);
    if ((unsigned)gy >= (unsigned)H || (unsigned)gx >= (unsigned)W) continue;
    const size_t o = (size_t)b * hw + (size_t)gy * W + gx;
    const float dy = dleaky(f[o], g[o], slope);
    const float4 wv = ld4(hp + tap * CX + 4 * cq);
    s.x = fmaf(wv.x, dy, s.x), s.y = fmaf(wv.y, dy, s.y), s.z = fmaf(wv.z, dy, s.z), s.w = fmaf(wv.w, dy, s.w);
  }
  *reinterpret_cast<float4*>(din + i * CX + 4 * cq) = s;
}

// ---- the batch min / max normalisation of a plane WITHOUT a clamp (:257-259), forward and reverse.  Block k of nblk owns the elements
// [k span, (k + 1) span), span = ceil(n / nblk).  Reverse, with r = max - min: d_x = d / r, plus at an element equal to the minimum
// (sum d (x - max) / r^2) / #minima, plus at one equal to the maximum (-sum d (x - min) / r^2) / #maxima: torch's even split ---------------
__device__ __forceinline__ void span_of(size_t n, int nblk, size_t& i0, size_t& i1) {
  const size_t span = (n + nblk - 1) / nblk;
  i0 = (size_t)blockIdx.x * span;
  i1 = i0 + span < n ? i0 + span : n;
}

__global__ __launch_bounds__(256) void mm_partial_k(const float* __restrict__ x, float* __restrict__ partial, size_t n) {
  size_t i0, i1;
  span_of(n, gridDim.x, i0, i1);
  float mn = INFINITY, mx = -INFINITY;
  for (size_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float v = x[i];
    mn = fminf(mn, v), mx = fmaxf(mx, v);
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m)), mx = fmaxf(mx, __shfl_xor(mx, m));
  __shared__ float smn[4], smx[4];
  if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = mn, smx[threadIdx.x >> 6] = mx;
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
    partial[gridDim.x + blockIdx.x] = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  }
}

__global__ __launch_bounds__(256) void mm_normalize_k(const float* __restrict__ x, const float* __restrict__ partial, int npartial, float* __restrict__ out,
                                                      float* __restrict__ minmax_out, size_t n) {
  float mn = INFINITY, mx = -INFINITY;
  for (int i = threadIdx.x; i < npartial; i += 256) mn = fminf(mn, partial[i]), mx = fmaxf(mx, partial[npartial + i]);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) mn = fminf(mn, __shfl_xor(mn, m)), mx = fmaxf(mx, __shfl_xor(mx, m));
  __shared__ float smn[4], smx[4];
  if ((threadIdx.x & 63) == 0) smn[threadIdx.x >> 6] = mn, smx[threadIdx.x >> 6] = mx;
  __syncthreads();
  mn = fminf(fminf(smn[0], smn[1]), fminf(smn[2], smn[3]));
  mx = fmaxf(fmaxf(smx[0], smx[1]), fmaxf(smx[2], smx[3]));
  if (blockIdx.x == 0 && threadIdx.x == 0) minmax_out[0] = mn, minmax_out[1] = mx;
  const float range = mx - mn;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) out[i] = __fdiv_rn(__fsub_rn(x[i], mn), range);
}

// partial[block] = (sum d (x - max), sum d (x - min), #(x == min), #(x == max))
__global__ __launch_bounds__(256) void mm_bwd_reduce_k(const float* __restrict__ dout, const float* __restrict__ x, const float* __restrict__ minmax,
                                                       float* __restrict__ partial, size_t n) {
  const float mn = minmax[0], mx = minmax[1];
  size_t i0, i1;
  span_of(n, gridDim.x, i0, i1);
  float a0 = 0.f, a1 = 0.f, c0 = 0.f, c1 = 0.f;
  for (size_t i = i0 + threadIdx.x; i < i1; i += 256) {
    const float v = x[i], d = dout[i];
    a0 = fmaf(d, v - mx, a0), a1 = fmaf(d, v - mn, a1);
    c0 += (v == mn) ? 1.f : 0.f, c1 += (v == mx) ? 1.f : 0.f;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) a0 += __shfl_xor(a0, m), a1 += __shfl_xor(a1, m), c0 += __shfl_xor(c0, m), c1 += __shfl_xor(c1, m);
  __shared__ float4 sm[4];
  if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = make_float4(a0, a1, c0, c1);
  __syncthreads();
  if (threadIdx.x == 0)
    *reinterpret_cast<float4*>(partial + (size_t)blockIdx.x * 4) =
        make_float4((sm[0].x + sm[1].x) + (sm[2].x + sm[3].x), (sm[0].y + sm[1].y) + (sm[2].y + sm[3].y), (sm[0].z + sm[1].z) + (sm[2].z + sm[3].z),
                    (sm[0].w + sm[1].w) + (sm[2].w + sm[3].w));
}

__global__ __launch_bounds__(256) void mm_bwd_apply_k(const float* __restrict__ dout, const float* __restrict__ x, const float* __restrict__ minmax,
                                                      const float* __restrict__ partial, int npartial, float* __restrict__ dx, size_t n) {
  __shared__ float4 tot;
  if (threadIdx.x < 64) {   // the totals in double (the tie counts are exact integers): every workgroup, the same order
    double sx = 0.0, sy = 0.0, cz = 0.0, cw = 0.0;
    for (int i = threadIdx.x; i < npartial; i += 64) {
      const float4 v = ld4(partial + (size_t)i * 4);
      sx += (double)v.x, sy += (double)v.y, cz += (double)v.z, cw += (double)v.w;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sx += __shfl_xor(sx, m), sy += __shfl_xor(sy, m), cz += __shfl_xor(cz, m), cw += __shfl_xor(cw, m);
    if (threadIdx.x == 0) tot = make_float4((float)sx, (float)sy, (float)cz, (float)cw);
  }
  __syncthreads();
  const float mn = minmax[0], mx = minmax[1];
  const float inv = 1.0f / (mx - mn);
  const float d_mn_share = (tot.x * inv * inv) / tot.z;
  const float d_mx_share = (-tot.y * inv * inv) / tot.w;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const float v = x[i];
    float d = dout[i] * inv;
    if (v == mn) d += d_mn_share;
    if (v == mx) d += d_mx_share;
    dx[i] = d;
  }
}

inline int grid1d(size_t n) {
  const size_t g = (n + 255) / 256;
  return (int)(g > 2048 ? 2048 : (g < 1 ? 1 : g));
}
inline int mm_blocks(size_t n) { return (int)((n + 2047) / 2048); }

inline int sk_blocks(int H, int W) { return (int)(((size_t)H * W + SK_PIX - 1) / SK_PIX); }

}  // namespace

#define SKFF_ARGS(name)                                                                                                                  \
  PAIF_REQUIRE(height == 2 || height == 3, PAIF_EINVAL, name ": %d inputs; two or three are built", height);                                            \
  PAIF_REQUIRE(d >= 1 && d <= SK_MAXD, PAIF_EINVAL, name ": d = %d outside [1, %d]", d, SK_MAXD);                                          \
  PAIF_REQUIRE(x0 && x1 && (height == 2 || x2), PAIF_EINVAL, name ": null input");                                                            \
  PAIF_REQUIRE(cs0 >= CX && cs1 >= CX && (height == 2 || cs2 >= CX) && cs0 % 4 == 0 && cs1 % 4 == 0 && (height == 2 || cs2 % 4 == 0), PAIF_EINVAL, \
               name ": an input's pixel stride is a multiple of 4, at least 64");                                                        \
  PAIF_SLAB_SHAPE(name, 1, "", 31);                                                                                                      \
  PAIF_REQUIRE(B <= 65535, PAIF_EINVAL, name ": more than 65535 images");                                                                \
  SkIn in{};                                                                                                                             \
  in.x[0] = x0, in.x[1] = x1, in.x[2] = height == 3 ? x2 : nullptr, in.cs[0] = cs0, in.cs[1] = cs1, in.cs[2] = height == 3 ? cs2 : 0;               \
  const size_t hw = (size_t)H * W;                                                                                                       \
  const int nblk = sk_blocks(H, W);                                                                                                      \
  const dim3 grid((unsigned)nblk, (unsigned)B);                                                                                          \
  const hipStream_t s = paif::as_stream(stream)

extern "C" size_t paif_skff_pack_floats(int height, int d) { return (size_t)sk_pack(height, d).floats; }

extern "C" int paif_skff_blocks(int H, int W) { return sk_blocks(H, W); }

extern "C" int paif_skff_fwd(const float* x0, int cs0, const float* x1, int cs1, const float* x2, int cs2, int height, int d, const float* pack, float slope,
                             float* partial, float* a, float* z, float* v, int v_cs, int v_off, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && partial && a && z && v, PAIF_EINVAL, "skff_fwd: null pointer");
  SKFF_ARGS("skff_fwd");
  PAIF_REQUIRE(v_off >= 0 && v_off % 4 == 0 && v_cs % 4 == 0 && v_cs >= v_off + CX, PAIF_EINVAL, "skff_fwd: V at channels [%d, %d) of %d", v_off,
               v_off + CX, v_cs);
  PAIF_REQUIRE(v != x0 && v != x1 && (height == 2 || v != x2), PAIF_EINVAL, "skff_fwd: V must not be one of the inputs");
  if (height == 2) hipLaunchKernelGGL(pool_k<2>, grid, dim3(256), 0, s, in, partial, hw);
  else hipLaunchKernelGGL(pool_k<3>, grid, dim3(256), 0, s, in, partial, hw);
  PAIF_LAUNCH_CHECK("skff_fwd(pool)");
  hipLaunchKernelGGL(gate_k, dim3((unsigned)B), dim3(256), 0, s, partial, nblk, pack, slope, height, d, 1.0 / (double)hw, a, z);
  PAIF_LAUNCH_CHECK("skff_fwd(gate)");
  if (height == 2) hipLaunchKernelGGL(apply_k<2>, grid, dim3(256), 0, s, in, a, v, v_cs, v_off, hw);
  else hipLaunchKernelGGL(apply_k<3>, grid, dim3(256), 0, s, in, a, v, v_cs, v_off, hw);
  PAIF_LAUNCH_CHECK("skff_fwd(apply)");
  return 0;
}

extern "C" int paif_skff_bwd(const float* x0, int cs0, const float* x1, int cs1, const float* x2, int cs2, int height, int d, const float* pack, float slope,
                             const float* a, const float* z, const float* d_v, int dv_cs, float* partial, float* d_s, float* d_x0, float* d_x1,
                             float* d_x2, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && a && z && d_v && partial && d_s, PAIF_EINVAL, "skff_bwd: null pointer");
  SKFF_ARGS("skff_bwd");
  PAIF_REQUIRE(dv_cs >= CX && dv_cs % 4 == 0, PAIF_EINVAL, "skff_bwd: dV's pixel stride is a multiple of 4, at least 64");
  PAIF_REQUIRE(d_x0 || d_x1 || (height == 3 && d_x2), PAIF_EINVAL, "skff_bwd: no gradient is asked for");
  SkOut out{};
  out.x[0] = d_x0, out.x[1] = d_x1, out.x[2] = height == 3 ? d_x2 : nullptr;
  for (int h = 0; h < height; ++h) PAIF_REQUIRE(out.x[h] != d_v, PAIF_EINVAL, "skff_bwd: a gradient must not be written over dV");
  if (height == 2) hipLaunchKernelGGL(reduce_k<2>, grid, dim3(256), 0, s, in, d_v, dv_cs, partial, hw);
  else hipLaunchKernelGGL(reduce_k<3>, grid, dim3(256), 0, s, in, d_v, dv_cs, partial, hw);
  PAIF_LAUNCH_CHECK("skff_bwd(reduce)");
  hipLaunchKernelGGL(gate_bwd_k, dim3((unsigned)B), dim3(256), 0, s, partial, nblk, pack, slope, height, d, a, z, d_s);
  PAIF_LAUNCH_CHECK("skff_bwd(gate)");
  const float inv_hw = (float)(1.0 / (double)hw);
  if (height == 2) hipLaunchKernelGGL(apply_bwd_k<2>, grid, dim3(256), 0, s, d_v, dv_cs, a, d_s, inv_hw, out, hw);
  else hipLaunchKernelGGL(apply_bwd_k<3>, grid, dim3(256), 0, s, d_v, dv_cs, a, d_s, inv_hw, out, hw);
  PAIF_LAUNCH_CHECK("skff_bwd(apply)");
  return 0;
}

// ---- Fusion_Network2 ---------------------------------------------------------------------------------------------------------------------------
extern "C" size_t paif_fn2_pack_floats(void) { return FK_FLOATS; }

extern "C" int paif_fn2_pack_conv(const float* w, const float* b, int conv, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && pack, PAIF_EINVAL, "fn2_pack_conv: null pointer");
  PAIF_REQUIRE(conv >= 0 && conv <= 2, PAIF_EINVAL, "fn2_pack_conv: conv %d outside [0, 2]", conv);
  const hipStream_t s = paif::as_stream(stream);
  if (conv == 2) {
    hipLaunchKernelGGL(pack_head_k, dim3(3), dim3(256), 0, s, w, pack + FK_HEAD_W, b, 1, pack + FK_HEAD_B);
  } else {
    hipLaunchKernelGGL(pack_head_k, dim3(1), dim3(256), 0, s, (const float*)nullptr, (float*)nullptr, b, CX, pack + FK_BIAS + conv * CX);
    pack_ops(w, CX, GUIDE_CIN[conv], 0, G_FWD[conv], 0, pack + guide_ops(conv, false), s);
    pack_ops(w, CX, GUIDE_CIN[conv], 0, G_BWD[conv], 1, pack + guide_ops(conv, true), s);
  }
  PAIF_LAUNCH_CHECK("fn2_pack_conv");
  return 0;
}

#define FN2_WHICH(name) PAIF_REQUIRE(which == 0 || which == 1, PAIF_EINVAL, name ": which %d is neither 0 (conv3) nor 1 (conv4)", which)

extern "C" int paif_fn2_guide_fwd(const float* pack, int which, const float* in, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && out && in != out, PAIF_EINVAL, "fn2_guide_fwd: null or aliased pointer");
  FN2_WHICH("fn2_guide_fwd");
  PAIF_SLAB_SHAPE("fn2_guide_fwd", 1, "", 31);
  PAIF_SLAB_TILES("fn2_guide_fwd");
  const Plan pl = G_FWD[which];
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = in, a.out = out, a.wpk = pack + guide_ops(which, false), a.bias = pack + FK_BIAS + which * CX, a.slope = 1.f;   // the identity
  a.in_cs = GUIDE_CIN[which], a.nq = GUIDE_CIN[which] / 4;
  a.out_cs = CX, a.out_off = 0, a.out_n = CX;
  hipLaunchKernelGGL((conv_k<1, 4, false, EPI_ACT>), conv_grid(pl, B, tx, ty), dim3(256), 0, paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("fn2_guide_fwd");
  return 0;
}

extern "C" int paif_fn2_guide_bwd(const float* pack, int which, const float* d_out, float* d_in, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && d_out && d_in && d_out != d_in, PAIF_EINVAL, "fn2_guide_bwd: null or aliased pointer");
  FN2_WHICH("fn2_guide_bwd");
  PAIF_SLAB_SHAPE("fn2_guide_bwd", 1, "", 31);
  PAIF_SLAB_TILES("fn2_guide_bwd");
  const Plan pl = G_BWD[which];
  ConvArgs a = conv_args(pl, H, W, tx, ty);
  a.in = d_out, a.out = d_in, a.wpk = pack + guide_ops(which, true);
  a.in_cs = CX, a.nq = CX / 4;
  a.out_cs = GUIDE_CIN[which], a.out_off = 0, a.out_n = GUIDE_CIN[which];
  hipLaunchKernelGGL((conv_k<1, 4, false, EPI_STORE>), conv_grid(pl, B, tx, ty), dim3(256), 0, paif::as_stream(stream), a);
  PAIF_LAUNCH_CHECK("fn2_guide_bwd");
  return 0;
}

#define FN2_SLOPE(name) \
  PAIF_REQUIRE(slope >= 0.f, PAIF_EINVAL, name ": the PReLU slope %g is negative (the branch is read off the taped output)", (double)slope)

extern "C" int paif_fn2_head_fwd(const float* pack, float slope, const float* in, float* f, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(pack && in && f, PAIF_EINVAL, "fn2_head_fwd: null pointer");
  FN2_SLOPE("fn2_head_fwd");
  PAIF_SLAB_SHAPE("fn2_head_fwd", 1, "", 31);
  hipLaunchKernelGGL(head64_fwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), pack + FK_HEAD_W, slope, in, f, H, W, n);
  PAIF_LAUNCH_CHECK("fn2_head_fwd");
  return 0;
}

extern "C" int paif_fn2_head_bwd(const float* pack, float slope, const float* f, const float* d_f, float* d_in, int B, int H, int W,
                                 paif_stream_t stream) {
  PAIF_REQUIRE(pack && f && d_f && d_in, PAIF_EINVAL, "fn2_head_bwd: null pointer");
  FN2_SLOPE("fn2_head_bwd");
  PAIF_SLAB_SHAPE("fn2_head_bwd", 1, "", 31);
  hipLaunchKernelGGL(head64_bwd_k, dim3((unsigned)((n + 15) / 16)), dim3(256), 0, paif::as_stream(stream), pack + FK_HEAD_W, slope, f, d_f, d_in, H, W,
                     n);
  PAIF_LAUNCH_CHECK("fn2_head_bwd");
  return 0;
}

extern "C" int paif_plane_minmax_nc_blocks(size_t n) { return mm_blocks(n); }

extern "C" int paif_plane_minmax_nc_fwd(const float* x, float* out, float* partial, float* minmax_out, size_t n, paif_stream_t stream) {
  PAIF_REQUIRE(x && out && partial && minmax_out && n > 0, PAIF_EINVAL, "plane_minmax_nc_fwd: bad arguments");
  const hipStream_t st = paif::as_stream(stream);
  const int nblk = mm_blocks(n);
  hipLaunchKernelGGL(mm_partial_k, dim3(nblk), dim3(256), 0, st, x, partial, n);
  PAIF_LAUNCH_CHECK("plane_minmax_nc_fwd(partial)");
  hipLaunchKernelGGL(mm_normalize_k, dim3(grid1d(n)), dim3(256), 0, st, x, partial, nblk, out, minmax_out, n);
  PAIF_LAUNCH_CHECK("plane_minmax_nc_fwd(normalize)");
  return 0;
}

extern "C" int paif_plane_minmax_nc_bwd_input(const float* dout, const float* x, const float* minmax, float* partial, float* dx, size_t n,
                                              paif_stream_t stream) {
  PAIF_REQUIRE(dout && x && minmax && partial && dx && n > 0, PAIF_EINVAL, "plane_minmax_nc_bwd_input: bad arguments");
  const hipStream_t st = paif::as_stream(stream);
  const int nblk = mm_blocks(n);
  hipLaunchKernelGGL(mm_bwd_reduce_k, dim3(nblk), dim3(256), 0, st, dout, x, minmax, partial, n);
  PAIF_LAUNCH_CHECK("plane_minmax_nc_bwd_input(reduce)");
  hipLaunchKernelGGL(mm_bwd_apply_k, dim3(grid1d(n)), dim3(256), 0, st, dout, x, minmax, partial, nblk, dx, n);
  PAIF_LAUNCH_CHECK("plane_minmax_nc_bwd_input(apply)");
  return 0;
}
