// ReCoNet baseline (reference fusion_model/Reconet.py): one recurrence of the forward as ONE launch, and its reverse pass (input gradients).
//
// One recurrence reads three 1-channel planes (i_1, i_f, i_2) and writes one; in between sit two sigmoid attention maps, a 3*dim-channel
// GELU map (three dilated 3 -> dim convs) and a 3*dim -> 1 conv + tanh.  The wide map never leaves the registers: the last conv has ONE
// output channel, so each thread reduces over the channels first -- for a pixel q it forms the 3*dim GELU values one after the other and
// at once the nine per-tap sums t[tap][q] = sum_c w_s[c][tap] * f[c][q]; only those nine planes go through LDS, and the output is
// tanh(b + sum_tap t[tap][p + tap]).  fp32 on the vector unit, two pixels per thread as one float2 (v_pk_fma_f32), the weights -- uniform
// over the workgroup -- through the scalar cache.
//
// BORDER RULE.  Every conv of the reference zero-pads its own input, so a halo pixel OUTSIDE the image is zero at all three levels:
// the max / mean planes (max(0,0) = 0 from the zero-filled staging), i_in (0 * att = 0) and -- the one that needs a mask, because
// GELU(bias) != 0 -- the 3*dim map: t[.][q] is forced to zero for q outside the image.  Total halo of one recurrence: 1 + 3 + 1 = 5.
//
// TIE RULE of the reverse pass (what torch's CPU autograd does, pinned by tests/golden/gr_reconet.npz): the channel max of the attention
// input, torch.max(cat([i_a, i_f]), dim=1), sends a tie's WHOLE gradient to index 0 = the image plane i_a (with init_f='max' that is an
// exact tie on about half of the pixels of the first recurrence); the elementwise torch.max(i_1, i_2) of the initialisation splits a tie
// 0.5 / 0.5.
//
// The reverse pass keeps only 1-channel planes on the tape (i_f[k], att_a[k], att_b[k]); the pre-GELU values are recomputed.  It uses the
// same reduce-over-channels-first idea: per pixel q and dilation, u[ch][tap] = sum_c w_d[c][ch][tap] * dz[c][q] in registers, then the 27
// values are added to the LDS planes d_i_in[ch][q + d*tap] tap by tap with a barrier in between -- inside one tap step all targets are
// distinct, so there is no atomic and the summation order is fixed (bit-reproducible).  d_i1 / d_i2 are owned per pixel: no atomics at all.
#include <math.h>

#include "paif_common.h"

namespace {

typedef float v2f __attribute__((ext_vector_type(2)));

// packed weights (paif_reconet_pack_*): [0,9) att_a on max, [9,18) att_a on mean, [18,36) att_b likewise, [36] conv_s bias; then one row
// of PK_ROW floats per (dilation, channel): [0,27) w[ch][ky][kx] (BatchNorm folded), [27] bias (folded), [28,37) w_s[d*dim + c][ky][kx]
constexpr int PK_HDR = 40, PK_ROW = 40;

__device__ __forceinline__ v2f splat(float s) { return v2f{s, s}; }

__device__ __forceinline__ v2f phi_neg_tail2(v2f x) {   // paif::phi_neg_tail on two values
  const v2f t = {fminf(fabsf(x.x), 5.8f), fminf(fabsf(x.y), 5.8f)};
  v2f r = splat(-3.315222873e-08f);
  r = r * t + splat(9.477192170e-07f);
  r = r * t + splat(-1.167834977e-05f);
  r = r * t + splat(7.916988962e-05f);
  r = r * t + splat(-2.841531522e-04f);
  r = r * t + splat(-2.489754232e-07f);
  r = r * t + splat(6.957890404e-03f);
  r = r * t + splat(-5.245515152e-02f);
  r = r * t + splat(-4.592144081e-01f);
  r = r * t + splat(-1.151105125e+00f);
  r = r * t + splat(-1.0f);
  return v2f{__builtin_amdgcn_exp2f(r.x), __builtin_amdgcn_exp2f(r.y)};
}
__device__ __forceinline__ v2f gelu2(v2f x) {
  const v2f e = phi_neg_tail2(x);
  return v2f{x.x * (x.x >= 0.f ? 1.0f - e.x : e.x), x.y * (x.y >= 0.f ? 1.0f - e.y : e.y)};
}
__device__ __forceinline__ v2f gelu_grad2(v2f x) {
  const v2f e = phi_neg_tail2(x);
  const v2f xx = x * x * splat(-0.72134752044448170368f);
  const v2f g = {__builtin_amdgcn_exp2f(xx.x), __builtin_amdgcn_exp2f(xx.y)};
  const v2f phi = {x.x >= 0.f ? 1.0f - e.x : e.x, x.y >= 0.f ? 1.0f - e.y : e.y};
  return phi + x * splat(0.39894228040143267794f) * g;
}
// Pre-GELU value of one channel: the three input channels' nine taps summed separately, the (BatchNorm-folded) bias added LAST.  A folded
// bias (b - mean) * s + beta can be several times larger than the conv sum; started from it, all 27 additions would round at its magnitude
// (measured: the input gradient of the BatchNorm configuration then missed the reference's own fp32 error by 35 %).
__device__ __forceinline__ v2f pre_gelu(const float* __restrict__ wr, const v2f (&x)[27]) {
  v2f s0 = splat(wr[0]) * x[0], s1 = splat(wr[9]) * x[9], s2 = splat(wr[18]) * x[18];
#pragma unroll
  for (int j = 1; j < 9; ++j) {
    s0 += splat(wr[j]) * x[j];
    s1 += splat(wr[9 + j]) * x[9 + j];
    s2 += splat(wr[18 + j]) * x[18 + j];
  }
  return ((s0 + s1) + s2) + splat(wr[27]);
}
__device__ __forceinline__ float sigmoid_exact(float v) { return 1.0f / (1.0f + expf(-v)); }

// ---- weight packing ---------------------------------------------------------------------------------------------------------------
__global__ void pack_group_k(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ gamma, const float* __restrict__ beta,
                             const float* __restrict__ mean, const float* __restrict__ var, float eps, const float* __restrict__ w_s, int dim, int d,
                             float* __restrict__ pack) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= dim) return;
  float s = 1.f, sh = 0.f;
  if (gamma) {   // eval-mode BatchNorm behind the conv: y = (conv + b - mean) * gamma / sqrt(var + eps) + beta
    s = gamma[c] / sqrtf(var[c] + eps);
    sh = beta[c] - mean[c] * s;
  }
  float* row = pack + PK_HDR + (size_t)(d * dim + c) * PK_ROW;
  for (int j = 0; j < 27; ++j) row[j] = w[c * 27 + j] * s;
  row[27] = b[c] * s + sh;
  for (int k = 0; k < 9; ++k) row[28 + k] = w_s[(d * dim + c) * 9 + k];
  row[37] = row[38] = row[39] = 0.f;
}

__global__ void pack_head_k(const float* __restrict__ wa, const float* __restrict__ wb, const float* __restrict__ bs, float* __restrict__ pack) {
  const int i = threadIdx.x;
  if (i < 18) pack[i] = wa[i];
  else if (i < 36) pack[i] = wb[i - 18];
  else if (i == 36) pack[i] = bs[0];
  else if (i < PK_HDR) pack[i] = 0.f;
}

// ---- i_f[0] and its reverse ---------------------------------------------------------------------------------------------------------
__global__ void init_k(const float* __restrict__ i1, size_t sb1, const float* __restrict__ i2, size_t sb2, int use_max, float* __restrict__ out,
                       int HW, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t b = i / HW, r = i - b * HW;
  const float a = i1[b * sb1 + r], c = i2[b * sb2 + r];
  out[i] = use_max ? fmaxf(a, c) : (a + c) / 2.f;
}

// d_i1 += route_1 * g, d_i2 += route_2 * g: torch.max(i_1, i_2) elementwise splits a tie 0.5 / 0.5; the mean is 0.5 / 0.5 everywhere
__global__ void init_bwd_k(const float* __restrict__ i1, size_t sb1, const float* __restrict__ i2, size_t sb2, int use_max, const float* __restrict__ g,
                           float* __restrict__ d_i1, float* __restrict__ d_i2, int HW, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t b = i / HW, r = i - b * HW;
  float r1 = 0.5f;
  if (use_max) {
    const float a = i1[b * sb1 + r], c = i2[b * sb2 + r];
    r1 = a > c ? 1.f : (a == c ? 0.5f : 0.f);
  }
  const float gv = g[i];
  d_i1[i] += r1 * gv;
  d_i2[i] += (1.f - r1) * gv;
}

// ---- one recurrence, forward ------------------------------------------------------------------------------------------------------
constexpr int FT = 30;        // output tile edge: the tile-plus-1 frame is 32 x 32 = 1024 pixels = 256 threads x 2 rounds x 2 pixels
constexpr int FR = FT + 10;   // staged image planes: halo 5
constexpr int FI = FT + 8;    // i_in planes: halo 4
constexpr int FQ = FT + 2;    // per-tap sums: halo 1
static_assert(FQ * FQ == 1024, "the stage-3 pixel mapping assumes a 32 x 32 frame");

__global__ __launch_bounds__(256) void step_fwd_k(const float* __restrict__ i1, size_t sb1, const float* __restrict__ i2, size_t sb2,
                                                  const float* __restrict__ fprev, const float* __restrict__ pack, int dim, float* __restrict__ fnext,
                                                  float* __restrict__ att_a, float* __restrict__ att_b, int H, int W, int tx, int ty) {
  __shared__ float s_t[9 * FQ * FQ];    // the nine per-tap planes; the three staged image planes (3 * FR * FR floats) live here first
  __shared__ float s_in[3 * FI * FI];   // i_in = [i_1 * att_a, i_f, i_2 * att_b]
  static_assert(3 * FR * FR <= 9 * FQ * FQ, "staging must fit under the per-tap planes");
  const int tid = threadIdx.x;
  const int b = blockIdx.x / (tx * ty), rem = blockIdx.x - b * tx * ty, by = rem / tx, bx = rem - by * tx;
  const int y0 = by * FT, x0 = bx * FT;
  const size_t HW = (size_t)H * W;
  const float* p1 = i1 + b * sb1;
  const float* p2 = i2 + b * sb2;
  const float* pf = fprev + b * HW;
  float* raw = s_t;

  // stage 1: the three image planes with halo 5, zero outside the image
  for (int e = tid; e < FR * FR; e += 256) {
    const int ly = e / FR, lx = e - ly * FR, gy = y0 - 5 + ly, gx = x0 - 5 + lx;
    const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    const size_t o = in ? (size_t)gy * W + gx : 0;
    raw[e] = in ? p1[o] : 0.f;
    raw[FR * FR + e] = in ? pf[o] : 0.f;
    raw[2 * FR * FR + e] = in ? p2[o] : 0.f;
  }
  __syncthreads();

  // stage 2: both attention maps and i_in on the tile + halo 4 (Reconet.py:98-105, :82-92).  Outside the image the staged planes are zero,
  // hence so are max / mean there (the attention conv's zero padding) and i_in = 0 * att (the dilated convs' zero padding).
  for (int e = tid; e < FI * FI; e += 256) {
    const int ly = e / FI, lx = e - ly * FI;
    float sa = 0.f, sb = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const int o = (ly + k / 3) * FR + lx + k % 3;
      const float v1 = raw[o], vf = raw[FR * FR + o], v2 = raw[2 * FR * FR + o];
      sa += pack[k] * fmaxf(v1, vf) + pack[9 + k] * ((v1 + vf) / 2.f);
      sb += pack[18 + k] * fmaxf(v2, vf) + pack[27 + k] * ((v2 + vf) / 2.f);
    }
    const float aa = sigmoid_exact(sa), ab = sigmoid_exact(sb);
    const int c = (ly + 1) * FR + lx + 1;
    s_in[e] = raw[c] * aa;
    s_in[FI * FI + e] = raw[FR * FR + c];
    s_in[2 * FI * FI + e] = raw[2 * FR * FR + c] * ab;
    const int y = ly - 4, x = lx - 4, gy = y0 + y, gx = x0 + x;
    if (att_a && (unsigned)y < (unsigned)FT && (unsigned)x < (unsigned)FT && gy < H && gx < W) {
      att_a[b * HW + (size_t)gy * W + gx] = aa;
      att_b[b * HW + (size_t)gy * W + gx] = ab;
    }
  }
  __syncthreads();   // the staged planes are dead from here: s_t is rewritten below

  // stage 3: per pixel of the tile + halo 1, the three dilated convs + GELU channel by channel, reduced at once into the nine per-tap sums
  // of conv_s (Reconet.py:33-52).  Two pixels (16 rows apart) per thread and round.
#pragma unroll 1
  for (int rnd = 0; rnd < 2; ++rnd) {
    const int e0 = tid + 256 * rnd, qy = e0 >> 5, qx = e0 & 31;   // second pixel: (qy + 16, qx)
    v2f t[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) t[k] = splat(0.f);
#pragma unroll 1
    for (int d = 1; d <= 3; ++d) {
      v2f x[27];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int o = ch * FI * FI + (qy + 3 + d * (k / 3 - 1)) * FI + qx + 3 + d * (k % 3 - 1);
          x[ch * 9 + k] = v2f{s_in[o], s_in[o + 16 * FI]};
        }
      const float* __restrict__ wr = pack + PK_HDR + (size_t)(d - 1) * dim * PK_ROW;
      v2f td[9];   // this dilation's share, summed on its own (shorter rounding chains than one sum over 3*dim channels)
#pragma unroll
      for (int k = 0; k < 9; ++k) td[k] = splat(0.f);
#pragma unroll 2
      for (int c = 0; c < dim; ++c, wr += PK_ROW) {
        const v2f z = pre_gelu(wr, x);
        const v2f f = gelu2(z);
#pragma unroll
        for (int k = 0; k < 9; ++k) td[k] += splat(wr[28 + k]) * f;
      }
#pragma unroll
      for (int k = 0; k < 9; ++k) t[k] += td[k];
    }
    // conv_s zero-pads the GELU map: a frame pixel outside the image contributes nothing
    const int gy = y0 - 1 + qy, gx = x0 - 1 + qx;
    const bool inx = (unsigned)gx < (unsigned)W;
    const bool in0 = inx && (unsigned)gy < (unsigned)H, in1 = inx && (unsigned)(gy + 16) < (unsigned)H;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      s_t[k * FQ * FQ + e0] = in0 ? t[k].x : 0.f;
      s_t[k * FQ * FQ + e0 + 512] = in1 ? t[k].y : 0.f;
    }
  }
  __syncthreads();

  // stage 4: conv_s as nine shifted reads, bias, tanh
  const float bs = pack[36];
  for (int e = tid; e < FT * FT; e += 256) {
    const int y = e / FT, x = e - y * FT, gy = y0 + y, gx = x0 + x;
    if (gy >= H || gx >= W) continue;
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) s += s_t[k * FQ * FQ + (y + k / 3) * FQ + x + k % 3];
    fnext[b * HW + (size_t)gy * W + gx] = tanhf(s + bs);
  }
}

// ---- one recurrence, reverse pass ------------------------------------------------------------------------------------------------
constexpr int BT = 32;        // tile edge
constexpr int BI = BT + 12;   // i_in planes: halo 6 (a dz pixel at halo 3 reads i_in 3 further out)
constexpr int BD = BT + 8;    // dy plane: halo 4 (a dz pixel at halo 3 reads dy 1 further out)

// d_fnext -> d(i_in) on the tile; the part of it that does not need neighbours is finished here:
//   d_fprev = d(i_in[1]);  d_i1 (+)= d(i_in[0]) * att_a;  ds_a = d(i_in[0]) * i_1 * att_a * (1 - att_a)  (the attention conv's output gradient)
__global__ __launch_bounds__(256) void step_bwd_k(const float* __restrict__ i1, size_t sb1, const float* __restrict__ i2, size_t sb2,
                                                  const float* __restrict__ fprev, const float* __restrict__ att_a, const float* __restrict__ att_b,
                                                  const float* __restrict__ fnext, const float* __restrict__ g, const float* __restrict__ pack, int dim,
                                                  float* __restrict__ d_i1, float* __restrict__ d_i2, float* __restrict__ d_fprev, float* __restrict__ ds_a,
                                                  float* __restrict__ ds_b, int accumulate, int H, int W, int tx, int ty) {
  __shared__ float s_in[3 * BI * BI];
  __shared__ float s_dy[BD * BD];
  __shared__ float s_acc[3 * BT * BT];
  const int tid = threadIdx.x;
  const int b = blockIdx.x / (tx * ty), rem = blockIdx.x - b * tx * ty, by = rem / tx, bx = rem - by * tx;
  const int y0 = by * BT, x0 = bx * BT;
  const size_t HW = (size_t)H * W;
  const float* p1 = i1 + b * sb1;
  const float* p2 = i2 + b * sb2;
  const size_t pb = b * HW;

  for (int e = tid; e < BI * BI; e += 256) {   // i_in recomposed from the taped planes, zero outside the image
    const int ly = e / BI, lx = e - ly * BI, gy = y0 - 6 + ly, gx = x0 - 6 + lx;
    const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    const size_t o = in ? (size_t)gy * W + gx : 0;
    s_in[e] = in ? p1[o] * att_a[pb + o] : 0.f;
    s_in[BI * BI + e] = in ? fprev[pb + o] : 0.f;
    s_in[2 * BI * BI + e] = in ? p2[o] * att_b[pb + o] : 0.f;
  }
  for (int e = tid; e < BD * BD; e += 256) {   // through the tanh: dy = g * (1 - out)(1 + out), zero outside the image
    const int ly = e / BD, lx = e - ly * BD, gy = y0 - 4 + ly, gx = x0 - 4 + lx;
    const bool in = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
    const size_t o = in ? pb + (size_t)gy * W + gx : 0;
    const float out = in ? fnext[o] : 0.f;
    s_dy[e] = in ? g[o] * ((1.f - out) * (1.f + out)) : 0.f;
  }
  for (int e = tid; e < 3 * BT * BT; e += 256) s_acc[e] = 0.f;
  __syncthreads();

#pragma unroll 1
  for (int d = 1; d <= 3; ++d) {
    const int n = BT + 2 * d;   // the dz frame of this dilation: tile + halo d
#pragma unroll 1
    for (int base = 0; base < n * n; base += 512) {
      int qy[2], qx[2];
      bool ok[2];
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        const int e = base + 256 * p + tid;
        const bool v = e < n * n;
        qy[p] = v ? e / n - d : 0;   // tile coordinates
        qx[p] = v ? e - (e / n) * n - d : 0;
        // the GELU map exists inside the image only (conv_s pads it with zeros, which are no function of anything)
        ok[p] = v && (unsigned)(y0 + qy[p]) < (unsigned)H && (unsigned)(x0 + qx[p]) < (unsigned)W;
      }
      v2f x[27], dyv[9], u[27];
#pragma unroll
      for (int ch = 0; ch < 3; ++ch)
#pragma unroll
        for (int k = 0; k < 9; ++k) {
          const int dy = d * (k / 3 - 1), dx = d * (k % 3 - 1);
          x[ch * 9 + k] = v2f{s_in[ch * BI * BI + (qy[0] + 6 + dy) * BI + qx[0] + 6 + dx], s_in[ch * BI * BI + (qy[1] + 6 + dy) * BI + qx[1] + 6 + dx]};
        }
#pragma unroll
      for (int k = 0; k < 9; ++k) {   // f[q] feeds out[q - tap] through w_s[tap]
        const int dy = 1 - k / 3, dx = 1 - k % 3;
        dyv[k] = v2f{s_dy[(qy[0] + 4 + dy) * BD + qx[0] + 4 + dx], s_dy[(qy[1] + 4 + dy) * BD + qx[1] + 4 + dx]};
      }
#pragma unroll
      for (int j = 0; j < 27; ++j) u[j] = splat(0.f);
      const float* __restrict__ wr = pack + PK_HDR + (size_t)(d - 1) * dim * PK_ROW;
#pragma unroll 1
      for (int c = 0; c < dim; ++c, wr += PK_ROW) {
        const v2f z = pre_gelu(wr, x);
        v2f df = splat(0.f);
#pragma unroll
        for (int k = 0; k < 9; ++k) df += splat(wr[28 + k]) * dyv[k];
        const v2f dz = df * gelu_grad2(z);
#pragma unroll
        for (int j = 0; j < 27; ++j) u[j] += splat(wr[j]) * dz;
      }
      // z[q] read i_in[q + d*tap]: add u[ch][tap] there.  One tap per step: all targets of a step are distinct (fixed summation order).
#pragma unroll
      for (int k = 0; k < 9; ++k) {
        const int dy = d * (k / 3 - 1), dx = d * (k % 3 - 1);
#pragma unroll
        for (int p = 0; p < 2; ++p) {
          const int ry = qy[p] + dy, rx = qx[p] + dx;
          if (ok[p] && (unsigned)ry < (unsigned)BT && (unsigned)rx < (unsigned)BT) {
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) s_acc[ch * BT * BT + ry * BT + rx] += p ? u[ch * 9 + k].y : u[ch * 9 + k].x;
          }
        }
        __syncthreads();
      }
    }
  }

  for (int e = tid; e < BT * BT; e += 256) {
    const int y = e / BT, x = e - y * BT, gy = y0 + y, gx = x0 + x;
    if (gy >= H || gx >= W) continue;
    const size_t r = (size_t)gy * W + gx, o = pb + r;
    const float d0 = s_acc[e], d1 = s_acc[BT * BT + e], d2 = s_acc[2 * BT * BT + e];
    const float aa = att_a[o], ab = att_b[o];
    d_fprev[o] = d1;
    d_i1[o] = (accumulate ? d_i1[o] : 0.f) + d0 * aa;
    d_i2[o] = (accumulate ? d_i2[o] : 0.f) + d2 * ab;
    ds_a[o] = d0 * p1[r] * aa * (1.f - aa);
    ds_b[o] = d2 * p2[r] * ab * (1.f - ab);
  }
}

// Transposed attention convs and the max / mean routing (Reconet.py:98-105).  torch.max(cat([i_a, i_f]), dim=1) on the CPU sends a tie to
// index 0, the image plane: i_a >= i_f takes the whole max-gradient.  Every pixel is owned by one thread.
__global__ __launch_bounds__(256) void att_bwd_k(const float* __restrict__ i1, size_t sb1, const float* __restrict__ i2, size_t sb2,
                                                 const float* __restrict__ fprev, const float* __restrict__ ds_a, const float* __restrict__ ds_b,
                                                 const float* __restrict__ pack, float* __restrict__ d_i1, float* __restrict__ d_i2, float* __restrict__ d_fprev,
                                                 int H, int W, size_t n) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t HW = (size_t)H * W, b = i / HW, r = i - b * HW;
  const int y = (int)(r / W), x = (int)(r - (size_t)y * W);
  float mxa = 0.f, ava = 0.f, mxb = 0.f, avb = 0.f;
#pragma unroll
  for (int k = 0; k < 9; ++k) {   // the output pixel r - tap read this pixel through tap
    const int yy = y - (k / 3 - 1), xx = x - (k % 3 - 1);
    if ((unsigned)yy >= (unsigned)H || (unsigned)xx >= (unsigned)W) continue;
    const size_t o = b * HW + (size_t)yy * W + xx;
    const float sa = ds_a[o], sb = ds_b[o];
    mxa += pack[k] * sa;
    ava += pack[9 + k] * sa;
    mxb += pack[18 + k] * sb;
    avb += pack[27 + k] * sb;
  }
  const float v1 = i1[b * sb1 + r], v2 = i2[b * sb2 + r], vf = fprev[i];
  const bool a1 = v1 >= vf, a2 = v2 >= vf;
  d_i1[i] += (a1 ? mxa : 0.f) + 0.5f * ava;
  d_i2[i] += (a2 ? mxb : 0.f) + 0.5f * avb;
  d_fprev[i] += (a1 ? 0.f : mxa) + (a2 ? 0.f : mxb) + 0.5f * ava + 0.5f * avb;
}

bool dim_ok(int dim) { return dim == 16 || dim == 32 || dim == 64; }

}  // namespace

extern "C" size_t paif_reconet_pack_floats(int dim) { return (size_t)PK_HDR + (size_t)3 * dim * PK_ROW; }

extern "C" int paif_reconet_pack_group(const float* w, const float* b, const float* bn_gamma, const float* bn_beta, const float* bn_mean,
                                       const float* bn_var, float bn_eps, const float* w_s, int dim, int group, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(w && b && w_s && pack, PAIF_EINVAL, "reconet_pack_group: null pointer");
  PAIF_REQUIRE(dim_ok(dim), PAIF_ENOSUP, "reconet_pack_group: dim %d not built (16, 32 and 64 are)", dim);
  PAIF_REQUIRE(group >= 0 && group < 3, PAIF_EINVAL, "reconet_pack_group: group %d outside [0, 3)", group);
  PAIF_REQUIRE(!bn_gamma || (bn_beta && bn_mean && bn_var), PAIF_EINVAL, "reconet_pack_group: BatchNorm needs all four vectors");
  hipLaunchKernelGGL(pack_group_k, dim3(1), dim3(64), 0, paif::as_stream(stream), w, b, bn_gamma, bn_beta, bn_mean, bn_var, bn_eps, w_s, dim, group, pack);
  PAIF_LAUNCH_CHECK("reconet_pack_group");
  return 0;
}

extern "C" int paif_reconet_pack_head(const float* att_a_w, const float* att_b_w, const float* b_s, float* pack, paif_stream_t stream) {
  PAIF_REQUIRE(att_a_w && att_b_w && b_s && pack, PAIF_EINVAL, "reconet_pack_head: null pointer");
  hipLaunchKernelGGL(pack_head_k, dim3(1), dim3(64), 0, paif::as_stream(stream), att_a_w, att_b_w, b_s, pack);
  PAIF_LAUNCH_CHECK("reconet_pack_head");
  return 0;
}

#define RECONET_SHAPE(name)                                                                                        \
  PAIF_REQUIRE(B >= 1 && H >= 1 && W >= 1, PAIF_EINVAL, name ": bad shape %d x %d x %d", B, H, W);                   \
  PAIF_REQUIRE((size_t)H* W <= sb1 && (size_t)H * W <= sb2, PAIF_EINVAL, name ": batch stride smaller than a plane"); \
  PAIF_REQUIRE((size_t)B* H* W < ((size_t)1 << 31), PAIF_EINVAL, name ": more than 2^31 pixels")

extern "C" int paif_reconet_init(const float* i1, size_t sb1, const float* i2, size_t sb2, int use_max, float* out, int B, int H, int W,
                                 paif_stream_t stream) {
  PAIF_REQUIRE(i1 && i2 && out, PAIF_EINVAL, "reconet_init: null pointer");
  RECONET_SHAPE("reconet_init");
  const size_t n = (size_t)B * H * W;
  hipLaunchKernelGGL(init_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), i1, sb1, i2, sb2, use_max, out, H * W, n);
  PAIF_LAUNCH_CHECK("reconet_init");
  return 0;
}

extern "C" int paif_reconet_init_bwd(const float* i1, size_t sb1, const float* i2, size_t sb2, int use_max, const float* d_f0, float* d_i1,
                                     float* d_i2, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(i1 && i2 && d_f0 && d_i1 && d_i2, PAIF_EINVAL, "reconet_init_bwd: null pointer");
  RECONET_SHAPE("reconet_init_bwd");
  const size_t n = (size_t)B * H * W;
  hipLaunchKernelGGL(init_bwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), i1, sb1, i2, sb2, use_max, d_f0, d_i1, d_i2,
                     H * W, n);
  PAIF_LAUNCH_CHECK("reconet_init_bwd");
  return 0;
}

extern "C" int paif_reconet_step_fwd(const float* i1, size_t sb1, const float* i2, size_t sb2, const float* f_prev, const float* pack, int dim,
                                     float* f_next, float* att_a, float* att_b, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(i1 && i2 && f_prev && pack && f_next, PAIF_EINVAL, "reconet_step_fwd: null pointer");
  PAIF_REQUIRE((att_a == nullptr) == (att_b == nullptr), PAIF_EINVAL, "reconet_step_fwd: att_a and att_b go together");
  PAIF_REQUIRE(f_prev != f_next, PAIF_EINVAL, "reconet_step_fwd: in-place recurrence (tiles read their neighbours' f_prev)");
  PAIF_REQUIRE(dim_ok(dim), PAIF_ENOSUP, "reconet_step_fwd: dim %d not built (16, 32 and 64 are)", dim);
  RECONET_SHAPE("reconet_step_fwd");
  const int tx = (W + FT - 1) / FT, ty = (H + FT - 1) / FT;
  PAIF_REQUIRE((size_t)tx * ty * B < ((size_t)1 << 31), PAIF_EINVAL, "reconet_step_fwd: too many tiles");
  hipLaunchKernelGGL(step_fwd_k, dim3((unsigned)(tx * ty * B)), dim3(256), 0, paif::as_stream(stream), i1, sb1, i2, sb2, f_prev, pack, dim, f_next, att_a,
                     att_b, H, W, tx, ty);
  PAIF_LAUNCH_CHECK("reconet_step_fwd");
  return 0;
}

extern "C" int paif_reconet_step_bwd(const float* i1, size_t sb1, const float* i2, size_t sb2, const float* f_prev, const float* att_a,
                                     const float* att_b, const float* f_next, const float* d_f_next, const float* pack, int dim, float* d_i1,
                                     float* d_i2, float* d_f_prev, float* workspace, int accumulate, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(i1 && i2 && f_prev && att_a && att_b && f_next && d_f_next && pack && d_i1 && d_i2 && d_f_prev && workspace, PAIF_EINVAL,
               "reconet_step_bwd: null pointer");
  PAIF_REQUIRE(d_f_prev != d_f_next, PAIF_EINVAL, "reconet_step_bwd: d_f_prev must not alias d_f_next (tiles read their neighbours' d_f_next)");
  PAIF_REQUIRE(dim_ok(dim), PAIF_ENOSUP, "reconet_step_bwd: dim %d not built (16, 32 and 64 are)", dim);
  RECONET_SHAPE("reconet_step_bwd");
  const int tx = (W + BT - 1) / BT, ty = (H + BT - 1) / BT;
  const size_t n = (size_t)B * H * W;
  float* ds_a = workspace;
  float* ds_b = workspace + n;
  hipLaunchKernelGGL(step_bwd_k, dim3((unsigned)(tx * ty * B)), dim3(256), 0, paif::as_stream(stream), i1, sb1, i2, sb2, f_prev, att_a, att_b, f_next,
                     d_f_next, pack, dim, d_i1, d_i2, d_f_prev, ds_a, ds_b, accumulate, H, W, tx, ty);
  PAIF_LAUNCH_CHECK("reconet_step_bwd");
  hipLaunchKernelGGL(att_bwd_k, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, paif::as_stream(stream), i1, sb1, i2, sb2, f_prev, ds_a, ds_b, pack, d_i1,
                     d_i2, d_f_prev, H, W, n);
  PAIF_LAUNCH_CHECK("reconet_step_bwd(attention)");
  return 0;
}
