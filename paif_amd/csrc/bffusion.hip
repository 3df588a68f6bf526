// BFFusion baseline (reference fusion_model/BFFusion.py, class BFFR).  Two encoder streams of four resolutions (a 1 x 1 stem, per level a
// DenseBlock over a concat slab, 2 x 2 max-pooling between levels), per level two channel-attention blocks (one per stream) whose mean is the
// fused map, a UNet++ decoder of six reflection-padded 3 x 3 convs over concats of fused maps and nearest-upsampled maps, a 1 x 1 head with
// tanh / 2 + 0.5.  The module (paif_amd/fusion_model/bffusion.py) holds the table of layers; this file holds the launches it is made of.
//
// LAYOUT.  fp32 NHWC.  Every concat a conv reads exists once, as a channel range of a slab (ops.bffusion_forward lists the slabs); a conv
// stores its output into the slab of its consumer.  A launch stores to channels it does not read, except the three that ADD into the
// element they own (the EPI_ADD epilogue of conv_slab.h, fold_k beyond n_store, pool_bwd_k, up_bwd_k with add).
//
// MATRIX CORE (conv_slab.h): every 3 x 3 and 1 x 1 conv with >= 16 input channels and its transpose, BatchNorm folded into the operand
// pack.  REFLECTION: forward by reflected staging (REFL_STAGE); the transpose is the zero-pad transposed conv on the (H + 2) x (W + 2) grid
// (REFL_RING, a ring map) and then fold_k: ring row -1 adds into row 1, row H into row H - 2, the same for columns, corners twice.
//
// VECTOR UNIT: stem, head, pool, upsample (+ fringe), gate / mean, LayerNorm, the attention's context reduction and its application,
// each forward and reverse.  The CONTEXT REDUCTION over the N = H W pixels of one image is two-stage: ctx_partial_k sums chunks of
// CTX_CHUNK pixels (the partition depends on N alone; inside a chunk G groups of lanes take every G-th pixel and are added in group order),
// ctx_softmax_k / ctx_softmax_bwd_k add the chunks in chunk order.  Both stages accumulate in float64.
// No atomics, no host synchronisation, every output element is summed by one lane in a fixed order: bit-reproducible and capturable.
#include <math.h>
#include <stdint.h>

#include "conv_slab.h"

namespace {

using namespace paif_slab;

constexpr int CTX_CHUNK = 1024;   // pixels per block of the context reduction
constexpr int MAX_D = 8;          // head dim

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ float4 add4(float4 a, float4 b) { return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w); }

// ---- stem: 1 x 1, 1 -> 16, bias, no activation, into channels [0, 16) of a slab.  One lane per pixel and channel quad ---------------------
__global__ __launch_bounds__(256) void stem_fwd_k(const float* __restrict__ x, size_t sb, const float* __restrict__ w, const float* __restrict__ bias,
                                                  float* __restrict__ out, int out_cs, size_t hw, size_t n) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t >> 2;
  const int c = 4 * (int)(t & 3);
  if (i >= n) return;
  const size_t b = i / hw;
  const float v = x[b * sb + (i - b * hw)];
  const float4 wv = ld4(w + c), bv = ld4(bias + c);
  st4(out + i * out_cs + c, make_float4(fmaf(wv.x, v, bv.x), fmaf(wv.y, v, bv.y), fmaf(wv.z, v, bv.z), fmaf(wv.w, v, bv.w)));
}
// Reverse: d_x = sum over the 16 channels of w[c] d[c], c ascending
__global__ __launch_bounds__(256) void stem_bwd_k(const float* __restrict__ w, const float* __restrict__ d, int d_cs, float* __restrict__ dx, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 16; c += 4) {
    const float4 wv = ld4(w + c), g = ld4(d + i * d_cs + c);
    s = fmaf(wv.x, g.x, s), s = fmaf(wv.y, g.y, s), s = fmaf(wv.z, g.z, s), s = fmaf(wv.w, g.w, s);
  }
  dx[i] = s;
}

// ---- head: 1 x 1, 16 -> 1, bias, tanh / 2 + 0.5 -------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void head_fwd_k(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ in, int in_cs,
                                                  float* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float s = bias[0];
#pragma unroll
  for (int c = 0; c < 16; c += 4) {
    const float4 wv = ld4(w + c), v = ld4(in + i * in_cs + c);
    s = fmaf(wv.x, v.x, s), s = fmaf(wv.y, v.y, s), s = fmaf(wv.z, v.z, s), s = fmaf(wv.w, v.w, s);
  }
  out[i] = 0.5f * tanhf(s) + 0.5f;
}
// Reverse, off the taped plane f: t = 2 f - 1, dz = g (1 - t^2) / 2; d[c] = w[c] dz
__global__ __launch_bounds__(256) void head_bwd_k(const float* __restrict__ w, const float* __restrict__ f, const float* __restrict__ g,
                                                  float* __restrict__ d, int d_cs, size_t n) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t >> 2;
  const int c = 4 * (int)(t & 3);
  if (i >= n) return;
  const float th = 2.f * f[i] - 1.f, dz = 0.5f * g[i] * ((1.f - th) * (1.f + th));
  const float4 wv = ld4(w + c);
  st4(d + i * d_cs + c, make_float4(wv.x * dz, wv.y * dz, wv.z * dz, wv.w * dz));
}

// ---- 2 x 2 max-pooling, stride 2; an odd last row or column is dropped.  One lane per pooled pixel and channel quad -------------------------
__device__ __forceinline__ void first_max(float v, int k, float& m, int& at) {   // torch: a later element wins only if it is greater (or NaN)
  if (v > m || v != v) m = v, at = k;
}
__global__ __launch_bounds__(256) void pool_fwd_k(const float* __restrict__ in, int in_cs, int C, int Hs, int Ws, float* __restrict__ out, int out_cs,
                                                  int Hp, int Wp, size_t n) {
  const int cq = C / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / cq;
  const int c = 4 * (int)(t - i * cq);
  if (i >= n) return;
  const size_t hw = (size_t)Hp * Wp, b = i / hw;
  const int y = (int)((i - b * hw) / Wp), x = (int)(i - b * hw - (size_t)y * Wp);
  const float* __restrict__ s = in + ((b * Hs + 2 * y) * Ws + 2 * x) * in_cs + c;
  const float4 a = ld4(s), e = ld4(s + in_cs), f = ld4(s + (size_t)Ws * in_cs), g = ld4(s + (size_t)(Ws + 1) * in_cs);
  st4(out + i * out_cs + c, make_float4(fmaxf(fmaxf(a.x, e.x), fmaxf(f.x, g.x)), fmaxf(fmaxf(a.y, e.y), fmaxf(f.y, g.y)),
                                        fmaxf(fmaxf(a.z, e.z), fmaxf(f.z, g.z)), fmaxf(fmaxf(a.w, e.w), fmaxf(f.w, g.w))));
}
// Reverse, one lane per SOURCE pixel and channel: the window's choice is read off the taped pre-pool map (the first maximum in row-major
// window order); the chosen element ADDS the pooled gradient to its own element of d_in, every other one (and the dropped fringe) adds nothing.
__global__ __launch_bounds__(256) void pool_bwd_k(const float* __restrict__ in, int in_cs, int C, int Hs, int Ws, const float* __restrict__ dp,
                                                  int dp_cs, int Hp, int Wp, float* __restrict__ din, int din_cs, size_t n) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / C;
  const int c = (int)(t - i * C);
  if (i >= n) return;
  const size_t hw = (size_t)Hs * Ws, b = i / hw;
  const int y = (int)((i - b * hw) / Ws), x = (int)(i - b * hw - (size_t)y * Ws);
  const int py = y >> 1, px = x >> 1;
  if (py >= Hp || px >= Wp) return;
  const float* __restrict__ s = in + ((b * Hs + 2 * py) * Ws + 2 * px) * in_cs + c;
  float m = s[0];
  int at = 0;
  first_max(s[in_cs], 1, m, at);
  first_max(s[(size_t)Ws * in_cs], 2, m, at);
  first_max(s[(size_t)(Ws + 1) * in_cs], 3, m, at);
  if (at == 2 * (y & 1) + (x & 1)) din[i * din_cs + c] += dp[((b * Hp + py) * Wp + px) * dp_cs + c];
}

// ---- nearest x 2 plus the reflected fringe: dst (y, x) = src (min(y >> 1, Hs - 1), min(x >> 1, Ws - 1)) -- row 2 Hs reflects to row 2 Hs - 2 ----
__global__ __launch_bounds__(256) void up_fwd_k(const float* __restrict__ src, int src_cs, int C, int Hs, int Ws, float* __restrict__ dst, int dst_cs,
                                                int Hd, int Wd, size_t n) {
  const int cq = C / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / cq;
  const int c = 4 * (int)(t - i * cq);
  if (i >= n) return;
  const size_t hw = (size_t)Hd * Wd, b = i / hw;
  const int y = (int)((i - b * hw) / Wd), x = (int)(i - b * hw - (size_t)y * Wd);
  const int sy = min(y >> 1, Hs - 1), sx = min(x >> 1, Ws - 1);
  st4(dst + i * dst_cs + c, ld4(src + ((b * Hs + sy) * Ws + sx) * src_cs + c));
}
// Reverse, one lane per source pixel and channel quad: the 4 (6, 9 at the fringe) readers, rows then columns ascending
template <bool ADD>
__global__ __launch_bounds__(256) void up_bwd_k(const float* __restrict__ dd, int dd_cs, int C, int Hd, int Wd, float* __restrict__ ds, int ds_cs,
                                                int Hs, int Ws, size_t n) {
  const int cq = C / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / cq;
  const int c = 4 * (int)(t - i * cq);
  if (i >= n) return;
  const size_t hw = (size_t)Hs * Ws, b = i / hw;
  const int y = (int)((i - b * hw) / Ws), x = (int)(i - b * hw - (size_t)y * Ws);
  const int y1 = (y == Hs - 1) ? Hd : 2 * y + 2, x1 = (x == Ws - 1) ? Wd : 2 * x + 2;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int yy = 2 * y; yy < y1; ++yy)
    for (int xx = 2 * x; xx < x1; ++xx) s = add4(s, ld4(dd + ((b * Hd + yy) * Wd + xx) * dd_cs + c));
  float* o = ds + i * ds_cs + c;
  if constexpr (ADD) s = add4(ld4(o), s);
  st4(o, s);
}

// ---- the gate skip + skip x of both attention blocks and their mean ------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gate_fwd_k(const float* __restrict__ sa, int sa_cs, const float* __restrict__ xa, const float* __restrict__ sb,
                                                  int sb_cs, const float* __restrict__ xb, int C, float* __restrict__ out, int out_cs, size_t n) {
  const int cq = C / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / cq;
  const int c = 4 * (int)(t - i * cq);
  if (i >= n) return;
  const float4 a = ld4(sa + i * sa_cs + c), u = ld4(xa + i * C + c), e = ld4(sb + i * sb_cs + c), v = ld4(xb + i * C + c);
  st4(out + i * out_cs + c, make_float4(0.5f * (fmaf(a.x, u.x, a.x) + fmaf(e.x, v.x, e.x)), 0.5f * (fmaf(a.y, u.y, a.y) + fmaf(e.y, v.y, e.y)),
                                        0.5f * (fmaf(a.z, u.z, a.z) + fmaf(e.z, v.z, e.z)), 0.5f * (fmaf(a.w, u.w, a.w) + fmaf(e.w, v.w, e.w))));
}
// Reverse of one block: h = 0.5 d_fused; d_x = skip h (the cotangent of the last ffn map); d_skip = h + h x (STORED: the first writer of d_skip)
__global__ __launch_bounds__(256) void gate_bwd_k(const float* __restrict__ df, int df_cs, const float* __restrict__ skip, int skip_cs,
                                                  const float* __restrict__ x, int C, float* __restrict__ dx, float* __restrict__ dskip, size_t n) {
  const int cq = C / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / cq;
  const int c = 4 * (int)(t - i * cq);
  if (i >= n) return;
  const float4 g = ld4(df + i * df_cs + c), s = ld4(skip + i * skip_cs + c), u = ld4(x + i * C + c);
  const float4 h = make_float4(0.5f * g.x, 0.5f * g.y, 0.5f * g.z, 0.5f * g.w);
  st4(dx + i * C + c, make_float4(s.x * h.x, s.y * h.y, s.z * h.z, s.w * h.w));
  st4(dskip + i * C + c, make_float4(fmaf(h.x, u.x, h.x), fmaf(h.y, u.y, h.y), fmaf(h.z, u.z, h.z), fmaf(h.w, u.w, h.w)));
}

// ---- LayerNorm over the C channels of a pixel (biased variance), one lane per pixel, channels ascending -------------------------------------
__global__ __launch_bounds__(256) void ln_fwd_k(const float* __restrict__ y, const float* __restrict__ gamma, const float* __restrict__ beta, float eps,
                                                int C, float* __restrict__ z, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ r = y + i * C;
  float m = 0.f;
  for (int c = 0; c < C; ++c) m += r[c];
  m /= (float)C;
  float v = 0.f;
  for (int c = 0; c < C; ++c) v = fmaf(r[c] - m, r[c] - m, v);
  const float rs = rsqrtf(v / (float)C + eps);
  for (int c = 0; c < C; ++c) z[i * C + c] = fmaf((r[c] - m) * rs, gamma[c], beta[c]);
}
// Reverse off the taped INPUT y: xh = (y - m) rs, g = dz gamma, dy = rs (g - mean(g) - xh mean(g xh))
__global__ __launch_bounds__(256) void ln_bwd_k(const float* __restrict__ y, const float* __restrict__ gamma, float eps, int C,
                                                const float* __restrict__ dz, float* __restrict__ dy, size_t n) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* __restrict__ r = y + i * C;
  const float* __restrict__ d = dz + i * C;
  float m = 0.f;
  for (int c = 0; c < C; ++c) m += r[c];
  m /= (float)C;
  float v = 0.f;
  for (int c = 0; c < C; ++c) v = fmaf(r[c] - m, r[c] - m, v);
  const float rs = rsqrtf(v / (float)C + eps);
  float sg = 0.f, sgx = 0.f;
  for (int c = 0; c < C; ++c) {
    const float g = d[c] * gamma[c];
    sg += g, sgx = fmaf(g, (r[c] - m) * rs, sgx);
  }
  sg /= (float)C, sgx /= (float)C;
  for (int c = 0; c < C; ++c) dy[i * C + c] = rs * (d[c] * gamma[c] - sg - (r[c] - m) * rs * sgx);
}

// ---- the context reduction, stage 1: partial[b][chunk][c d + j] = sum over the chunk's pixels n of a[n][c] b[n][(c / d) d + j] ---------------
// E = dim d elements.  E < 256: G = 256 / E groups of E lanes, group g takes the pixels n0 + g, n0 + g + G, ...; the groups are added in
// group order through LDS.  E >= 256: every lane takes its elements e, e + 256, ... over all pixels of the chunk.
__global__ __launch_bounds__(256) void ctx_partial_k(const float* __restrict__ a, int a_cs, const float* __restrict__ bm, int b_cs, int dim, int d,
                                                     int N, int chunks, double* __restrict__ partial) {
  __shared__ double sh[256];
  const int tid = threadIdx.x, E = dim * d, G = E >= 256 ? 1 : 256 / E;
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int n0 = chunk * CTX_CHUNK, n1 = min(N, n0 + CTX_CHUNK);
  const float* __restrict__ pa = a + (size_t)b * N * a_cs;
  const float* __restrict__ pb = bm + (size_t)b * N * b_cs;
  double* __restrict__ dst = partial + ((size_t)b * chunks + chunk) * E;
  for (int e0 = 0; e0 < E; e0 += 256) {   // more than one round only where G = 1
    const int g = G == 1 ? 0 : tid / E, e = G == 1 ? e0 + tid : tid - g * E;
    const bool active = G == 1 ? e < E : g < G;
    double s = 0.0;
    if (active) {
      const int c = e / d, cb = (c / d) * d + (e - c * d);
      for (int n = n0 + g; n < n1; n += G) s = fma((double)pa[(size_t)n * a_cs + c], (double)pb[(size_t)n * b_cs + cb], s);
    }
    if (G == 1) {
      if (active) dst[e] = s;
    } else {
      sh[tid] = s;
      __syncthreads();
      if (tid < E) {
        double t = sh[tid];
        for (int k = 1; k < G; ++k) t += sh[k * E + tid];
        dst[tid] = t;
      }
    }
  }
}
// Stage 2, one lane per image and column (h, j): the chunks in order, times scale, softmax over i -> ctx[b][(h d + i) d + j]
__global__ __launch_bounds__(256) void ctx_softmax_k(const double* __restrict__ partial, int chunks, int dim, int d, float scale, float* __restrict__ ctx,
                                                     int n) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int b = t / dim, col = t - b * dim, h = col / d, j = col - h * d, E = dim * d;
  float l[MAX_D];
  float m = -INFINITY;
  for (int i = 0; i < d; ++i) {
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += partial[((size_t)b * chunks + k) * E + (h * d + i) * d + j];
    l[i] = (float)s * scale;
    m = fmaxf(m, l[i]);
  }
  float z = 0.f;
  for (int i = 0; i < d; ++i) l[i] = expf(l[i] - m), z += l[i];
  for (int i = 0; i < d; ++i) ctx[(size_t)b * E + (h * d + i) * d + j] = l[i] / z;
}
// Reverse: d_ctx from the chunks; dS[i][j] = scale ctx[i][j] (d_ctx[i][j] - sum over i' of ctx[i'][j] d_ctx[i'][j]) -- the cotangent of q^T k
__global__ __launch_bounds__(256) void ctx_softmax_bwd_k(const double* __restrict__ partial, int chunks, int dim, int d, float scale,
                                                         const float* __restrict__ ctx, float* __restrict__ dS, int n) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const int b = t / dim, col = t - b * dim, h = col / d, j = col - h * d, E = dim * d;
  float g[MAX_D];
  float dot = 0.f;
  for (int i = 0; i < d; ++i) {
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += partial[((size_t)b * chunks + k) * E + (h * d + i) * d + j];
    g[i] = (float)s;
    dot = fmaf(ctx[(size_t)b * E + (h * d + i) * d + j], g[i], dot);
  }
  for (int i = 0; i < d; ++i) {
    const size_t o = (size_t)b * E + (h * d + i) * d + j;
    dS[o] = scale * ctx[o] * (g[i] - dot);
  }
}
// x[n][h d + j] = sum over i of v[n][h d + i] ctx[(h d + i) d + j]; v = channels [2 dim, 3 dim) of qkv.  One lane per pixel and channel
__global__ __launch_bounds__(256) void attn_apply_fwd_k(const float* __restrict__ qkv, const float* __restrict__ ctx, int dim, int d, int N,
                                                        float* __restrict__ x, size_t n) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / dim;
  const int c = (int)(t - i * dim);
  if (i >= n) return;
  const int h = c / d, j = c - h * d;
  const float* __restrict__ v = qkv + i * 3 * dim + 2 * dim + h * d;
  const float* __restrict__ m = ctx + (i / N) * (size_t)(dim * d) + (size_t)h * d * d + j;
  float s = 0.f;
  for (int k = 0; k < d; ++k) s = fmaf(v[k], m[k * d], s);
  x[t] = s;
}
// Reverse: d_q[n][h d + i] = sum_j dS[i][j] k[n][h d + j]; d_k[n][h d + j] = sum_i dS[i][j] q[n][h d + i]; d_v[n][h d + i] = sum_j d_x[n][h d + j] ctx[i][j]
__global__ __launch_bounds__(256) void attn_apply_bwd_k(const float* __restrict__ qkv, const float* __restrict__ dx, const float* __restrict__ ctx,
                                                        const float* __restrict__ dS, int dim, int d, int N, float* __restrict__ dqkv, size_t n) {
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / dim;
  const int c = (int)(t - i * dim);
  if (i >= n) return;
  const int h = c / d, r = c - h * d;
  const size_t mo = (i / N) * (size_t)(dim * d) + (size_t)h * d * d;
  const float* __restrict__ q = qkv + i * 3 * dim + h * d;
  const float* __restrict__ k = q + dim;
  const float* __restrict__ g = dx + i * dim + h * d;
  float sq = 0.f, sk = 0.f, sv = 0.f;
  for (int e = 0; e < d; ++e) {
    sq = fmaf(dS[mo + r * d + e], k[e], sq);
    sk = fmaf(dS[mo + e * d + r], q[e], sk);
    sv = fmaf(g[e], ctx[mo + r * d + e], sv);
  }
  float* o = dqkv + i * 3 * dim + c;
  o[0] = sq, o[dim] = sk, o[2 * dim] = sv;
}

// ---- the fold of a reflected conv's transpose: ring [B][H + 2][W + 2][M] -> the plane.  Pixel (y, x) sums ring (y + 1, x + 1), and where it
// is row 1 the ring's row 0, where it is row H - 2 the ring's row H + 1, the same for columns: rows then columns in that order.  Channels
// below n_store are STORED, the others ADDED to the element the lane owns.  One lane per pixel and channel quad.
__global__ __launch_bounds__(256) void fold_k(const float* __restrict__ ring, int M, int n_store, float* __restrict__ dst, int dst_cs, int H, int W,
                                              size_t n) {
  const int cq = M / 4;
  const size_t t = (size_t)blockIdx.x * 256 + threadIdx.x, i = t / cq;
  const int c = 4 * (int)(t - i * cq);
  if (i >= n) return;
  const size_t hw = (size_t)H * W, b = i / hw;
  const int y = (int)((i - b * hw) / W), x = (int)(i - b * hw - (size_t)y * W);
  int ry[3], rx[3], ny = 0, nx = 0;
  ry[ny++] = y + 1;
  if (y == 1) ry[ny++] = 0;
  if (y == H - 2) ry[ny++] = H + 1;
  rx[nx++] = x + 1;
  if (x == 1) rx[nx++] = 0;
  if (x == W - 2) rx[nx++] = W + 1;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int a = 0; a < ny; ++a)
    for (int e = 0; e < nx; ++e) s = add4(s, ld4(ring + ((b * (H + 2) + ry[a]) * (W + 2) + rx[e]) * M + c));
  float* o = dst + i * dst_cs + c;
  if (c >= n_store) s = add4(ld4(o), s);
  st4(o, s);
}

inline unsigned blocks(size_t threads) { return (unsigned)((threads + 255) / 256); }

}  // namespace

#define BFF_CH(name, C, cs) \
  PAIF_REQUIRE((C) >= 4 && (C) % 4 == 0 && (cs) >= (C) && (cs) % 4 == 0, PAIF_EINVAL, name ": %d channels at stride %d", (int)(C), (int)(cs))

extern "C" size_t paif_bffusion_ops_floats(int M, int K, int taps) {
  if (M < 1 || K < 1 || (taps != 1 && taps != 9)) return 0;
  return plan_for(M, K, taps).floats();
}

extern "C" int paif_bffusion_pack_ops(const float* w, int co, int n, int off, int M, int K, int taps, int transposed, float* dst, paif_stream_t stream) {
  PAIF_REQUIRE(w && dst, PAIF_EINVAL, "bffusion_pack_ops: null pointer");
  PAIF_REQUIRE((taps == 1 || taps == 9) && co >= 1 && n >= 1 && off >= 0 && M >= 1 && K >= 1, PAIF_EINVAL, "bffusion_pack_ops: bad arguments");
  PAIF_REQUIRE(transposed ? (co <= K && off + n <= M) : (co <= M && off + n <= K), PAIF_EINVAL,
               "bffusion_pack_ops: a [%d][%d] weight at offset %d does not fit M = %d, K = %d", co, n, off, M, K);
  const Plan pl = plan_for(M, K, taps);
  hipLaunchKernelGGL(pack_ops_k, dim3(blocks(pl.floats())), dim3(256), 0, paif::as_stream(stream), w, co, n, off, pl, transposed, dst);
  PAIF_LAUNCH_CHECK("bffusion_pack_ops");
  return 0;
}

extern "C" int paif_bffusion_conv(const float* wpk, const float* bias, float slope, int epi, int taps, int refl, const float* in, const float* mask,
                                  int in_cs, int K, float* out, int out_cs, int M, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(wpk && in && out, PAIF_EINVAL, "bffusion_conv: null pointer");
  PAIF_REQUIRE(K >= 16 && K % 16 == 0 && in_cs >= K && in_cs % 4 == 0 && M >= 16 && M % 16 == 0 && out_cs >= M && out_cs % 4 == 0, PAIF_EINVAL,
               "bffusion_conv: K = %d at stride %d, M = %d at stride %d", K, in_cs, M, out_cs);
  PAIF_REQUIRE((epi == EPI_ACT) == (bias != nullptr), PAIF_EINVAL, "bffusion_conv: the activation epilogue, and only it, takes a bias");
  PAIF_SLAB_SHAPE("bffusion_conv", 1, "", 26);
  PAIF_REQUIRE(refl == REFL_NONE || (H >= 2 && W >= 2), PAIF_EINVAL, "bffusion_conv: reflection padding needs H, W >= 2");
  const int ring = refl == REFL_RING ? 2 : 0;
  const int tx = (W + ring + DT - 1) / DT, ty = (H + ring + DT - 1) / DT;
  const Plan pl = plan_for(M, K, taps);
  ConvArgs a;
  a.in = in, a.mask = mask, a.out = out, a.wpk = wpk, a.bias = bias, a.bias2 = nullptr, a.slope = slope;
  a.in_cs = in_cs, a.nq = K / 4, a.out_cs = out_cs, a.out_off = 0, a.out_n = M, a.chunks = pl.chunks, a.H = H, a.W = W, a.tx = tx, a.ty = ty;
  const dim3 grid((unsigned)(tx * ty * B), (unsigned)pl.groups);
  const hipStream_t s = paif::as_stream(stream);
  const bool m = mask != nullptr;
  // the forms the network is made of
  if (taps == 9 && refl == REFL_NONE && !m && epi == EPI_ACT) launch_conv<9, false, EPI_ACT>(pl.MB, grid, s, a);            // DenseBlock 3 x 3
  else if (taps == 9 && refl == REFL_STAGE && !m && epi == EPI_ACT) launch_conv_r<false, EPI_ACT, REFL_STAGE>(pl.MB, grid, s, a);   // f_ConvLayer, ConvLayer
  else if (taps == 1 && refl == REFL_NONE && !m && epi == EPI_ACT) launch_conv<1, false, EPI_ACT>(pl.MB, grid, s, a);       // conv_down, end_proj1
  else if (taps == 1 && refl == REFL_NONE && !m && epi == EPI_STORE) launch_conv<1, false, EPI_STORE>(pl.MB, grid, s, a);   // q | k | v, and transposes
  else if (taps == 1 && refl == REFL_NONE && m && epi == EPI_STORE) launch_conv<1, true, EPI_STORE>(pl.MB, grid, s, a);     // conv_down'
  else if (taps == 9 && refl == REFL_NONE && m && epi == EPI_ADD) launch_conv<9, true, EPI_ADD>(pl.MB, grid, s, a);         // DenseBlock 3 x 3'
  else if (taps == 9 && refl == REFL_RING && m && epi == EPI_STORE) launch_conv_r<true, EPI_STORE, REFL_RING>(pl.MB, grid, s, a);   // reflected'
  else PAIF_REQUIRE(false, PAIF_EINVAL, "bffusion_conv: taps %d, reflection %d, mask %d, epilogue %d is not a form of this network", taps, refl, (int)m, epi);
  PAIF_LAUNCH_CHECK("bffusion_conv");
  return 0;
}

extern "C" int paif_bffusion_fold(const float* ring, int M, int n_store, float* dst, int dst_cs, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(ring && dst, PAIF_EINVAL, "bffusion_fold: null pointer");
  BFF_CH("bffusion_fold", M, dst_cs);
  PAIF_REQUIRE(n_store >= 0 && n_store <= M && n_store % 4 == 0, PAIF_EINVAL, "bffusion_fold: n_store %d of %d", n_store, M);
  PAIF_SLAB_SHAPE("bffusion_fold", 1, "", 26);
  PAIF_REQUIRE(H >= 2 && W >= 2, PAIF_EINVAL, "bffusion_fold: reflection padding needs H, W >= 2");
  hipLaunchKernelGGL(fold_k, dim3(blocks(n * (M / 4))), dim3(256), 0, paif::as_stream(stream), ring, M, n_store, dst, dst_cs, H, W, n);
  PAIF_LAUNCH_CHECK("bffusion_fold");
  return 0;
}

extern "C" int paif_bffusion_stem_fwd(const float* x, size_t sb, const float* w, const float* bias, float* out, int out_cs, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(x && w && bias && out, PAIF_EINVAL, "bffusion_stem_fwd: null pointer");
  BFF_CH("bffusion_stem_fwd", 16, out_cs);
  PAIF_SLAB_SHAPE("bffusion_stem_fwd", 1, "", 26);
  PAIF_REQUIRE((size_t)H * W <= sb, PAIF_EINVAL, "bffusion_stem_fwd: batch stride smaller than a plane");
  hipLaunchKernelGGL(stem_fwd_k, dim3(blocks(n * 4)), dim3(256), 0, paif::as_stream(stream), x, sb, w, bias, out, out_cs, (size_t)H * W, n);
  PAIF_LAUNCH_CHECK("bffusion_stem_fwd");
  return 0;
}

extern "C" int paif_bffusion_stem_bwd(const float* w, const float* d, int d_cs, float* d_x, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(w && d && d_x, PAIF_EINVAL, "bffusion_stem_bwd: null pointer");
  BFF_CH("bffusion_stem_bwd", 16, d_cs);
  PAIF_SLAB_SHAPE("bffusion_stem_bwd", 1, "", 26);
  hipLaunchKernelGGL(stem_bwd_k, dim3(blocks(n)), dim3(256), 0, paif::as_stream(stream), w, d, d_cs, d_x, n);
  PAIF_LAUNCH_CHECK("bffusion_stem_bwd");
  return 0;
}

extern "C" int paif_bffusion_head_fwd(const float* w, const float* bias, const float* in, int in_cs, float* fused, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(w && bias && in && fused, PAIF_EINVAL, "bffusion_head_fwd: null pointer");
  BFF_CH("bffusion_head_fwd", 16, in_cs);
  PAIF_SLAB_SHAPE("bffusion_head_fwd", 1, "", 26);
  hipLaunchKernelGGL(head_fwd_k, dim3(blocks(n)), dim3(256), 0, paif::as_stream(stream), w, bias, in, in_cs, fused, n);
  PAIF_LAUNCH_CHECK("bffusion_head_fwd");
  return 0;
}

extern "C" int paif_bffusion_head_bwd(const float* w, const float* fused, const float* d_fused, float* d, int d_cs, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(w && fused && d_fused && d, PAIF_EINVAL, "bffusion_head_bwd: null pointer");
  BFF_CH("bffusion_head_bwd", 16, d_cs);
  PAIF_SLAB_SHAPE("bffusion_head_bwd", 1, "", 26);
  hipLaunchKernelGGL(head_bwd_k, dim3(blocks(n * 4)), dim3(256), 0, paif::as_stream(stream), w, fused, d_fused, d, d_cs, n);
  PAIF_LAUNCH_CHECK("bffusion_head_bwd");
  return 0;
}

// H, W: the map that is pooled; the pooled map is (H / 2) x (W / 2)
extern "C" int paif_bffusion_pool_fwd(const float* in, int in_cs, int C, float* out, int out_cs, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(in && out, PAIF_EINVAL, "bffusion_pool_fwd: null pointer");
  BFF_CH("bffusion_pool_fwd", C, in_cs);
  BFF_CH("bffusion_pool_fwd", C, out_cs);
  PAIF_SLAB_SHAPE("bffusion_pool_fwd", 1, "", 26);
  PAIF_REQUIRE(H >= 2 && W >= 2, PAIF_EINVAL, "bffusion_pool_fwd: a 2 x 2 window needs H, W >= 2");
  const int Hp = H / 2, Wp = W / 2;
  const size_t np = (size_t)B * Hp * Wp;
  hipLaunchKernelGGL(pool_fwd_k, dim3(blocks(np * (C / 4))), dim3(256), 0, paif::as_stream(stream), in, in_cs, C, H, W, out, out_cs, Hp, Wp, np);
  PAIF_LAUNCH_CHECK("bffusion_pool_fwd");
  return 0;
}

// ADDS into d_in (laid out as the taped map `in` is, at stride din_cs)
extern "C" int paif_bffusion_pool_bwd(const float* in, int in_cs, int C, const float* d_pooled, int dp_cs, float* d_in, int din_cs, int B, int H, int W,
                                      paif_stream_t stream) {
  PAIF_REQUIRE(in && d_pooled && d_in, PAIF_EINVAL, "bffusion_pool_bwd: null pointer");
  PAIF_REQUIRE(in != d_in && d_pooled != d_in, PAIF_EINVAL, "bffusion_pool_bwd: the map that is added to must be a third one");
  BFF_CH("bffusion_pool_bwd", C, in_cs);
  BFF_CH("bffusion_pool_bwd", C, dp_cs);
  BFF_CH("bffusion_pool_bwd", C, din_cs);
  PAIF_SLAB_SHAPE("bffusion_pool_bwd", 1, "", 26);
  PAIF_REQUIRE(H >= 2 && W >= 2, PAIF_EINVAL, "bffusion_pool_bwd: a 2 x 2 window needs H, W >= 2");
  hipLaunchKernelGGL(pool_bwd_k, dim3(blocks(n * C)), dim3(256), 0, paif::as_stream(stream), in, in_cs, C, H, W, d_pooled, dp_cs, H / 2, W / 2, d_in,
                     din_cs, n);
  PAIF_LAUNCH_CHECK("bffusion_pool_bwd");
  return 0;
}

// H, W: the DESTINATION; the source is (H / 2) x (W / 2)
extern "C" int paif_bffusion_up_fwd(const float* src, int src_cs, int C, float* dst, int dst_cs, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(src && dst, PAIF_EINVAL, "bffusion_up_fwd: null pointer");
  BFF_CH("bffusion_up_fwd", C, src_cs);
  BFF_CH("bffusion_up_fwd", C, dst_cs);
  PAIF_SLAB_SHAPE("bffusion_up_fwd", 1, "", 26);
  PAIF_REQUIRE(H >= 2 && W >= 2, PAIF_EINVAL, "bffusion_up_fwd: the destination needs H, W >= 2");
  hipLaunchKernelGGL(up_fwd_k, dim3(blocks(n * (C / 4))), dim3(256), 0, paif::as_stream(stream), src, src_cs, C, H / 2, W / 2, dst, dst_cs, H, W, n);
  PAIF_LAUNCH_CHECK("bffusion_up_fwd");
  return 0;
}

extern "C" int paif_bffusion_up_bwd(const float* d_dst, int dd_cs, int C, float* d_src, int ds_cs, int add, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(d_dst && d_src, PAIF_EINVAL, "bffusion_up_bwd: null pointer");
  BFF_CH("bffusion_up_bwd", C, dd_cs);
  BFF_CH("bffusion_up_bwd", C, ds_cs);
  PAIF_SLAB_SHAPE("bffusion_up_bwd", 1, "", 26);
  PAIF_REQUIRE(H >= 2 && W >= 2, PAIF_EINVAL, "bffusion_up_bwd: the destination needs H, W >= 2");
  const int Hs = H / 2, Ws = W / 2;
  const size_t ns = (size_t)B * Hs * Ws;
  const dim3 grid(blocks(ns * (C / 4)));
  if (add) hipLaunchKernelGGL(up_bwd_k<true>, grid, dim3(256), 0, paif::as_stream(stream), d_dst, dd_cs, C, H, W, d_src, ds_cs, Hs, Ws, ns);
  else hipLaunchKernelGGL(up_bwd_k<false>, grid, dim3(256), 0, paif::as_stream(stream), d_dst, dd_cs, C, H, W, d_src, ds_cs, Hs, Ws, ns);
  PAIF_LAUNCH_CHECK("bffusion_up_bwd");
  return 0;
}

// x_a, x_b: the last ffn maps, dense [.., C]
extern "C" int paif_bffusion_gate_fwd(const float* skip_a, int sa_cs, const float* x_a, const float* skip_b, int sb_cs, const float* x_b, int C,
                                      float* out, int out_cs, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(skip_a && x_a && skip_b && x_b && out, PAIF_EINVAL, "bffusion_gate_fwd: null pointer");
  BFF_CH("bffusion_gate_fwd", C, sa_cs);
  BFF_CH("bffusion_gate_fwd", C, sb_cs);
  BFF_CH("bffusion_gate_fwd", C, out_cs);
  PAIF_SLAB_SHAPE("bffusion_gate_fwd", 1, "", 26);
  hipLaunchKernelGGL(gate_fwd_k, dim3(blocks(n * (C / 4))), dim3(256), 0, paif::as_stream(stream), skip_a, sa_cs, x_a, skip_b, sb_cs, x_b, C, out, out_cs,
                     n);
  PAIF_LAUNCH_CHECK("bffusion_gate_fwd");
  return 0;
}

extern "C" int paif_bffusion_gate_bwd(const float* d_fused, int df_cs, const float* skip, int skip_cs, const float* x, int C, float* d_x, float* d_skip,
                                      int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(d_fused && skip && x && d_x && d_skip, PAIF_EINVAL, "bffusion_gate_bwd: null pointer");
  BFF_CH("bffusion_gate_bwd", C, df_cs);
  BFF_CH("bffusion_gate_bwd", C, skip_cs);
  PAIF_SLAB_SHAPE("bffusion_gate_bwd", 1, "", 26);
  hipLaunchKernelGGL(gate_bwd_k, dim3(blocks(n * (C / 4))), dim3(256), 0, paif::as_stream(stream), d_fused, df_cs, skip, skip_cs, x, C, d_x, d_skip, n);
  PAIF_LAUNCH_CHECK("bffusion_gate_bwd");
  return 0;
}

extern "C" int paif_bffusion_ln_fwd(const float* y, const float* gamma, const float* beta, float eps, int C, float* z, int B, int H, int W,
                                    paif_stream_t stream) {
  PAIF_REQUIRE(y && gamma && beta && z && y != z, PAIF_EINVAL, "bffusion_ln_fwd: null or aliased pointer");
  PAIF_REQUIRE(C >= 1 && eps >= 0.f, PAIF_EINVAL, "bffusion_ln_fwd: C = %d, eps = %g", C, eps);
  PAIF_SLAB_SHAPE("bffusion_ln_fwd", 1, "", 26);
  hipLaunchKernelGGL(ln_fwd_k, dim3(blocks(n)), dim3(256), 0, paif::as_stream(stream), y, gamma, beta, eps, C, z, n);
  PAIF_LAUNCH_CHECK("bffusion_ln_fwd");
  return 0;
}

extern "C" int paif_bffusion_ln_bwd(const float* y, const float* gamma, float eps, int C, const float* d_z, float* d_y, int B, int H, int W,
                                    paif_stream_t stream) {
  PAIF_REQUIRE(y && gamma && d_z && d_y && d_y != y && d_y != d_z, PAIF_EINVAL, "bffusion_ln_bwd: null or aliased pointer");
  PAIF_REQUIRE(C >= 1 && eps >= 0.f, PAIF_EINVAL, "bffusion_ln_bwd: C = %d, eps = %g", C, eps);
  PAIF_SLAB_SHAPE("bffusion_ln_bwd", 1, "", 26);
  hipLaunchKernelGGL(ln_bwd_k, dim3(blocks(n)), dim3(256), 0, paif::as_stream(stream), y, gamma, eps, C, d_z, d_y, n);
  PAIF_LAUNCH_CHECK("bffusion_ln_bwd");
  return 0;
}

extern "C" int paif_bffusion_ctx_chunks(int H, int W) { return H >= 1 && W >= 1 ? (int)(((size_t)H * W + CTX_CHUNK - 1) / CTX_CHUNK) : 0; }

#define BFF_HEADS(name)                                                                                                       \
  PAIF_REQUIRE(dim >= 4 && d >= 1 && d <= MAX_D && dim % d == 0 && dim * d <= 1024, PAIF_EINVAL, name ": dim %d, head dim %d", dim, d); \
  const int chunks = paif_bffusion_ctx_chunks(H, W);                                                                          \
  (void)chunks

// partial: B x chunks x dim d doubles
extern "C" int paif_bffusion_ctx_partial(const float* a, int a_cs, const float* b, int b_cs, int dim, int d, double* partial, int B, int H, int W,
                                         paif_stream_t stream) {
  PAIF_REQUIRE(a && b && partial, PAIF_EINVAL, "bffusion_ctx_partial: null pointer");
  PAIF_REQUIRE(a_cs >= dim && b_cs >= dim, PAIF_EINVAL, "bffusion_ctx_partial: stride below dim");
  PAIF_SLAB_SHAPE("bffusion_ctx_partial", 1, "", 26);
  BFF_HEADS("bffusion_ctx_partial");
  PAIF_REQUIRE(B <= 65535, PAIF_EINVAL, "bffusion_ctx_partial: batch above 65535");
  hipLaunchKernelGGL(ctx_partial_k, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, paif::as_stream(stream), a, a_cs, b, b_cs, dim, d, H * W, chunks,
                     partial);
  PAIF_LAUNCH_CHECK("bffusion_ctx_partial");
  return 0;
}

extern "C" int paif_bffusion_ctx_softmax(const double* partial, int dim, int d, float scale, float* ctx, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(partial && ctx, PAIF_EINVAL, "bffusion_ctx_softmax: null pointer");
  PAIF_SLAB_SHAPE("bffusion_ctx_softmax", 1, "", 26);
  BFF_HEADS("bffusion_ctx_softmax");
  hipLaunchKernelGGL(ctx_softmax_k, dim3(blocks((size_t)B * dim)), dim3(256), 0, paif::as_stream(stream), partial, chunks, dim, d, scale, ctx, B * dim);
  PAIF_LAUNCH_CHECK("bffusion_ctx_softmax");
  return 0;
}

extern "C" int paif_bffusion_ctx_softmax_bwd(const double* partial, int dim, int d, float scale, const float* ctx, float* d_s, int B, int H, int W,
                                             paif_stream_t stream) {
  PAIF_REQUIRE(partial && ctx && d_s, PAIF_EINVAL, "bffusion_ctx_softmax_bwd: null pointer");
  PAIF_SLAB_SHAPE("bffusion_ctx_softmax_bwd", 1, "", 26);
  BFF_HEADS("bffusion_ctx_softmax_bwd");
  hipLaunchKernelGGL(ctx_softmax_bwd_k, dim3(blocks((size_t)B * dim)), dim3(256), 0, paif::as_stream(stream), partial, chunks, dim, d, scale, ctx, d_s,
                     B * dim);
  PAIF_LAUNCH_CHECK("bffusion_ctx_softmax_bwd");
  return 0;
}

extern "C" int paif_bffusion_attn_apply_fwd(const float* qkv, const float* ctx, int dim, int d, float* x, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(qkv && ctx && x, PAIF_EINVAL, "bffusion_attn_apply_fwd: null pointer");
  PAIF_SLAB_SHAPE("bffusion_attn_apply_fwd", 1, "", 26);
  BFF_HEADS("bffusion_attn_apply_fwd");
  hipLaunchKernelGGL(attn_apply_fwd_k, dim3(blocks(n * dim)), dim3(256), 0, paif::as_stream(stream), qkv, ctx, dim, d, H * W, x, n);
  PAIF_LAUNCH_CHECK("bffusion_attn_apply_fwd");
  return 0;
}

extern "C" int paif_bffusion_attn_apply_bwd(const float* qkv, const float* d_x, const float* ctx, const float* d_s, int dim, int d, float* d_qkv, int B,
                                            int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(qkv && d_x && ctx && d_s && d_qkv, PAIF_EINVAL, "bffusion_attn_apply_bwd: null pointer");
  PAIF_SLAB_SHAPE("bffusion_attn_apply_bwd", 1, "", 26);
  BFF_HEADS("bffusion_attn_apply_bwd");
  hipLaunchKernelGGL(attn_apply_bwd_k, dim3(blocks(n * dim)), dim3(256), 0, paif::as_stream(stream), qkv, d_x, ctx, d_s, dim, d, H * W, d_qkv, n);
  PAIF_LAUNCH_CHECK("bffusion_attn_apply_bwd");
  return 0;
}
