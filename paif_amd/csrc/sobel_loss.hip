// Sobel fusion criteria of the training API (core/loss.py:423-603: Fusionloss, Fusionloss2/3/4/6, Fusionloss_add,
// Total_fusion_loss3) and the operator they share (Sobelxy, core/loss.py:634-650):
//   S(x) = |Gx * x| + |Gy * x|,  Gx = [-1 0 1; -2 0 2; -1 0 1],  Gy = [1 2 1; 0 0 0; -1 -2 -1]  (cross-correlation, zero padding 1,
//   every image of the batch padded on its own).
// A criterion is a weighted sum of up to two intensity terms mean|T - f| and one gradient term mean|Q - S(f)| on the generated
// plane f, with T / Q formed from the planes a (infrared channel 0), b (Y) and m (mask channel 0): paif_sobel_desc.
//
// Forward: one workgroup = a 32 x 64 tile of one image, 2 x 4 pixels per thread; the 34 x 66 halo tiles of the planes the terms
// read sit in LDS, zero outside the image.  The three sums are reduced in the wave by shuffles, then over the four waves in a
// fixed order into partial[3 * block + term]; sobel_loss_finish_kernel adds the partials in block order in double.  No float
// atomics, no workgroup waits for another, nothing returns to the host.
//
// Gradient w.r.t. f: df = -sum_i k_i sign(T_i - f) + Gx^T(e sign(Gx f)) + Gy^T(e sign(Gy f)),  e = -k_q sign(Q - S(f)),
// sign(0) = 0 everywhere (torch's abs and l1_loss at a tie).  One launch: the planes with a halo of 2 in LDS, the two products
// e sign(G f) once per position of the 34 x 66 tile into LDS as small integers (-1, 0, 1), then each output pixel gathers its
// twelve neighbours; k_q multiplies the integer sum once.  k_i = upstream gradient (read from device memory) * weight_i / N.
#include <limits.h>

#include "paif_common.h"

namespace {

constexpr int TH = 32, TW = 64, NT = 256;   // tile of one workgroup; thread (tid >> 4, tid & 15) owns rows 2 ly.., columns 4 lx..

__device__ __forceinline__ float sgn(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
// alpha * a + beta * b as torch forms it: two rounded products, one rounded sum (no contraction into an fma)
__device__ __forceinline__ float lin2(float al, float a, float be, float b) { return __fadd_rn(__fmul_rn(al, a), __fmul_rn(be, b)); }

// (TH + 2R) x (TW + 2R) tile of one plane with its top-left corner at (y0, x0): unconditional clamped load, zero by select
template <int R>
__device__ __forceinline__ void stage(float* __restrict__ s, const float* __restrict__ p, int y0, int x0, int H, int W, int tid) {
  constexpr int HH = TH + 2 * R, WW = TW + 2 * R;
  for (int i = tid; i < HH * WW; i += NT) {
    const int r = i / WW, c = i - r * WW;
    const int gy = y0 + r, gx = x0 + c;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    const float v = p[(size_t)min(max(gy, 0), H - 1) * W + min(max(gx, 0), W - 1)];
    s[i] = in ? v : 0.f;
  }
}

// the Sobel pair at the centre of a 3 x 3 neighbourhood given by ld(dr, dc)
template <class L>
__device__ __forceinline__ void sobel_pair(L ld, float& gx, float& gy) {
  const float nw = ld(-1, -1), n = ld(-1, 0), ne = ld(-1, 1), w = ld(0, -1), e = ld(0, 1), sw = ld(1, -1), s = ld(1, 0), se = ld(1, 1);
  gx = (ne + 2.f * e + se) - (nw + 2.f * w + sw);
  gy = (nw + 2.f * n + ne) - (sw + 2.f * s + se);
}
template <class L>
__device__ __forceinline__ float sobel_abs(L ld) {
  float gx, gy;
  sobel_pair(ld, gx, gy);
  return fabsf(gx) + fabsf(gy);
}

// target of an intensity term at LDS offset o
__device__ __forceinline__ float target_t(int kind, float al, float be, const float* sa, const float* sb, const float* sm, int o) {
  if (kind == PAIF_SOBEL_MAX) return fmaxf(sa[o], sb[o]);
  if (kind == PAIF_SOBEL_MASK) return sm[o];
  return lin2(al, sa[o], be, sb[o]);
}
// target of the gradient term at LDS offset o of planes with pitch P
__device__ __forceinline__ float target_q(int kind, float al, float be, const float* sa, const float* sb, const float* sm, int o, int P) {
  if (kind == PAIF_SOBEL_MAX)
    return fmaxf(sobel_abs([&](int dr, int dc) { return sa[o + dr * P + dc]; }), sobel_abs([&](int dr, int dc) { return sb[o + dr * P + dc]; }));
  if (kind == PAIF_SOBEL_MASK) return sobel_abs([&](int dr, int dc) { return sm[o + dr * P + dc]; });
  return sobel_abs([&](int dr, int dc) { return lin2(al, sa[o + dr * P + dc], be, sb[o + dr * P + dc]); });
}

struct tile_id { int b, ty, tx; };
__device__ __forceinline__ tile_id tile_of(int t, int tilesX, int tilesY) {
  tile_id r;
  r.tx = t % tilesX; t /= tilesX;
  r.ty = t % tilesY;
  r.b = t / tilesY;
  return r;
}

__global__ __launch_bounds__(NT) void sobel_loss_kernel(paif_sobel_desc d, float* __restrict__ partial, int H, int W, int tilesX, int tilesY) {
  constexpr int P = TW + 2, HH = TH + 2;
  __shared__ float sf[HH * P], sa[HH * P], sb[HH * P], sm[HH * P];
  __shared__ float red[3][4];
  const int tid = threadIdx.x;
  const tile_id t = tile_of(blockIdx.x, tilesX, tilesY);
  const int y0 = t.ty * TH - 1, x0 = t.tx * TW - 1;
  stage<1>(sf, d.f + (size_t)t.b * d.f_bs, y0, x0, H, W, tid);
  if (d.a) stage<1>(sa, d.a + (size_t)t.b * d.a_bs, y0, x0, H, W, tid);
  if (d.b) stage<1>(sb, d.b + (size_t)t.b * d.b_bs, y0, x0, H, W, tid);
  if (d.m) stage<1>(sm, d.m + (size_t)t.b * d.m_bs, y0, x0, H, W, tid);
  __syncthreads();
  const int ly = (tid >> 4) * 2, lx = (tid & 15) * 4;
  float s0 = 0.f, s1 = 0.f, sq = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      if (t.ty * TH + ly + j < H && t.tx * TW + lx + i < W) {
        const int o = (ly + j + 1) * P + lx + i + 1;
        const float fv = sf[o];
        if (d.t_kind[0]) s0 += fabsf(target_t(d.t_kind[0], d.t_alpha[0], d.t_beta[0], sa, sb, sm, o) - fv);
        if (d.t_kind[1]) s1 += fabsf(target_t(d.t_kind[1], d.t_alpha[1], d.t_beta[1], sa, sb, sm, o) - fv);
        if (d.q_kind) {
          const float q = target_q(d.q_kind, d.q_alpha, d.q_beta, sa, sb, sm, o, P);
          sq += fabsf(q - sobel_abs([&](int dr, int dc) { return sf[o + dr * P + dc]; }));
        }
      }
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    s0 += __shfl_xor(s0, m);
    s1 += __shfl_xor(s1, m);
    sq += __shfl_xor(sq, m);
  }
  if ((tid & 63) == 0) { red[0][tid >> 6] = s0; red[1][tid >> 6] = s1; red[2][tid >> 6] = sq; }
  __syncthreads();
  if (tid < 3) partial[3 * (size_t)blockIdx.x + tid] = (red[tid][0] + red[tid][1]) + (red[tid][2] + red[tid][3]);
}

// out[i] = mean of term i (i = 0, 1: intensity, 2: gradient), out[3] = sum_i weight_i * mean_i; block order, double
__global__ void sobel_loss_finish_kernel(const float* __restrict__ partial, int nblk, double inv_n, float w0, float w1, float wq,
                                         float* __restrict__ out) {
  __shared__ double sl[3][64];
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) {
    a += partial[3 * (size_t)i]; b += partial[3 * (size_t)i + 1]; c += partial[3 * (size_t)i + 2];
  }
  sl[0][threadIdx.x] = a; sl[1][threadIdx.x] = b; sl[2][threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x == 0) {
    double m[3];
    for (int k = 0; k < 3; ++k) {
      double s = 0.0;
      for (int i = 0; i < 64; ++i) s += sl[k][i];
      m[k] = s * inv_n;
      out[k] = (float)m[k];
    }
    out[3] = (float)((double)w0 * m[0] + (double)w1 * m[1] + (double)wq * m[2]);
  }
}

// MAP = false: the criterion's gradient (cot = the upstream scalar, c* = weight / N); MAP = true: Sobelxy's adjoint, cot = the
// per-pixel cotangent map [B,1,H,W] (dense), no intensity terms.
template <bool MAP>
__global__ __launch_bounds__(NT) void sobel_bwd_kernel(paif_sobel_desc d, const float* __restrict__ cot, float c0, float c1, float cq,
                                                       float* __restrict__ df, int H, int W, int tilesX, int tilesY) {
  constexpr int P2 = TW + 4, H2 = TH + 4, P1 = TW + 2, H1 = TH + 2;
  __shared__ float sf[H2 * P2];
  __shared__ float sabm[MAP ? 1 : 3 * H2 * P2];
  __shared__ float ux[H1 * P1], uy[H1 * P1];
  const float *sa = sabm, *sb = sabm + (MAP ? 0 : H2 * P2), *sm = sabm + (MAP ? 0 : 2 * H2 * P2);
  const int tid = threadIdx.x;
  const tile_id t = tile_of(blockIdx.x, tilesX, tilesY);
  const int y0 = t.ty * TH, x0 = t.tx * TW;
  const size_t img = (size_t)t.b * H * W;   // df and the cotangent map are dense
  stage<2>(sf, d.f + (size_t)t.b * d.f_bs, y0 - 2, x0 - 2, H, W, tid);
  if constexpr (!MAP) {
    if (d.a) stage<2>(sabm, d.a + (size_t)t.b * d.a_bs, y0 - 2, x0 - 2, H, W, tid);
    if (d.b) stage<2>(sabm + H2 * P2, d.b + (size_t)t.b * d.b_bs, y0 - 2, x0 - 2, H, W, tid);
    if (d.m) stage<2>(sabm + 2 * H2 * P2, d.m + (size_t)t.b * d.m_bs, y0 - 2, x0 - 2, H, W, tid);
  }
  __syncthreads();
  const bool has_q = MAP || d.q_kind != 0;
  if (has_q) {
    for (int i = tid; i < H1 * P1; i += NT) {
      const int r = i / P1, c = i - r * P1;
      const int gy = y0 - 1 + r, gx = x0 - 1 + c;
      float vx = 0.f, vy = 0.f;
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {   // a position outside the image has no output pixel: its products stay zero
        const int o = (r + 1) * P2 + c + 1;
        float fx, fy;
        sobel_pair([&](int dr, int dc) { return sf[o + dr * P2 + dc]; }, fx, fy);
        float e;
        if constexpr (MAP) e = cot[img + (size_t)gy * W + gx];
        else e = -sgn(target_q(d.q_kind, d.q_alpha, d.q_beta, sa, sb, sm, o, P2) - (fabsf(fx) + fabsf(fy)));
        vx = e * sgn(fx);
        vy = e * sgn(fy);
      }
      ux[i] = vx;
      uy[i] = vy;
    }
    __syncthreads();
  }
  float k0 = 0.f, k1 = 0.f, kq = 1.f;
  if constexpr (!MAP) {
    const float g = cot[0];
    k0 = g * c0; k1 = g * c1; kq = g * cq;
  }
  const int ly = (tid >> 4) * 2, lx = (tid & 15) * 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int py = y0 + ly + j;
    if (py >= H) continue;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float acc = 0.f;
      if (has_q) {
        const int o = (ly + j + 1) * P1 + lx + i + 1;
        acc = ((ux[o - P1 - 1] + 2.f * ux[o - 1] + ux[o + P1 - 1]) - (ux[o - P1 + 1] + 2.f * ux[o + 1] + ux[o + P1 + 1])) +
              ((uy[o + P1 - 1] + 2.f * uy[o + P1] + uy[o + P1 + 1]) - (uy[o - P1 - 1] + 2.f * uy[o - P1] + uy[o - P1 + 1]));
      }
      if constexpr (!MAP) {
        const int o2 = (ly + j + 2) * P2 + lx + i + 2;
        const float fv = sf[o2];
        acc *= kq;
        if (d.t_kind[0]) acc -= k0 * sgn(target_t(d.t_kind[0], d.t_alpha[0], d.t_beta[0], sa, sb, sm, o2) - fv);
        if (d.t_kind[1]) acc -= k1 * sgn(target_t(d.t_kind[1], d.t_alpha[1], d.t_beta[1], sa, sb, sm, o2) - fv);
      }
      v[i] = acc;
    }
    const int px = x0 + lx;
    float* o = df + img + (size_t)py * W + px;
    if ((W & 3) == 0) {   // then px + 3 < W whenever px < W, and the row starts on 16 bytes
      if (px < W) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < W) o[i] = v[i];
    }
  }
}

// out = S(x)
__global__ __launch_bounds__(NT) void sobelxy_kernel(const float* __restrict__ x, size_t x_bs, float* __restrict__ out, int H, int W, int tilesX,
                                                     int tilesY) {
  constexpr int P = TW + 2, HH = TH + 2;
  __shared__ float sx[HH * P];
  const int tid = threadIdx.x;
  const tile_id t = tile_of(blockIdx.x, tilesX, tilesY);
  const int y0 = t.ty * TH, x0 = t.tx * TW;
  stage<1>(sx, x + (size_t)t.b * x_bs, y0 - 1, x0 - 1, H, W, tid);
  __syncthreads();
  const int ly = (tid >> 4) * 2, lx = (tid & 15) * 4;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int py = y0 + ly + j;
    if (py >= H) continue;
    float v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int o = (ly + j + 1) * P + lx + i + 1;
      v[i] = sobel_abs([&](int dr, int dc) { return sx[o + dr * P + dc]; });
    }
    const int px = x0 + lx;
    float* o = out + (size_t)t.b * H * W + (size_t)py * W + px;
    if ((W & 3) == 0) {
      if (px < W) *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (px + i < W) o[i] = v[i];
    }
  }
}

// number of 32 x 64 tiles of a batch, or -1 where it does not fit the 32-bit block index
inline long long tiles_of(int B, int H, int W) { return (long long)B * ((H + TH - 1) / TH) * ((W + TW - 1) / TW); }

inline bool kind_ok(int k) { return k >= PAIF_SOBEL_NONE && k <= PAIF_SOBEL_LIN; }
inline bool needs_ab(int k) { return k == PAIF_SOBEL_MAX || k == PAIF_SOBEL_LIN; }

int check_desc(const paif_sobel_desc* d, int B, int H, int W, const char* who) {
  PAIF_REQUIRE(d && d->f && B > 0 && H > 0 && W > 0, PAIF_EINVAL, "%s: bad arguments", who);
  PAIF_REQUIRE(tiles_of(B, H, W) <= INT_MAX, PAIF_ENOSUP, "%s: %d x %d x %d needs more than 2^31 - 1 tiles of %d x %d", who, B, H, W, TH, TW);
  const size_t HW = (size_t)H * W;
  const int ks[3] = {d->t_kind[0], d->t_kind[1], d->q_kind};
  bool ab = false, mk = false;
  for (int k : ks) {
    PAIF_REQUIRE(kind_ok(k), PAIF_EINVAL, "%s: term kind %d", who, k);
    ab |= needs_ab(k);
    mk |= k == PAIF_SOBEL_MASK;
  }
  PAIF_REQUIRE(!ab || (d->a && d->b), PAIF_EINVAL, "%s: a term reads the image planes a, b and one of them is NULL", who);
  PAIF_REQUIRE(!mk || d->m, PAIF_EINVAL, "%s: a term reads the mask plane and it is NULL", who);
  PAIF_REQUIRE(B == 1 || (d->f_bs >= HW && (!d->a || d->a_bs >= HW) && (!d->b || d->b_bs >= HW) && (!d->m || d->m_bs >= HW)), PAIF_EINVAL,
               "%s: a batch stride is smaller than one %d x %d plane", who, H, W);
  return 0;
}

}  // namespace

extern "C" int paif_sobel_loss_blocks(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  const long long n = tiles_of(B, H, W);
  return n <= INT_MAX ? (int)n : -1;
}

extern "C" int paif_sobel_loss_fwd(const paif_sobel_desc* d, float* partial, float* out, int B, int H, int W, paif_stream_t stream) {
  if (int rc = check_desc(d, B, H, W, "sobel_loss")) return rc;
  PAIF_REQUIRE(partial && out, PAIF_EINVAL, "sobel_loss: bad arguments");
  const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH, nblk = B * tilesX * tilesY;
  hipStream_t st = paif::as_stream(stream);
  hipLaunchKernelGGL(sobel_loss_kernel, dim3(nblk), dim3(NT), 0, st, *d, partial, H, W, tilesX, tilesY);
  PAIF_LAUNCH_CHECK("sobel_loss");
  hipLaunchKernelGGL(sobel_loss_finish_kernel, dim3(1), dim3(64), 0, st, partial, nblk, 1.0 / ((double)B * H * W), d->t_weight[0],
                     d->t_weight[1], d->q_weight, out);
  PAIF_LAUNCH_CHECK("sobel_loss_finish");
  return 0;
}

extern "C" int paif_sobel_loss_bwd(const paif_sobel_desc* d, const float* g, float* df, int B, int H, int W, paif_stream_t stream) {
  if (int rc = check_desc(d, B, H, W, "sobel_loss_bwd")) return rc;
  PAIF_REQUIRE(g && df, PAIF_EINVAL, "sobel_loss_bwd: bad arguments");
  const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
  const double n = (double)B * H * W;
  hipLaunchKernelGGL(sobel_bwd_kernel<false>, dim3(B * tilesX * tilesY), dim3(NT), 0, paif::as_stream(stream), *d, g,
                     (float)(d->t_weight[0] / n), (float)(d->t_weight[1] / n), (float)(d->q_weight / n), df, H, W, tilesX, tilesY);
  PAIF_LAUNCH_CHECK("sobel_loss_bwd");
  return 0;
}

extern "C" int paif_sobelxy_fwd(const float* x, size_t x_bs, float* out, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(x && out && B > 0 && H > 0 && W > 0 && (B == 1 || x_bs >= (size_t)H * W), PAIF_EINVAL, "sobelxy: bad arguments");
  PAIF_REQUIRE(tiles_of(B, H, W) <= INT_MAX, PAIF_ENOSUP, "sobelxy: %d x %d x %d needs more than 2^31 - 1 tiles of %d x %d", B, H, W, TH, TW);
  const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
  hipLaunchKernelGGL(sobelxy_kernel, dim3(B * tilesX * tilesY), dim3(NT), 0, paif::as_stream(stream), x, x_bs, out, H, W, tilesX, tilesY);
  PAIF_LAUNCH_CHECK("sobelxy");
  return 0;
}

extern "C" int paif_sobelxy_bwd(const float* x, size_t x_bs, const float* g, float* dx, int B, int H, int W, paif_stream_t stream) {
  PAIF_REQUIRE(x && g && dx && B > 0 && H > 0 && W > 0 && (B == 1 || x_bs >= (size_t)H * W), PAIF_EINVAL, "sobelxy_bwd: bad arguments");
  PAIF_REQUIRE(tiles_of(B, H, W) <= INT_MAX, PAIF_ENOSUP, "sobelxy_bwd: %d x %d x %d needs more than 2^31 - 1 tiles of %d x %d", B, H, W, TH,
               TW);
  const int tilesX = (W + TW - 1) / TW, tilesY = (H + TH - 1) / TH;
  paif_sobel_desc d = {};
  d.f = x;
  d.f_bs = x_bs;
  hipLaunchKernelGGL(sobel_bwd_kernel<true>, dim3(B * tilesX * tilesY), dim3(NT), 0, paif::as_stream(stream), d, g, 0.f, 0.f, 0.f, dx, H, W,
                     tilesX, tilesY);
  PAIF_LAUNCH_CHECK("sobelxy_bwd");
  return 0;
}
