// The segmentation criteria of the training path (core/loss.py:342-383: NormalLoss, SoftmaxFocalLoss, OhemCELoss) on bilinearly
// upsampled logits, value and gradient w.r.t. the FULL-RESOLUTION logits, without the full-resolution logits ever being stored and
// without a sort or a host read:
//
//   o[c]  = bilinear(logits)[c] at the label's resolution (F.interpolate, align_corners=False; bilinear_src.h)
//   l_i   = max(logsumexp(o) - o[label], 0) on valid pixels, 0 on ignored ones (an ignored pixel still counts as an element)
//   kind 0  NormalLoss   sum_i l_i / n                                   (n = ALL pixels)
//   kind 1  Focal        sum_valid -(1-p)^gamma log p / #valid,          1 - p = sum_{c != label} exp(o_c - lse)
//   kind 2  OHEM         cnt = #{l_i > T};  cnt >= n_min: mean{l_i > T}   (mode A)
//                        else, v = the n_min-th largest l:  (sum_{l > v} l + (n_min - n_gt) v) / n_min   (mode B)
//
// v is found exactly by a radix select over the fp32 bit pattern of l (l >= 0, so the pattern orders as an unsigned integer): three
// histogram levels of 11 / 11 / 10 bits, LDS histograms with integer atomics merged by integer global atomics (order-independent),
// a one-wave pick kernel after each.  The mode is decided on the device; in mode A the later passes return at once.
// Float sums: per-block partials in a fixed lane order, then ONE wave adds the blocks in a fixed order in double -- no float atomics,
// two runs are bit-equal.
//
// Gradient (mode B): 1/n_min where l_i > v; the pixels with l_i == v share the remaining (n_min - n_gt)/n_min equally (torch's sort
// hands it to an unspecified subset of the ties; the value is the same).  Focal: where 1 - p is exactly 0 the gradient is 0.
#include <math.h>

#include "bilinear_src.h"
#include "paif_common.h"

namespace {

constexpr int SC_MAXC = 32;        // = CE_MAXC of upsample_ce
constexpr int SC_MAXGRID = 256 * 8;
constexpr int KIND_NORMAL = 0, KIND_FOCAL = 1, KIND_OHEM = 2;

// workspace, in 4-byte words: three histograms, counters + select state (all zeroed per call), then 3 float partials per block
constexpr int H0_BINS = 2048, H1_BINS = 2048, H2_BINS = 1024;      // bits 31..21, 20..10, 9..0
constexpr int H0_OFF = 0, H1_OFF = H0_OFF + H0_BINS, H2_OFF = H1_OFF + H1_BINS, CTR_OFF = H2_OFF + H2_BINS;
constexpr int CTR_WORDS = 16, PART_OFF = CTR_OFF + CTR_WORDS;
constexpr int SC_NPART = 3;        // plain sum, sum{l > T}, sum{l > v}
enum { C_VALID = 0, C_BAD = 1, C_GT_T = 2, C_NGT = 3, C_NTIE = 4, S_MODE_A = 8, S_PREFIX = 9, S_K = 10 };

inline int sc_grid(size_t n) {
  size_t g = (n + 255) / 256;
  if (g > (size_t)SC_MAXGRID) g = SC_MAXGRID;
  return (int)(g < 1 ? 1 : g);
}

__device__ __forceinline__ float block_sum(float v, float* s4) {   // every thread calls; result valid in thread 0
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

__device__ __forceinline__ unsigned block_sum_u(unsigned v, unsigned* s4) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s4[threadIdx.x >> 6] = v;
  __syncthreads();
  return (s4[0] + s4[1]) + (s4[2] + s4[3]);
}

// nonzero bins of the block's LDS histogram -> the global one (integer atomics: exact, order-independent)
__device__ __forceinline__ void merge_hist(const unsigned* h, unsigned* __restrict__ g, int nbins) {
  for (int b = threadIdx.x; b < nbins; b += 256) {
    const unsigned c = h[b];
    if (c) atomicAdd(&g[b], c);
  }
}

#define PAIF_INTERP(c) (hy * (hx * p00[c] + lx * p01[c]) + ly * (hx * p10[c] + lx * p11[c]))

// One thread per output pixel: l_i (or the focal term) and lse_i as two planes, the block's partial sums, the counters, and for
// OHEM the first-level histogram.  param = gamma (focal) or T (OHEM).
template <int KIND>
__global__ __launch_bounds__(256) void seg_pixel_kernel(const float* __restrict__ logits, const long long* __restrict__ label,
                                                        float* __restrict__ lplane, float* __restrict__ lseplane,
                                                        unsigned* __restrict__ ws, float param, int B, int IH, int IW, int C, int OH,
                                                        int OW, int ignore) {
  __shared__ unsigned hist[KIND == KIND_OHEM ? H0_BINS : 1];
  __shared__ float sf[4];
  __shared__ unsigned su[4];
  if (KIND == KIND_OHEM) {
    for (int b = threadIdx.x; b < H0_BINS; b += 256) hist[b] = 0;
    __syncthreads();
  }
  const size_t total = (size_t)B * OH * OW;
  const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
  float s_all = 0.f, s_t = 0.f;
  unsigned n_valid = 0, n_bad = 0, n_t = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    size_t t = i / OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    const long long lab = label[i];
    // a label outside [0, C) that is not `ignore`: dropped like an ignored pixel, counted, never used as an index
    const bool bad = lab != (long long)ignore && (lab < 0 || lab >= (long long)C);
    const bool valid = lab != (long long)ignore && !bad;
    n_bad += bad ? 1u : 0u;
    float l = 0.f, lse = 0.f;
    if (valid) {
      int y0, y1, x0, x1; float ly, lx;
      paif::src_index(sy, oy, IH, y0, y1, ly);
      paif::src_index(sx, ox, IW, x0, x1, lx);
      const float hy = 1.f - ly, hx = 1.f - lx;
      const float* p00 = logits + (((size_t)b * IH + y0) * IW + x0) * C;
      const float* p01 = logits + (((size_t)b * IH + y0) * IW + x1) * C;
      const float* p10 = logits + (((size_t)b * IH + y1) * IW + x0) * C;
      const float* p11 = logits + (((size_t)b * IH + y1) * IW + x1) * C;
      // the interpolated logits are recomputed per pass instead of being kept in a runtime-indexed array (scratch memory)
      float mx = -INFINITY;
#pragma unroll 1
      for (int c = 0; c < C; ++c) mx = fmaxf(mx, PAIF_INTERP(c));
      float se = 0.f, se_other = 0.f;
#pragma unroll 1
      for (int c = 0; c < C; ++c) {
        const float e = expf(PAIF_INTERP(c) - mx);
        se += e;
        if (KIND == KIND_FOCAL && c != (int)lab) se_other += e;
      }
      lse = mx + logf(se);
      const float nll = lse - PAIF_INTERP((int)lab);
      if (KIND == KIND_FOCAL) {
        const float q = se_other / se;                    // 1 - p as the sum over the other classes, not as 1 - exp(.)
        l = fmaxf(powf(q, param) * nll, 0.f);             // powf(0, 0) = 1, as torch.pow
      } else {
        l = fmaxf(nll, 0.f);                              // >= 0: the bit pattern orders as an unsigned integer
      }
      n_valid += 1u;
    }
    lplane[i] = l;
    lseplane[i] = lse;
    s_all += l;
    if (KIND == KIND_OHEM) {
      if (l > param) { s_t += l; n_t += 1u; }
      atomicAdd(&hist[__float_as_uint(l) >> 21], 1u);
    }
  }
  float* partial = reinterpret_cast<float*>(ws + PART_OFF);
  unsigned* ctr = ws + CTR_OFF;
  const float b_all = block_sum(s_all, sf);
  const unsigned b_valid = block_sum_u(n_valid, su);
  const unsigned b_bad = block_sum_u(n_bad, su);
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = b_all;
    if (b_valid) atomicAdd(&ctr[C_VALID], b_valid);
    if (b_bad) atomicAdd(&ctr[C_BAD], b_bad);
  }
  if (KIND == KIND_OHEM) {
    const float b_t = block_sum(s_t, sf);
    const unsigned b_nt = block_sum_u(n_t, su);
    if (threadIdx.x == 0) {
      partial[gridDim.x + blockIdx.x] = b_t;
      if (b_nt) atomicAdd(&ctr[C_GT_T], b_nt);
    }
    merge_hist(hist, ws + H0_OFF, H0_BINS);      // block_sum's barriers are behind every LDS atomic above
  }
}

// One wave.  Level 0 decides the mode (cnt >= n_min: mode A, nothing more to select).  Otherwise: the bin of this level's histogram
// (the elements that match the prefix found so far) that holds the k-th largest element; prefix and k move one level down.
__global__ __launch_bounds__(64) void seg_pick_kernel(unsigned* __restrict__ ws, int hist_off, int nbins, int shift, int level,
                                                      unsigned n_min) {
  __shared__ unsigned lane_sum[64];
  unsigned* ctr = ws + CTR_OFF;
  const unsigned* hist = ws + hist_off;
  const int lane = threadIdx.x;
  if (level == 0) {
    if (ctr[C_GT_T] >= n_min) {                    // wave-uniform
      if (lane == 0) ctr[S_MODE_A] = 1u;
      return;
    }
  } else if (ctr[S_MODE_A] == 1u) {
    return;
  }
  const unsigned k = level == 0 ? n_min : ctr[S_K];
  const unsigned prefix = level == 0 ? 0u : ctr[S_PREFIX];
  const int per = nbins / 64;                      // lane 0 owns the `per` highest bins, and so on downwards
  unsigned s = 0;
  for (int j = 0; j < per; ++j) s += hist[nbins - 1 - lane * per - j];
  lane_sum[lane] = s;
  __syncthreads();
  if (lane == 0) {
    unsigned acc = 0;
    int L = 0;
    for (; L < 63; ++L) {
      if (acc + lane_sum[L] >= k) break;
      acc += lane_sum[L];
    }
    int bin = nbins - 1 - L * per;
    for (int j = 0; j < per - 1; ++j) {            // the histogram holds at least k elements, so the last bin needs no test
      const unsigned c = hist[bin];
      if (acc + c >= k) break;
      acc += c;
      --bin;
    }
    ctr[S_PREFIX] = prefix | ((unsigned)bin << shift);
    ctr[S_K] = k - acc;
  }
}

// histogram of this level's bits over the elements whose higher bits match the prefix
__global__ __launch_bounds__(256) void seg_hist_kernel(const float* __restrict__ lplane, size_t total, unsigned* __restrict__ ws,
                                                       int hist_off, int nbins, int shift, int match_shift) {
  __shared__ unsigned hist[2048];
  const unsigned* ctr = ws + CTR_OFF;
  if (ctr[S_MODE_A] == 1u) return;                 // launch-uniform
  const unsigned want = ctr[S_PREFIX] >> match_shift;
  for (int b = threadIdx.x; b < nbins; b += 256) hist[b] = 0;
  __syncthreads();
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const unsigned bits = __float_as_uint(lplane[i]);
    if ((bits >> match_shift) == want) atomicAdd(&hist[(bits >> shift) & (unsigned)(nbins - 1)], 1u);
  }
  __syncthreads();
  merge_hist(hist, ws + hist_off, nbins);
}

// with v known: sum{l > v} per block, n_gt and n_tie
__global__ __launch_bounds__(256) void seg_select_sum_kernel(const float* __restrict__ lplane, size_t total, unsigned* __restrict__ ws) {
  __shared__ float sf[4];
  __shared__ unsigned su[4];
  unsigned* ctr = ws + CTR_OFF;
  if (ctr[S_MODE_A] == 1u) return;                 // launch-uniform
  const unsigned vbits = ctr[S_PREFIX];
  float s = 0.f;
  unsigned ngt = 0, ntie = 0;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const float l = lplane[i];
    const unsigned bits = __float_as_uint(l);
    if (bits > vbits) { s += l; ngt += 1u; }
    ntie += bits == vbits ? 1u : 0u;
  }
  const float bs = block_sum(s, sf);
  const unsigned bg = block_sum_u(ngt, su);
  const unsigned bt = block_sum_u(ntie, su);
  if (threadIdx.x == 0) {
    reinterpret_cast<float*>(ws + PART_OFF)[2 * gridDim.x + blockIdx.x] = bs;
    if (bg) atomicAdd(&ctr[C_NGT], bg);
    if (bt) atomicAdd(&ctr[C_NTIE], bt);
  }
}

// coef[8] (device): [0] value  [1] mode (0 Normal / focal, 1 OHEM mode A, 2 OHEM mode B)  [2] the threshold the gradient compares l
// with (T, v; -1 where every valid pixel is in)  [3] weight where l > threshold  [4] weight where l == threshold  [5] #valid
// [6] #labels outside [0, C) that are not ignore  [7] #{l > threshold} (OHEM)
__global__ __launch_bounds__(64) void seg_finish_kernel(const unsigned* __restrict__ ws, int nblk, int kind, float T, unsigned n_min,
                                                        double n_all, float* __restrict__ coef) {
  const unsigned* ctr = ws + CTR_OFF;
  const float* partial = reinterpret_cast<const float*>(ws + PART_OFF);
  const bool mode_a = kind == KIND_OHEM && ctr[S_MODE_A] == 1u;
  const int which = kind != KIND_OHEM ? 0 : (mode_a ? 1 : 2);
  // single wave: lane-strided sums in block order, then a fixed shuffle tree, in double -> deterministic
  double acc = 0.0;
  for (int i = threadIdx.x; i < nblk; i += 64) acc += (double)partial[(size_t)which * nblk + i];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m);
  if (threadIdx.x == 0) {
    const double nv = (double)ctr[C_VALID];
    float value, mode = 0.f, thr = -1.f, w_gt, w_tie = 0.f, n_in = 0.f;
    if (kind == KIND_NORMAL) {
      value = (float)(acc / n_all);
      w_gt = (float)(1.0 / n_all);
    } else if (kind == KIND_FOCAL) {
      value = (float)(acc / nv);                    // #valid = 0: NaN, as torch
      w_gt = (float)(1.0 / nv);
    } else if (mode_a) {
      const double cnt = (double)ctr[C_GT_T];
      value = (float)(acc / cnt);
      mode = 1.f; thr = T; w_gt = (float)(1.0 / cnt); n_in = (float)cnt;
    } else {
      const float v = __uint_as_float(ctr[S_PREFIX]);
      const double ngt = (double)ctr[C_NGT], ntie = (double)ctr[C_NTIE], k = (double)n_min;
      value = (float)((acc + (k - ngt) * (double)v) / k);
      mode = 2.f; thr = v; w_gt = (float)(1.0 / k); w_tie = (float)((k - ngt) / (ntie * k)); n_in = (float)ngt;
    }
    coef[0] = value; coef[1] = mode; coef[2] = thr; coef[3] = w_gt; coef[4] = w_tie;
    coef[5] = (float)nv; coef[6] = (float)ctr[C_BAD]; coef[7] = n_in;
  }
}

// d value / d o at full resolution, NHWC with the channels padded to CP (pad channels zero).  Reads l_i and lse_i: no max, no sum.
template <bool FOCAL>
__global__ __launch_bounds__(256) void seg_grad_kernel(const float* __restrict__ logits, const long long* __restrict__ label,
                                                       const float* __restrict__ lplane, const float* __restrict__ lseplane,
                                                       const float* __restrict__ coef, const float* __restrict__ upstream,
                                                       float* __restrict__ dfull, float gamma, int B, int IH, int IW, int C, int OH,
                                                       int OW, int ignore, int CP) {
  const size_t total = (size_t)B * OH * OW;
  const float sy = (float)IH / (float)OH, sx = (float)IW / (float)OW;
  const float up = *upstream;
  const float thr = coef[2], w_gt = coef[3] * up, w_tie = coef[4] * up;
  const int nq = CP / 4;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
    const int ox = (int)(i % OW);
    size_t t = i / OW;
    const int oy = (int)(t % OH);
    const int b = (int)(t / OH);
    const long long lab = label[i];
    const bool valid = lab != (long long)ignore && lab >= 0 && lab < (long long)C;
    const float l = lplane[i], lse = lseplane[i];
    float w = 0.f;
    if (valid) w = FOCAL ? w_gt : (l > thr ? w_gt : (l == thr ? w_tie : 0.f));
    float4* drow = reinterpret_cast<float4*>(dfull + i * CP);
    if (w == 0.f) {          // ignored, out of range, or outside OHEM's selection
      for (int q4 = 0; q4 < nq; ++q4) drow[q4] = make_float4(0.f, 0.f, 0.f, 0.f);
      continue;
    }
    int y0, y1, x0, x1; float ly, lx;
    paif::src_index(sy, oy, IH, y0, y1, ly);
    paif::src_index(sx, ox, IW, x0, x1, lx);
    const float hy = 1.f - ly, hx = 1.f - lx;
    const float* p00 = logits + (((size_t)b * IH + y0) * IW + x0) * C;
    const float* p01 = logits + (((size_t)b * IH + y0) * IW + x1) * C;
    const float* p10 = logits + (((size_t)b * IH + y1) * IW + x0) * C;
    const float* p11 = logits + (((size_t)b * IH + y1) * IW + x1) * C;
    float g = w;             // d_c = g * (p_c - delta_c)
    if (FOCAL) {
      // f = -(1-p)^gamma log p:  df/do_c = [gamma (1-p)^(gamma-1) p log p - (1-p)^gamma] (delta_c - p_c)
      const float logp = PAIF_INTERP((int)lab) - lse;
      float q = 0.f;
#pragma unroll 1
      for (int c = 0; c < C; ++c)
        if (c != (int)lab) q += expf(PAIF_INTERP(c) - lse);
      float a = 0.f;         // 1 - p exactly 0: no gradient (torch gives NaN there for 0 < gamma < 1)
      if (q > 0.f) a = (gamma > 0.f ? gamma * powf(q, gamma - 1.f) * expf(logp) * logp : 0.f) - powf(q, gamma);
      g = -w * a;
    }
#pragma unroll 1
    for (int q4 = 0; q4 < nq; ++q4) {
      float d[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int c = q4 * 4 + j;
        const int cc = c < C ? c : C - 1;              // clamped address, the pad channel is zeroed by select
        const float pc = expf(PAIF_INTERP(cc) - lse);
        d[j] = c < C ? g * (pc - (c == (int)lab ? 1.f : 0.f)) : 0.f;
      }
      drow[q4] = make_float4(d[0], d[1], d[2], d[3]);
    }
  }
}

#undef PAIF_INTERP

}  // namespace

extern "C" {

int paif_seg_criterion_blocks(int B, int OH, int OW) {
  if (B <= 0 || OH <= 0 || OW <= 0) return 0;
  return sc_grid((size_t)B * OH * OW);
}

size_t paif_seg_criterion_workspace_words(int B, int OH, int OW) {
  return (size_t)PART_OFF + (size_t)SC_NPART * paif_seg_criterion_blocks(B, OH, OW);
}

int paif_seg_criterion_fwd(const float* logits, const long long* label, float* lplane, float* lseplane, void* workspace, float* coef,
                           int kind, float param, int n_min, int B, int IH, int IW, int C, int OH, int OW, int ignore_index,
                           paif_stream_t stream) {
  PAIF_REQUIRE(logits && label && lplane && lseplane && workspace && coef && B > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0, PAIF_EINVAL,
               "seg_criterion_fwd: bad arguments");
  PAIF_REQUIRE(kind >= KIND_NORMAL && kind <= KIND_OHEM, PAIF_EINVAL, "seg_criterion_fwd: kind %d (0 Normal, 1 focal, 2 OHEM)", kind);
  PAIF_REQUIRE(C > 0 && C <= SC_MAXC, PAIF_ENOSUP, "seg_criterion_fwd: C=%d (max %d)", C, SC_MAXC);
  const size_t total = (size_t)B * OH * OW;
  PAIF_REQUIRE(total < ((size_t)1 << 31), PAIF_ENOSUP, "seg_criterion_fwd: %zu pixels (the counters are 32-bit)", total);
  if (kind == KIND_FOCAL) PAIF_REQUIRE(param >= 0.f, PAIF_EINVAL, "seg_criterion_fwd: gamma %g < 0", (double)param);
  if (kind == KIND_OHEM) {
    PAIF_REQUIRE(param >= 0.f, PAIF_EINVAL, "seg_criterion_fwd: T = -log(thresh) = %g < 0", (double)param);
    PAIF_REQUIRE(n_min >= 1 && (size_t)n_min <= total, PAIF_EINVAL, "seg_criterion_fwd: n_min %d outside [1, %zu]", n_min, total);
  }
  hipStream_t st = paif::as_stream(stream);
  unsigned* ws = static_cast<unsigned*>(workspace);
  const int nblk = sc_grid(total);
  hipError_t e = hipMemsetAsync(ws, 0, (size_t)PART_OFF * sizeof(unsigned), st);
  PAIF_REQUIRE(e == hipSuccess, (int)e, "seg_criterion_fwd: memset failed: %s", hipGetErrorString(e));
#define SC_PIXEL(K) \
  hipLaunchKernelGGL(seg_pixel_kernel<K>, dim3(nblk), dim3(256), 0, st, logits, label, lplane, lseplane, ws, param, B, IH, IW, C, OH, OW, ignore_index)
  if (kind == KIND_NORMAL) SC_PIXEL(KIND_NORMAL);
  else if (kind == KIND_FOCAL) SC_PIXEL(KIND_FOCAL);
  else SC_PIXEL(KIND_OHEM);
#undef SC_PIXEL
  PAIF_LAUNCH_CHECK("seg_criterion_pixel");
  if (kind == KIND_OHEM) {
    const unsigned k = (unsigned)n_min;
    hipLaunchKernelGGL(seg_pick_kernel, dim3(1), dim3(64), 0, st, ws, H0_OFF, H0_BINS, 21, 0, k);
    PAIF_LAUNCH_CHECK("seg_criterion_pick0");
    hipLaunchKernelGGL(seg_hist_kernel, dim3(nblk), dim3(256), 0, st, (const float*)lplane, total, ws, H1_OFF, H1_BINS, 10, 21);
    PAIF_LAUNCH_CHECK("seg_criterion_hist1");
    hipLaunchKernelGGL(seg_pick_kernel, dim3(1), dim3(64), 0, st, ws, H1_OFF, H1_BINS, 10, 1, k);
    PAIF_LAUNCH_CHECK("seg_criterion_pick1");
    hipLaunchKernelGGL(seg_hist_kernel, dim3(nblk), dim3(256), 0, st, (const float*)lplane, total, ws, H2_OFF, H2_BINS, 0, 10);
    PAIF_LAUNCH_CHECK("seg_criterion_hist2");
    hipLaunchKernelGGL(seg_pick_kernel, dim3(1), dim3(64), 0, st, ws, H2_OFF, H2_BINS, 0, 2, k);
    PAIF_LAUNCH_CHECK("seg_criterion_pick2");
    hipLaunchKernelGGL(seg_select_sum_kernel, dim3(nblk), dim3(256), 0, st, (const float*)lplane, total, ws);
    PAIF_LAUNCH_CHECK("seg_criterion_select_sum");
  }
  hipLaunchKernelGGL(seg_finish_kernel, dim3(1), dim3(64), 0, st, (const unsigned*)ws, nblk, kind, param, (unsigned)(n_min > 0 ? n_min : 1),
                     (double)total, coef);
  PAIF_LAUNCH_CHECK("seg_criterion_finish");
  return 0;
}

int paif_seg_criterion_bwd(const float* logits, const long long* label, const float* lplane, const float* lseplane, const float* coef,
                           const float* upstream, float* dfull, int kind, float gamma, int B, int IH, int IW, int C, int OH, int OW,
                           int ignore_index, int CP, paif_stream_t stream) {
  PAIF_REQUIRE(logits && label && lplane && lseplane && coef && upstream && dfull && B > 0 && IH > 0 && IW > 0 && OH > 0 && OW > 0,
               PAIF_EINVAL, "seg_criterion_bwd: bad arguments");
  PAIF_REQUIRE(kind >= KIND_NORMAL && kind <= KIND_OHEM, PAIF_EINVAL, "seg_criterion_bwd: kind %d", kind);
  PAIF_REQUIRE(C > 0 && C <= SC_MAXC && CP >= C && CP % 4 == 0, PAIF_ENOSUP, "seg_criterion_bwd: C=%d CP=%d", C, CP);
  PAIF_REQUIRE((size_t)B * OH * OW < ((size_t)1 << 31), PAIF_ENOSUP, "seg_criterion_bwd: too many pixels");
  if (kind == KIND_FOCAL) PAIF_REQUIRE(gamma >= 0.f, PAIF_EINVAL, "seg_criterion_bwd: gamma %g < 0", (double)gamma);
  const int nblk = sc_grid((size_t)B * OH * OW);
  hipStream_t st = paif::as_stream(stream);
  if (kind == KIND_FOCAL)
    hipLaunchKernelGGL(seg_grad_kernel<true>, dim3(nblk), dim3(256), 0, st, logits, label, lplane, lseplane, coef, upstream, dfull, gamma, B,
                       IH, IW, C, OH, OW, ignore_index, CP);
  else
    hipLaunchKernelGGL(seg_grad_kernel<false>, dim3(nblk), dim3(256), 0, st, logits, label, lplane, lseplane, coef, upstream, dfull, 0.f, B,
                       IH, IW, C, OH, OW, ignore_index, CP);
  PAIF_LAUNCH_CHECK("seg_criterion_bwd");
  return 0;
}

}  // extern "C"
