// Flash self-attention of the SelAttention primitive (operations_m.py:31-61, Attention inside SelfPath :90-112):
//   out[b, n, 64 hd + :] = softmax_j( q[b,n,hd,:] . k[b,j,hd,:] * 64^-0.5 ) @ v[b,j,hd,:]      over ALL N = H*W keys,
// q | k | v read IN PLACE from the [B, N, 192 heads] tensor the to_qkv GEMM writes (row stride 192 heads, column blocks at
// 0 / 64 heads / 128 heads, head hd at 64 hd in each).  Nothing of size N^2 exists anywhere; all element indices are 64-bit.
//
// Forward: fp16 operand pairs (hi + lo, three products on v_mfma_f32_32x32x16_f16, fp32 accumulate; paif::splitN<2, 1>).  K and V
// are split ONCE per call by self_attention_pack_kernel into a workspace of 64-key tile images that are byte for byte what the main
// kernel wants in LDS:
//   K part  [64 keys][hi 64 dims | lo 64 dims] fp16, 16-byte chunks XOR-swizzled with key & 7   (A operand of S^T = K . Q^T)
//   V part  [64 dims][hi 64 slots | lo 64 slots | 16 B pad] fp16: V^T, the key slots of each 32-key half permuted so that the 8 slots a
//           lane half feeds to a K=16 step are the keys its softmax registers hold (as csrc/attention.hip)   (A operand of O^T += V^T . P^T)
// so a tile load is a linear 16-byte copy.  The main kernel (8 waves x 32 queries) double-buffers the images: the global loads of
// tile t+1 are issued before the MFMAs of tile t and land in the other buffer after them, one barrier per 64 keys.
// Orientation as csrc/attention.hip ("key on the register, query on the lane").  P = exp(s - m) is carried scaled by 2^10 (in P, l
// and O alike, so it cancels in O / l and is subtracted from lse): entries down to 2^-24 of the row maximum keep a normal fp16 hi piece.
// The softmax runs in the log2 domain (one fma + one v_exp_f32 per score) and is the bound of the kernel: vector issue, not the MFMAs.
//
// Reverse: P is recomputed from q, k and lse.  Two main kernels from one body on the exact fp32 MFMA (v_mfma_f32_32x32x2_f32): the owner
// rows (32 per wave) sit in registers, the swept rows stream through a double-buffered LDS tile of 32 rows:
//   OWNQ = true : owns queries, sweeps keys:     S^T = K Q^T, dP^T = V dO^T, A^T += K^T (P dP)^T, M^T += K^T P^T, L = sum P, d = sum P dP
//                 -> delta = d / L, lse' = lse + log L, dQ = scale (A - delta M) / L
//   OWNQ = false: owns keys,    sweeps queries:  S = Q K^T,  dP = dO V^T,  P = exp(s - lse'),  dS = P (dP - delta),  dK^T += Q^T dS, dV^T += dO^T P
// delta is NOT rowsum(dO . O): the forward's O and lse carry its fp16-pair rounding, and with scores of +-60 and keys of magnitude 60 a
// delta that is inconsistent with the recomputed P by 3e-5 shows up times scale * |sum_j P k_j| = 7.5 in dQ (measured: 2.5e-4 against a
// bound of 6.5e-5).  So the query-owning kernel forms L and delta from the very P it multiplies with, renormalises lse by log L, and
// hands both to the key-owning kernel, which runs after it.  Eight products instead of the five of an atomic-add backward, accepted for:
// no atomics, no workgroup waits on another, no partial slabs -- every output element has one writer and a fixed summation order.
#include "paif_common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
using paif::bf16x8_t;
using paif::mfma_pieces;
using paif::splitN;

constexpr int D = 64;
constexpr int KT = 64;                          // keys per tile image
constexpr int KREC = D * 2 * 2;                 // 256 B: hi | lo of one key
constexpr int VREC = KT * 2 * 2 + 16;           // 272 B: hi slots | lo slots | pad of one dim
constexpr int K_BYTES = KT * KREC;              // 16,384
constexpr int V_BYTES = D * VREC;               // 17,408
constexpr int TILE_BYTES = K_BYTES + V_BYTES;   // 33,792
constexpr int TILE_CHUNKS = TILE_BYTES / 16;    // 2,112
constexpr int FWD_NT = 512;
constexpr int FWD_FULL = TILE_CHUNKS / FWD_NT;                 // 4 chunks per thread in flight ...
constexpr int FWD_TAIL = TILE_CHUNKS - FWD_FULL * FWD_NT;      // ... and a fifth in the first 64 threads
constexpr float P_SHIFT_LOG2 = 10.0f;           // P is carried times 2^10
constexpr float LOG2E = 1.4426950408889634f, LN2 = 0.6931471805599453f;

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

// P (eight values in [0, 2^10]) -> fp16 hi | lo: hi by ONE packed convert per pair (round toward zero: the remainder is exact and
// non-negative), lo = rn(remainder); 22 significant bits as paif::splitN<2, 1>, four vector instructions per value instead of five
__device__ __forceinline__ void split_p8(const float (&v)[8], bf16x8_t (&pc)[2]) {
  u32x4 hi, lo;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const auto h2 = __builtin_amdgcn_cvt_pkrtz(v[2 * i], v[2 * i + 1]);
    const f16x2 l2 = {(_Float16)(v[2 * i] - (float)h2[0]), (_Float16)(v[2 * i + 1] - (float)h2[1])};
    hi[i] = __builtin_bit_cast(unsigned, h2);
    lo[i] = __builtin_bit_cast(unsigned, l2);
  }
  pc[0] = __builtin_bit_cast(bf16x8_t, hi);
  pc[1] = __builtin_bit_cast(bf16x8_t, lo);
}

struct FullArgs {
  const float* qkv; float* out; float* lse; char* ws;
  int B, N, heads, ntiles;
  float scale;
};

// one workgroup per (tile, head, batch): K and V of 64 keys -> one tile image; keys past N are zeros
__global__ __launch_bounds__(256) void self_attention_pack_kernel(FullArgs a) {
  const int tid = threadIdx.x, tile = blockIdx.x, hd = blockIdx.y, b = blockIdx.z;
  const long ld = 192L * a.heads;
  char* img = a.ws + ((size_t)((size_t)b * a.heads + hd) * a.ntiles + tile) * TILE_BYTES;
  const float* kb = a.qkv + (long)b * a.N * ld + 64L * a.heads + 64L * hd;
  const float* vb = kb + 64L * a.heads;
  for (int idx = tid; idx < KT * (D / 8); idx += 256) {
    const int key = idx >> 3, c = idx & 7;
    const long gk = (long)tile * KT + key;
    float k8[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (gk < a.N) {
      const float4 k0 = *reinterpret_cast<const float4*>(kb + gk * ld + c * 8);
      const float4 k1 = *reinterpret_cast<const float4*>(kb + gk * ld + c * 8 + 4);
      k8[0] = k0.x; k8[1] = k0.y; k8[2] = k0.z; k8[3] = k0.w; k8[4] = k1.x; k8[5] = k1.y; k8[6] = k1.z; k8[7] = k1.w;
    }
    bf16x8_t pc[2];
    splitN<2, 1>(k8, pc);
#pragma unroll
    for (int q = 0; q < 2; ++q) *reinterpret_cast<bf16x8_t*>(img + key * KREC + q * (D * 2) + ((c ^ (key & 7)) << 4)) = pc[q];
  }
  for (int idx = tid; idx < KT * (D / 4); idx += 256) {
    const int key = idx >> 4, q4 = idx & 15;
    const long gk = (long)tile * KT + key;
    float4 vv = make_float4(0.f, 0.f, 0.f, 0.f);
    if (gk < a.N) vv = *reinterpret_cast<const float4*>(vb + gk * ld + q4 * 4);
    const int sub = key >> 5, kk = key & 31;
    const int hh = (kk >> 2) & 1, r = (kk & 3) + 4 * (kk >> 3);
    const int slot = sub * 32 + (r >> 3) * 16 + 8 * hh + (r & 7);
    const float vf[4] = {vv.x, vv.y, vv.z, vv.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int dim = q4 * 4 + i;
      float rr = vf[i];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        float back;
        *reinterpret_cast<__bf16*>(img + K_BYTES + dim * VREC + q * (KT * 2) + slot * 2) = paif::piece16<1>(rr, back);
        rr -= back;
      }
    }
  }
}

__global__ __launch_bounds__(FWD_NT) void self_attention_fwd_kernel(FullArgs a) {
  extern __shared__ __align__(16) char lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
  const int hd = blockIdx.y, b = blockIdx.z, N = a.N;
  const long ld = 192L * a.heads;
  const int q0 = blockIdx.x * (FWD_NT / 2) + wave * 32;
  const bool wave_live = q0 < N;          // dead waves still copy tiles and hit the barriers
  const int qi = min(q0 + p, N - 1);      // lanes past N compute a duplicate and do not store
  const float* qrow = a.qkv + ((long)b * N + qi) * ld + 64L * hd;
  bf16x8_t qp[4][2];
#pragma unroll
  for (int o = 0; o < 4; ++o) {
    const float4 q0v = *reinterpret_cast<const float4*>(qrow + 16 * o + 8 * h);
    const float4 q1v = *reinterpret_cast<const float4*>(qrow + 16 * o + 8 * h + 4);
    const float q8[8] = {q0v.x, q0v.y, q0v.z, q0v.w, q1v.x, q1v.y, q1v.z, q1v.w};
    splitN<2, 1>(q8, qp[o]);
  }
  f32x16 oacc[2];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) oacc[t][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float sc2 = a.scale * LOG2E;

  const u32x4* src = reinterpret_cast<const u32x4*>(a.ws + (size_t)((size_t)b * a.heads + hd) * a.ntiles * TILE_BYTES);
  for (int i = tid; i < TILE_CHUNKS; i += FWD_NT) reinterpret_cast<u32x4*>(lds)[i] = src[i];
  __syncthreads();
  // the next tile's image on its way through registers: 4 full rounds of 512 chunks + 64 chunks.  Named native vectors, not an array:
  // hipcc kept an array of HIP's uint4 in scratch, which put a vmcnt(0) in front of the MFMAs
  u32x4 pre0 = 0, pre1 = 0, pre2 = 0, pre3 = 0, pre_tail = 0;
  static_assert(FWD_FULL == 4, "four named prefetch registers");

  for (int t = 0; t < a.ntiles; ++t) {
    const char* cur = lds + (t & 1) * TILE_BYTES;
    const bool more = t + 1 < a.ntiles;
    if (more) {
      const u32x4* nxt = src + (size_t)(t + 1) * TILE_CHUNKS + tid;
      pre0 = nxt[0];
      pre1 = nxt[FWD_NT];
      pre2 = nxt[2 * FWD_NT];
      pre3 = nxt[3 * FWD_NT];
      if (tid < FWD_TAIL) pre_tail = nxt[4 * FWD_NT];
    }
    if (wave_live) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int kb = t * KT + s * 32;
        if (kb >= N) break;
        // ---- S^T tile = K_tile . Q^T ----
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.f;
        const char* krow = cur + (s * 32 + p) * KREC;
        const int sw = p & 7;
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int c = 2 * o + h;
          bf16x8_t kp[2];
#pragma unroll
          for (int q = 0; q < 2; ++q) kp[q] = *reinterpret_cast<const bf16x8_t*>(krow + q * (D * 2) + ((c ^ sw) << 4));
          mfma_pieces<2, 1>(st, kp, qp[o]);
        }
        // ---- online softmax in the log2 domain (register r <-> key kb + (r&3) + 8(r>>2) + 4h): m_run = max of s * c, c = scale * log2 e;
        //      p = 2^(s c - m + 10) is one fma and one v_exp_f32 per score; the softmax is vector-issue bound, so every instruction counts ----
        if (kb + 32 > N) {                             // the ragged half tile (wave-uniform): keys past N get -inf, i.e. p = 0
#pragma unroll
          for (int r = 0; r < 16; ++r)
            if (kb + (r & 3) + 8 * (r >> 2) + 4 * h >= N) st[r] = -INFINITY;
        }
        float mt = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) mt = fmaxf(mt, st[r]);
        mt = fmaxf(mt, __shfl_xor(mt, 32));
        const float m_new = fmaxf(m_run, mt * sc2);    // finite: kb < N, so the half tile has a valid key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);       // 2^-inf = 0 on the first tile
        const float off = P_SHIFT_LOG2 - m_new;
        float ls = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          st[r] = __builtin_amdgcn_exp2f(fmaf(st[r], sc2, off));         // masked keys: 2^-inf = 0
          ls += st[r];
        }
        ls += __shfl_xor(ls, 32);
        l_run = l_run * alpha + ls;
        m_run = m_new;
        if (__any(alpha != 1.f)) {                     // (wave-uniform) the running maximum rarely moves after the first tiles
#pragma unroll
          for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        }
        // ---- O^T += V_tile^T . P^T ----
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
          float p8[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) p8[i] = st[8 * s2 + i];
          bf16x8_t pp[2];
          split_p8(p8, pp);
          const int soff = (s * 32 + s2 * 16 + 8 * h) * 2;
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) {
            const int dim = 32 * dt + p;
            bf16x8_t vp[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) vp[q] = *reinterpret_cast<const bf16x8_t*>(cur + K_BYTES + dim * VREC + q * (KT * 2) + soff);
            mfma_pieces<2, 1>(oacc[dt], vp, pp);
          }
        }
      }
    }
    if (more) {
      u32x4* dst = reinterpret_cast<u32x4*>(lds + ((t + 1) & 1) * TILE_BYTES) + tid;
      dst[0] = pre0;
      dst[FWD_NT] = pre1;
      dst[2 * FWD_NT] = pre2;
      dst[3 * FWD_NT] = pre3;
      if (tid < FWD_TAIL) dst[4 * FWD_NT] = pre_tail;
    }
    __syncthreads();
  }

  if (!wave_live || q0 + p >= N) return;
  if (a.lse && h == 0) a.lse[((long)b * a.heads + hd) * N + q0 + p] = (m_run - P_SHIFT_LOG2) * LN2 + logf(l_run);
  const float inv = 1.0f / l_run;
  float* orow = a.out + ((long)b * N + q0 + p) * (64L * a.heads) + 64L * hd;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4*>(orow + 32 * dt + 8 * g + 4 * h) =
          make_float4(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv, oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
}

// ---------------------------------------------------------------------------------------------------------------------------------
struct BwdArgs {
  const float* qkv; const float* dout; const float* lse; float* lse2; float* delta; float* dqkv;     // lse2, delta: [B, heads, N] workspace
  int B, N, heads;
  float scale;
};

constexpr int BWD_NT = 512;

template <bool OWNQ>
__device__ __forceinline__ void self_attention_bwd_body(const BwdArgs& a) {
  __shared__ __align__(16) float Y1s[2][32 * D];      // swept rows, 16-byte chunks XOR-swizzled with row & 15
  __shared__ __align__(16) float Y2s[2][32 * D];
  __shared__ float Ls[2][32], Ds[2][32];              // lse / delta of the swept queries (OWNQ = false)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, p = lane & 31;
  const int hd = blockIdx.y, b = blockIdx.z, N = a.N;
  const long ld = 192L * a.heads, ldo = 64L * a.heads;
  const int r0 = blockIdx.x * (BWD_NT / 2) + wave * 32;
  const bool wave_live = r0 < N;
  const int ri = min(r0 + p, N - 1);
  const float* qb = a.qkv + (long)b * N * ld + 64L * hd;
  const float* kb = qb + 64L * a.heads;
  const float* vb = kb + 64L * a.heads;
  const float* gb = a.dout + (long)b * N * ldo + 64L * hd;
  const long stat0 = ((long)b * a.heads + hd) * N;
  const float* lseb = OWNQ ? a.lse + stat0 : a.lse2 + stat0;      // the key-owning kernel reads what the query-owning one left
  const float* delb = a.delta + stat0;

  // owner rows in registers; swept rows from y1 / y2
  const float* x1row = OWNQ ? qb + (long)ri * ld : kb + (long)ri * ld;
  const float* x2row = OWNQ ? gb + (long)ri * ldo : vb + (long)ri * ld;
  const float* y1 = OWNQ ? kb : qb;
  const float* y2 = OWNQ ? vb : gb;
  const long ldy2 = OWNQ ? ld : ldo;
  float4 x1f[8], x2f[8];
#pragma unroll
  for (int o = 0; o < 8; ++o) {
    x1f[o] = *reinterpret_cast<const float4*>(x1row + 8 * o + 4 * h);
    x2f[o] = *reinterpret_cast<const float4*>(x2row + 8 * o + 4 * h);
  }
  const float lse_o = OWNQ ? lseb[ri] : 0.f;
  float l_sum = 0.f, d_sum = 0.f;   // OWNQ: sum_j P, sum_j P dP of this lane's query over the keys of its half

  f32x16 acc1[2], acc2[2];       // OWNQ: acc1 = A^T, acc2 = M^T;  else acc1 = dK^T, acc2 = dV^T
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc1[t][r] = 0.f; acc2[t][r] = 0.f; }

  const int srow = tid >> 4, sc = tid & 15;
  const int soff = srow * D + ((sc ^ (srow & 15)) << 2);
  const int ntile = (N + 31) / 32;
  float4 v1, v2;
  float ll = 0.f, dd = 0.f;
  auto fetch = [&](int t) {
    const long gr = (long)t * 32 + srow;
    v1 = make_float4(0.f, 0.f, 0.f, 0.f);
    v2 = v1;
    if (gr < N) {
      v1 = *reinterpret_cast<const float4*>(y1 + gr * ld + sc * 4);
      v2 = *reinterpret_cast<const float4*>(y2 + gr * ldy2 + sc * 4);
    }
    if (!OWNQ && tid < 32) {
      const long g = (long)t * 32 + tid;
      ll = g < N ? lseb[g] : 0.f;
      dd = g < N ? delb[g] : 0.f;
    }
  };
  auto park = [&](int buf) {
    *reinterpret_cast<float4*>(&Y1s[buf][soff]) = v1;
    *reinterpret_cast<float4*>(&Y2s[buf][soff]) = v2;
    if (!OWNQ && tid < 32) { Ls[buf][tid] = ll; Ds[buf][tid] = dd; }
  };
  fetch(0);
  park(0);
  __syncthreads();

  for (int t = 0; t < ntile; ++t) {
    const int cur = t & 1;
    const bool more = t + 1 < ntile;
    if (more) fetch(t + 1);
    if (wave_live) {
      f32x16 st, dp;
#pragma unroll
      for (int r = 0; r < 16; ++r) { st[r] = 0.f; dp[r] = 0.f; }
      const float* y1r = &Y1s[cur][p * D];
      const float* y2r = &Y2s[cur][p * D];
      const int sw = p & 15;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        const float4 kf = *reinterpret_cast<const float4*>(y1r + (((2 * o + h) ^ sw) << 2));
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.x, x1f[o].x, st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.y, x1f[o].y, st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.z, x1f[o].z, st, 0, 0, 0);
        st = __builtin_amdgcn_mfma_f32_32x32x2f32(kf.w, x1f[o].w, st, 0, 0, 0);
        const float4 vf = *reinterpret_cast<const float4*>(y2r + (((2 * o + h) ^ sw) << 2));
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.x, x2f[o].x, dp, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.y, x2f[o].y, dp, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.z, x2f[o].z, dp, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x2f32(vf.w, x2f[o].w, dp, 0, 0, 0);
      }
      // register r of half h <-> swept row (r&3) + 8(r>>2) + 4h; P = exp(s - lse) of the QUERY, 0 for swept rows past N
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
        const float l = OWNQ ? lse_o : Ls[cur][row];
        const float pr = (t * 32 + row < N) ? expf(st[r] * a.scale - l) : 0.f;
        st[r] = pr;
        if (OWNQ) {
          dp[r] = pr * dp[r];
          l_sum += pr;
          d_sum += dp[r];
        } else {
          dp[r] = pr * (dp[r] - Ds[cur][row]);
        }
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = (r & 3) + 8 * (r >> 2) + 4 * h;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
          const int dim = 32 * dt + p;
          const int off = row * D + (((dim >> 2) ^ (row & 15)) << 2) + (dim & 3);
          acc1[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(Y1s[cur][off], dp[r], acc1[dt], 0, 0, 0);
          acc2[dt] = __builtin_amdgcn_mfma_f32_32x32x2f32(OWNQ ? Y1s[cur][off] : Y2s[cur][off], st[r], acc2[dt], 0, 0, 0);
        }
      }
    }
    if (more) park(cur ^ 1);
    __syncthreads();
  }

  if (!wave_live) return;
  float s1 = a.scale, s2 = 1.f;       // out = acc1 * s1 - acc2 * s2  (OWNQ);  acc1 * s1 and acc2 (else)
  if (OWNQ) {
    l_sum += __shfl_xor(l_sum, 32);   // the two lane halves hold the two halves of the query's keys
    d_sum += __shfl_xor(d_sum, 32);
    const float inv = 1.0f / l_sum, delta = d_sum * inv;
    s1 = a.scale * inv;
    s2 = a.scale * inv * delta;
    if (h == 0 && r0 + p < N) {
      a.delta[stat0 + r0 + p] = delta;
      a.lse2[stat0 + r0 + p] = lse_o + logf(l_sum);
    }
  }
  if (r0 + p >= N) return;
  // lane (h, j) holds dims 32 dt + 8 g + 4 h + (0..3) of owner row j
  float* o1 = a.dqkv + ((long)b * N + r0 + p) * ld + 64L * hd + (OWNQ ? 0L : 64L * a.heads);
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (OWNQ) {
        *reinterpret_cast<float4*>(o1 + 32 * dt + 8 * g + 4 * h) =
            make_float4(acc1[dt][4 * g] * s1 - acc2[dt][4 * g] * s2, acc1[dt][4 * g + 1] * s1 - acc2[dt][4 * g + 1] * s2,
                        acc1[dt][4 * g + 2] * s1 - acc2[dt][4 * g + 2] * s2, acc1[dt][4 * g + 3] * s1 - acc2[dt][4 * g + 3] * s2);
      } else {
        *reinterpret_cast<float4*>(o1 + 32 * dt + 8 * g + 4 * h) =
            make_float4(acc1[dt][4 * g] * s1, acc1[dt][4 * g + 1] * s1, acc1[dt][4 * g + 2] * s1, acc1[dt][4 * g + 3] * s1);
        *reinterpret_cast<float4*>(o1 + 64L * a.heads + 32 * dt + 8 * g + 4 * h) =
            make_float4(acc2[dt][4 * g], acc2[dt][4 * g + 1], acc2[dt][4 * g + 2], acc2[dt][4 * g + 3]);
      }
    }
}

__global__ __launch_bounds__(BWD_NT) void self_attention_bwd_dq_kernel(BwdArgs a) { self_attention_bwd_body<true>(a); }
__global__ __launch_bounds__(BWD_NT) void self_attention_bwd_dkv_kernel(BwdArgs a) { self_attention_bwd_body<false>(a); }

int check_shape(const char* what, int B, int N, int heads) {
  PAIF_REQUIRE(B > 0 && N > 0 && heads > 0, PAIF_EINVAL, "%s: B=%d N=%d heads=%d", what, B, N, heads);
  PAIF_REQUIRE(B <= 65535 && heads <= 65535, PAIF_ENOSUP, "%s: B=%d / heads=%d exceed the launch grid (65535) -- not built", what, B, heads);
  PAIF_REQUIRE(N <= (1 << 30), PAIF_ENOSUP, "%s: N=%d tokens (> 2^30) not built", what, N);
  return 0;
}

}  // namespace

extern "C" size_t paif_self_attention_workspace_bytes(int B, int N, int heads) {
  if (B <= 0 || N <= 0 || heads <= 0 || B > 65535 || heads > 65535 || N > (1 << 30)) return 0;
  return (size_t)B * heads * ((N + KT - 1) / KT) * TILE_BYTES;
}

extern "C" int paif_self_attention_fwd(const float* qkv, float* out, float* lse, void* workspace, int B, int N, int heads,
                                       paif_stream_t stream) {
  PAIF_REQUIRE(qkv && out && workspace, PAIF_EINVAL, "self_attention: null pointer");
  if (int e = check_shape("self_attention", B, N, heads)) return e;
  FullArgs a;
  a.qkv = qkv; a.out = out; a.lse = lse; a.ws = static_cast<char*>(workspace);
  a.B = B; a.N = N; a.heads = heads; a.ntiles = (N + KT - 1) / KT;
  a.scale = 0.125f;
  hipStream_t st = paif::as_stream(stream);
  hipLaunchKernelGGL(self_attention_pack_kernel, dim3(a.ntiles, heads, B), dim3(256), 0, st, a);
  PAIF_LAUNCH_CHECK("self_attention(pack)");
  const int lds_bytes = 2 * TILE_BYTES;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&self_attention_fwd_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  if (e != hipSuccess) {
    paif::set_error("self_attention: cannot raise dynamic LDS to %d: %s", lds_bytes, hipGetErrorString(e));
    return (int)e;
  }
  hipLaunchKernelGGL(self_attention_fwd_kernel, dim3((N + FWD_NT / 2 - 1) / (FWD_NT / 2), heads, B), dim3(FWD_NT), lds_bytes, st, a);
  PAIF_LAUNCH_CHECK("self_attention");
  return 0;
}

extern "C" size_t paif_self_attention_bwd_workspace_bytes(int B, int N, int heads) {
  if (B <= 0 || N <= 0 || heads <= 0 || B > 65535 || heads > 65535 || N > (1 << 30)) return 0;
  return (size_t)2 * B * heads * N * sizeof(float);      // lse' | delta
}

extern "C" int paif_self_attention_bwd_input(const float* qkv, const float* out, const float* dout, const float* lse, float* dqkv,
                                             void* workspace, int B, int N, int heads, paif_stream_t stream) {
  (void)out;   // not read: delta is formed from the recomputed P (see the head of this file), not from rowsum(dout * out)
  PAIF_REQUIRE(qkv && dout && lse && dqkv && workspace, PAIF_EINVAL, "self_attention_bwd: null pointer");
  if (int e = check_shape("self_attention_bwd", B, N, heads)) return e;
  BwdArgs a;
  a.qkv = qkv; a.dout = dout; a.lse = lse; a.dqkv = dqkv;
  a.lse2 = static_cast<float*>(workspace);
  a.delta = a.lse2 + (size_t)B * heads * N;
  a.B = B; a.N = N; a.heads = heads; a.scale = 0.125f;
  hipStream_t st = paif::as_stream(stream);
  const dim3 grid((N + BWD_NT / 2 - 1) / (BWD_NT / 2), heads, B);
  hipLaunchKernelGGL(self_attention_bwd_dq_kernel, grid, dim3(BWD_NT), 0, st, a);       // writes lse', delta ...
  PAIF_LAUNCH_CHECK("self_attention_bwd(dq)");
  hipLaunchKernelGGL(self_attention_bwd_dkv_kernel, grid, dim3(BWD_NT), 0, st, a);      // ... which this one reads (stream order)
  PAIF_LAUNCH_CHECK("self_attention_bwd(dkv)");
  return 0;
}
