// ECA block, conv2 = 3x3 dilation-1 32 -> 32 over PReLU(r) (fp16 NHWC-32 map, plain fp16 weights), run TWICE on the row-streaming LDS-DMA
// body of conv_rows.h (halo 1) so that its output map is never stored: the POOL pass writes only the per-tile channel sums the gate is
// made of, the GATED pass recomputes the conv and writes PReLU(fp16(o) * gate + r).  Replaces conv_mfma_bf16x3<3, 1, false, 14> +
// eca_apply_kernel<2> on large fp16 maps (785 MB -> 472 MB per block).  What is this kernel's own:
//   * a chain is (image, 32-column strip); runs are whole 8-row tiles (paif_conv2d_blocks numbering), so one wave owns every pool partial
//     it writes;
//   * INPUT PReLU ONCE PER ROW PIECE: when a piece has landed the wave rewrites it in place (3 x 16 B per lane, prelu_h2 below: the bits
//     of conv_mfma_split_body's staging, fp16 -> fp32, v >= 0 ? v : slope * v, round to nearest even -> fp16) before its first use as an
//     operand, through the hooks of conv_row(): in the shadow of the row's first six MFMAs; a piece feeds 9 fragment reads.  The GATED
//     pass takes r (un-activated) from the piece BEFORE the rewrite, in the store layout, one row ahead of its use (two register sets);
//   * the pool's cross-lane sums are the one LDS access that is not inline asm: the compiler waits for its own;
//   * arithmetic as conv_mfma_split_body<3, 1, false, 14> runs it, one MFMA per product.  POOL: epilogue_lds_n's summation tree (rows
//     2w, 2w + 1 of a tile form group w; lane (q, j) chains pixels it * 8 + j, it = 0..7, from 0.f; butterfly over j;
//     ((g0 + g1) + g2) + g3).  GATED: eca_apply_kernel<2> on fp16(acc).  Same operations in the same order on every element, so the
//     same bits as the three launches replaced.
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "conv_eca_rows.h"
#include "conv_rows.h"

namespace paif_eca_rows {
namespace {

using namespace paif_rows;
typedef Ring<1> R;
constexpr int RW = R::RW, DPS = R::DPS, SLOT = R::SLOT, NSLOT = R::NSLOT, PF = R::PF, WAVES = R::WAVES;
constexpr int TR = 8;                         // rows of a pool tile
constexpr int MIN_RUN = MIN_RUN_ROWS / TR;    // tiles per wave at least
constexpr int N_ROW = PF * DPS;               // younger loads behind the DMAs of row t + 2 at the wait of step t

#ifndef ER_LD_AUX_POOL
#define ER_LD_AUX_POOL 0     // cache policy of the POOL pass's LDS-DMA loads: 0 = default (the GATED pass re-reads the map), 2 = streaming (nt)
#endif
#ifndef ER_LD_AUX_GATED
#define ER_LD_AUX_GATED 2    // ... of the GATED pass's: the last reader of r
#endif
#ifndef ER_ST_AUX
#define ER_ST_AUX 0          // cache policy of the output stores (conv_h16_dma_1x1 and conv3x3_h16_dma_rows measured default best)
#endif

// The input PReLU on stored fp16 values: the bits of f32_to_f16x4(prelu_f(float(x), slope)), the staging of conv_mfma_split_body, in 7
// instructions per PAIR instead of the 11 of compare-and-select in fp32 (this rewrite shares the SIMD with the row's first six MFMAs):
//   y = fp16(fp32(x) * slope) for both halves, whatever their sign: the fp32 product rounded to fp32, then to nearest even in fp16
//       (v_fma_mixlo / mixhi_f16 do NOT give these bits: 103 of 63,490 inputs differ at slope 0.1);
//   x >= 0 ? x : y by the bits of x: the halves above 0x8000 (negative and not -0) have the sign set after a saturating `- 1`; +-0,
//       positive values and +NaN keep x.  Proved over all 65,536 patterns by tests/test_eca_rows_gpu.py.
__device__ __forceinline__ unsigned prelu_h2(unsigned x, float slope) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 f = __builtin_convertvector(__builtin_bit_cast(paif::f16x2_t, x), f32x2) * slope;
  const unsigned y = __builtin_bit_cast(unsigned, __builtin_convertvector(f, paif::f16x2_t));
  // (as inline asm: written in C++, hipcc turns the three packed operations back into a compare and a select per half)
  unsigned t, m, r;
  asm("v_pk_sub_u16 %0, %1, %2 clamp" : "=v"(t) : "v"(x), "v"(0x00010001u));
  asm("v_pk_ashrrev_i16 %0, %1, %2" : "=v"(m) : "v"(0x000f000fu), "v"(t));      // 0xffff where the half takes y
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(y), "v"(x));            // (m & y) | (~m & x)
  return r;
}
__device__ __forceinline__ u32x4 prelu_h8(u32x4 v, float slope) {
  const unsigned a = v.x, b = v.y, c = v.z, d = v.w;
  const u32x4 o = {prelu_h2(a, slope), prelu_h2(b, slope), prelu_h2(c, slope), prelu_h2(d, slope)};
  return o;
}

// total = B * SX * TY tiles (SX strips of 32 columns, TY tiles of 8 rows) in the order (image, strip, tile row); wave g owns
// [g * run, (g + 1) * run) and splits it at chain boundaries.
template <int MODE>
__global__ __launch_bounds__(WAVES * 64, 2) void eca_conv2_rows(Args a, int total, int SX, int TY, int run) {
  constexpr int LD_AUX = MODE == POOL ? ER_LD_AUX_POOL : ER_LD_AUX_GATED;
  __shared__ __attribute__((aligned(16))) unsigned char smem[R::LDS_BYTES];
  asm volatile("" ::"v"((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem) : "memory");   // only asm touches it

  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = l & 31, hh = l >> 5;
  const int gw = blockIdx.x * WAVES + w;
  int pos = gw * run;
  const int end = min(total, pos + run);
  if (pos >= end) return;                      // (no barrier anywhere: a wave may leave on its own)
  const int H = a.H, W = a.W;

  const int map_bytes = a.B * H * W * 64;
  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.r), 0, map_bytes, RSRC_W3);
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(MODE == POOL ? (void*)a.partial : a.out, 0,
                                                                          MODE == POOL ? a.B * TY * SX * 128 : map_bytes, RSRC_W3);

  u32x4 bw[9][2];
  ROWS_LOAD_BW(bw, a.wpk, l)
#pragma unroll
  for (int tap = 0; tap < 9; ++tap) asm volatile("" : "+v"(bw[tap][0]), "+v"(bw[tap][1]));   // waited for HERE, not inside the row loop
  float in_slope = *a.in_prelu;
  float slope = MODE == GATED ? *a.prelu : 0.f;
  asm volatile("" : "+v"(in_slope), "+v"(slope));

  // ---- geometry of this lane ----
  int d_col[DPS];
  unsigned d_rel[DPS];
  ROWS_DMA_GEOMETRY(DPS, l, d_col, d_rel)
  const unsigned lds_w = (unsigned)(w * R::WAVE_LDS);                                      // this wave's ring; its park buffer behind it
  unsigned a_rd[3][2];
  ROWS_A_ADDRS(1, lds_w, p, hh, a_rd)
  const unsigned a_rw = lds_w + (unsigned)l * 16u;                                         // the in-place rewrite: chunk 64 i + l, + i * 1024
  const unsigned a_pw = ROWS_PARK_WR_ADDR(lds_w + NSLOT * SLOT, p, hh);
  // park re-read.  POOL: virtual lane (j = l >> 3, q = l & 7) of epilogue_lds_n, pixel it * 8 + j, channel quad q (+ it * 1024).
  // otherwise the store layout
  const unsigned a_pr = MODE == POOL ? lds_w + NSLOT * SLOT + (unsigned)((l >> 3) * 128 + (l & 7) * 16) : ROWS_PARK_RD_ADDR(lds_w + NSLOT * SLOT, l);
  // the stored values of output pixel 16 it + (l >> 2), channels 8 (l & 3) ..: piece column 16 it + (l >> 2) + 1, logical chunk l & 3
  unsigned a_st[2];
#pragma unroll
  for (int it = 0; it < 2; ++it) {
    const int c = 16 * it + (l >> 2) + 1;
    a_st[it] = lds_w + ROWS_SWIZZLED(c, l & 3);
  }
  const unsigned o_lane = (unsigned)l * 16u;                                               // (pixel l >> 2, chunk l & 3) inside 16 pixels of the output row

  u32x4 rawr[2][2];            // GATED: r of output rows t (set t & 1) and t + 1, 2 x 16 B per lane
  float ps[4] = {0.f, 0.f, 0.f, 0.f}, tot[4] = {0.f, 0.f, 0.f, 0.f};   // POOL: the open row pair's chain, the open tile's groups
  f32x16 acc;

  // PReLU of the row piece in ring slot `sb` (byte offset), in place
  auto prelu_slot = [&](unsigned sb) {
    u32x4 v0, v1, v2;
    const unsigned ad = a_rw + sb;
    ROWS_RD128(v0, ad, 0);
    ROWS_RD128(v1, ad, 1024);
    ROWS_RD128(v2, ad, 2048);
    ROWS_LGKMWAIT(0, "+v"(v0), "+v"(v1), "+v"(v2));
    v0 = prelu_h8(v0, in_slope);
    v1 = prelu_h8(v1, in_slope);
    v2 = prelu_h8(v2, in_slope);
    ROWS_WR128(ad, v0, 0);
    ROWS_WR128(ad, v1, 1024);
    ROWS_WR128(ad, v2, 2048);
  };

  while (pos < end) {
    // ---- the run: chain (image b, strip x0), tiles ty0 .. ty0 + k - 1 = rows y0 .. y0 + n - 1 ----
    const int q = pos / TY, ty0 = pos - q * TY;
    const int k = min(TY - ty0, end - pos);
    const int y0 = ty0 * TR;
    const int n = min(H, (ty0 + k) * TR) - y0;
    const int b = q / SX, sx = q - b * SX, x0 = sx * RW;
    pos += k;
    bool colok[DPS];
    ROWS_COL_OK(R::RWH, 1, DPS, d_col, x0, W, colok)
    const bool xok0 = x0 + (l >> 2) < W, xok1 = x0 + 16 + (l >> 2) < W;
    bool xokp[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) xokp[it] = x0 + it * 8 + (l >> 3) < W;
    float gt[8];
    if constexpr (MODE == GATED) {             // gate[b][8 (l & 3) + j]: waited for here, before the run's first DMA
      const __amdgpu_buffer_rsrc_t rs_g = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.gate), 0, a.B * 128, RSRC_W3);
      u32x4 g0 = __builtin_amdgcn_raw_buffer_load_b128(rs_g, (unsigned)(b * 128 + (l & 3) * 32), 0, 0);
      u32x4 g1 = __builtin_amdgcn_raw_buffer_load_b128(rs_g, (unsigned)(b * 128 + (l & 3) * 32 + 16), 0, 0);
      asm volatile("" : "+v"(g0), "+v"(g1));
      gt[0] = __uint_as_float(g0.x); gt[1] = __uint_as_float(g0.y); gt[2] = __uint_as_float(g0.z); gt[3] = __uint_as_float(g0.w);
      gt[4] = __uint_as_float(g1.x); gt[5] = __uint_as_float(g1.y); gt[6] = __uint_as_float(g1.z); gt[7] = __uint_as_float(g1.w);
    }
    // the DMAs of load m: row y0 - 1 + m into slot m % NSLOT (loads 0 .. n + 1 are the run; its first and last may lie outside the image)
    auto issue_row = [&](int m, int slot) {
      const int j = y0 - 1 + m;
      const unsigned dead = (j >= 0 && j < H && m <= n + 1) ? 0u : OOB;
      const unsigned rowb = ROWS_ROW_BYTE(1, b * H + j, W, x0);
      ROWS_ISSUE_ROW(LD_AUX, DPS, SLOT, rs_src, colok, d_rel, rowb, dead, lds_w, slot)
    };

    int cur = 0;             // ring slot of load t (the row above the output row)
    // Step t: output row y0 + t from loads t, t + 1, t + 2.  SET: t & 1.
    auto step = [&](auto settag, int t) {
      constexpr int SET = decltype(settag)::value;
      const Slots<NSLOT> sl(cur);
      issue_row(t + 2 + PF, sl.fill);
      ROWS_VMWAIT(N_ROW);                                  // load t + 2 has landed (and every older one)
      const unsigned rb[3] = {(unsigned)(cur * SLOT), (unsigned)(sl.s1 * SLOT), (unsigned)(sl.s2 * SLOT)};
      // the new row piece (load t + 2): r of output row t + 1 out of it, then its PReLU in place -- in the shadow of the first tap row's MFMAs
      u32x4 n0, n1, n2;
      const unsigned nad = a_rw + rb[2];
      ROWS_RD128(n0, nad, 0);
      ROWS_RD128(n1, nad, 1024);
      ROWS_RD128(n2, nad, 2048);
      if constexpr (MODE == GATED) {
        const unsigned r0 = a_st[0] + rb[2], r1 = a_st[1] + rb[2];
        ROWS_RD128(rawr[SET ^ 1][0], r0, 0);
        ROWS_RD128(rawr[SET ^ 1][1], r1, 0);
      }
      conv_row<2, 3>(
          acc, a_rd, rb, bw,
          [&] {                                             // the new piece (and r out of it) is in registers
            if constexpr (MODE == GATED) {
              ROWS_LGKMWAIT(12, "+v"(n0), "+v"(n1), "+v"(n2), "+v"(rawr[SET ^ 1][0]), "+v"(rawr[SET ^ 1][1]));
            } else {
              ROWS_LGKMWAIT(12, "+v"(n0), "+v"(n1), "+v"(n2));
            }
          },
          [&] {
            n0 = prelu_h8(n0, in_slope);
            n1 = prelu_h8(n1, in_slope);
            n2 = prelu_h8(n2, in_slope);
          },
          [&] {                                             // the 3 LDS operations of conv_row<.., 3>
            ROWS_WR128(nad, n0, 0);
            ROWS_WR128(nad, n1, 1024);
            ROWS_WR128(nad, n2, 2048);
          });

      // ---- the finished row: through the park buffer, then the pass's epilogue ----
      mfma_to_lds_wait();
      park_write(acc, a_pw);
      if constexpr (MODE == POOL) {
        u32x4 tq[4];
        ROWS_RD128(tq[0], a_pr, 0);                             // (the writes are in: same wave, in order)
        ROWS_RD128(tq[1], a_pr, 1024);
        ROWS_RD128(tq[2], a_pr, 2048);
        ROWS_RD128(tq[3], a_pr, 3072);
        ROWS_LGKMWAIT(0, "+v"(tq[0]), "+v"(tq[1]), "+v"(tq[2]), "+v"(tq[3]));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int it = 0; it < 4; ++it) {                      // pixels it * 8 + j of this row: elements 4 SET + it of the pair's chain
          const u32x4 tv = tq[it];
          const float v0 = __uint_as_float(tv.x), v1 = __uint_as_float(tv.y), v2 = __uint_as_float(tv.z), v3 = __uint_as_float(tv.w);
          ps[0] += xokp[it] ? v0 : 0.f;                       // (the padded conv's values at x >= W are not zero; s + 0.f = s: s is never -0)
          ps[1] += xokp[it] ? v1 : 0.f;
          ps[2] += xokp[it] ? v2 : 0.f;
          ps[3] += xokp[it] ? v3 : 0.f;
        }
        const bool last = t == n - 1;                         // a run ends where a tile ends
        if (SET == 1 || last) {                               // the pair is complete (or the image ends inside it): butterfly over j, next group
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            float s = ps[c];
            s += __shfl_xor(s, 8);
            s += __shfl_xor(s, 16);
            s += __shfl_xor(s, 32);
            tot[c] += s;
            ps[c] = 0.f;
          }
        }
        if ((t & (TR - 1)) == TR - 1 || last) {               // the tile is complete: lanes 0..7 hold its 8 channel quads
          const int tile = (b * TY + ty0 + (t >> 3)) * SX + sx;
          u32x4 od = {__float_as_uint(tot[0]), __float_as_uint(tot[1]), __float_as_uint(tot[2]), __float_as_uint(tot[3])};
          __builtin_amdgcn_raw_buffer_store_b128(od, rs_out, l < 8 ? (unsigned)(tile * 128 + l * 16) : OOB, 0, 0);
          asm volatile("s_nop 2" : "+v"(od));
          tot[0] = tot[1] = tot[2] = tot[3] = 0.f;
        }
      } else {
        u32x4 tq[2][2];
        park_read(tq, a_pr);
        u32x4 sv[2];                                           // STAGED: the operand row itself (load t + 1, rewritten a step ago)
        if constexpr (MODE == STAGED) {
          const unsigned c0 = a_st[0] + rb[1], c1 = a_st[1] + rb[1];
          ROWS_RD128(sv[0], c0, 0);
          ROWS_RD128(sv[1], c1, 0);
          ROWS_LGKMWAIT(0, ROWS_PARKED(tq), "+v"(sv[0]), "+v"(sv[1]));
        } else {
          ROWS_LGKMWAIT(0, ROWS_PARKED(tq));
        }
        __builtin_amdgcn_sched_barrier(0);
        const unsigned orow = (unsigned)((b * H + y0 + t) * W + x0) * 64u;
#pragma unroll
        for (int it = 0; it < 2; ++it) {
          u32x4 od;
          if constexpr (MODE == STAGED) {
            od = sv[it];
          } else {
            // eca_apply_kernel<2> on o16 = fp16(acc): out = fp16(PReLU(o16 * gate + r))
            const u32x4 t0 = tq[it][0], t1 = tq[it][1], rv = rawr[SET][it];
            const float4 o0 = paif::f16x4_to_f32(paif::f32_to_f16x4(
                make_float4(__uint_as_float(t0.x), __uint_as_float(t0.y), __uint_as_float(t0.z), __uint_as_float(t0.w))));
            const float4 o1 = paif::f16x4_to_f32(paif::f32_to_f16x4(
                make_float4(__uint_as_float(t1.x), __uint_as_float(t1.y), __uint_as_float(t1.z), __uint_as_float(t1.w))));
            const float4 r0 = paif::f16x4_to_f32(make_uint2(rv.x, rv.y)), r1 = paif::f16x4_to_f32(make_uint2(rv.z, rv.w));
            float4 u0, u1;
            u0.x = __fadd_rn(__fmul_rn(o0.x, gt[0]), r0.x); u0.y = __fadd_rn(__fmul_rn(o0.y, gt[1]), r0.y);
            u0.z = __fadd_rn(__fmul_rn(o0.z, gt[2]), r0.z); u0.w = __fadd_rn(__fmul_rn(o0.w, gt[3]), r0.w);
            u1.x = __fadd_rn(__fmul_rn(o1.x, gt[4]), r1.x); u1.y = __fadd_rn(__fmul_rn(o1.y, gt[5]), r1.y);
            u1.z = __fadd_rn(__fmul_rn(o1.z, gt[6]), r1.z); u1.w = __fadd_rn(__fmul_rn(o1.w, gt[7]), r1.w);
            const uint2 h0 = paif::f32_to_f16x4(make_float4(paif::prelu_f(u0.x, slope), paif::prelu_f(u0.y, slope), paif::prelu_f(u0.z, slope),
                                                            paif::prelu_f(u0.w, slope)));
            const uint2 h1 = paif::f32_to_f16x4(make_float4(paif::prelu_f(u1.x, slope), paif::prelu_f(u1.y, slope), paif::prelu_f(u1.z, slope),
                                                            paif::prelu_f(u1.w, slope)));
            od = u32x4{h0.x, h0.y, h1.x, h1.y};
          }
          const bool ok = it ? xok1 : xok0;
          __builtin_amdgcn_raw_buffer_store_b128(od, rs_out, ok ? orow + (unsigned)(it * 1024) + o_lane : OOB, 0, ER_ST_AUX);
          asm volatile("s_nop 2" : "+v"(od));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      cur = sl.s1;
    };

    // ---- prologue: loads 0 .. 1 + PF into slots 0 .. 1 + PF; rows y0 - 1 and y0 are staged here, every later one by the step that waits for it ----
    static_assert(PF == 2 && NSLOT >= 4, "the prologue lists 2 + PF = 4 loads");
    issue_row(0, 0);
    issue_row(1, 1);
    issue_row(2, 2);
    issue_row(3, 3);
    ROWS_VMWAIT(2 * DPS);      // loads 0 and 1 have landed
    if constexpr (MODE == GATED) {
      const unsigned r0 = a_st[0] + SLOT, r1 = a_st[1] + SLOT;
      ROWS_RD128(rawr[0][0], r0, 0);                            // r of output row 0 = load 1
      ROWS_RD128(rawr[0][1], r1, 0);
      ROWS_LGKMWAIT(0, "+v"(rawr[0][0]), "+v"(rawr[0][1]));
    }
    prelu_slot(0);
    prelu_slot(SLOT);
    for (int t = 0;; t += 2) {
      step(std::integral_constant<int, 0>{}, t);
      if (t + 1 >= n) break;
      step(std::integral_constant<int, 1>{}, t + 1);
      if (t + 2 >= n) break;
    }
    ROWS_VMWAIT(0);            // no LDS-DMA of this run may land in the next run's ring, or after the workgroup's LDS is released
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  }
}

template <int MODE>
int launch_f(const Args& a, hipStream_t st, const char* what) {
  const int SX = (a.W + RW - 1) / RW, TY = (a.H + TR - 1) / TR;
  const int total = a.B * SX * TY;
  const Partition pt(total, MIN_RUN, R::MAX_WAVES);
  const int run = pt.run, waves = pt.waves;
  hipLaunchKernelGGL((eca_conv2_rows<MODE>), dim3((waves + WAVES - 1) / WAVES), dim3(WAVES * 64), 0, st, a, total, SX, TY, run);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    paif::set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace

int env_switch() {
  const char* e = getenv("PAIF_ECA_ROWS");
  if (!e || !e[0]) return -1;
  return e[0] == '0' ? 0 : 1;
}

bool fits(int B, int H, int W) {
  // 32-bit byte offsets into the maps, and the out-of-range marker above every one of them
  return B > 0 && H > 0 && W > 0 && (long long)B * H * W * 64 < (1ll << 31);
}

bool by_size_rule(int B, int H, int W) {
  return fits(B, H, W) && fills_chip(B, H, W);   // conv3x3_h16_dma_rows' rule
}

int launch(Mode m, const Args& a, hipStream_t st) {
  switch (m) {
    case POOL: return launch_f<POOL>(a, st, "eca_conv2_rows(pool)");
    case GATED: return launch_f<GATED>(a, st, "eca_conv2_rows(gated)");
    default: return launch_f<STAGED>(a, st, "eca_conv2_rows(staged)");
  }
}

}  // namespace paif_eca_rows
