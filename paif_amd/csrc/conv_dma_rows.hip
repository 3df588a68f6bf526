// The 3x3 dilation-2 conv over ONE 16-bit NHWC-32 source with plain 16-bit weights (32 -> 32), 0-3 residual maps, 16-bit or fp32 output,
// on the row-streaming LDS-DMA body of conv_rows.h (halo 2).  Replaces conv_bf16x3_ws<3, 2, 4 | 12 | 15> (conv_mfma.hip) on large maps:
// the ResidualModule's composed conv is a pure stream (one source's worth of MFMA work under 2.5 times the bytes of
// conv3x3_h16_dma<1, 0>), and the persistent wave-specialised kernel stages it through registers (loader waves, VALU writes to LDS, two
// barriers per stage) although a stored 16-bit value IS the MFMA operand.  What is this kernel's own:
//   * PARITY CHAINS: the vertical taps of output row o are rows o - 2, o, o + 2, so even and odd rows are independent problems.  A chain is
//     (image, 32-column strip, row parity); a run is consecutive chain rows;
//   * the vector-memory pattern of a step: residual loads of row t + D, 3 DMAs of row t + 2 + PF, the row's stores;
//   * arithmetic as conv_ws_body<3, 2, ST> runs it: epilogue fma(acc, scale, shift) -> activation -> * alpha (fused into the first
//     residual add, as hipcc contracts the storers' expression) -> + res[1] + res[2] -> f32_to_h4<F> or an fp32 store: the same
//     operations in the same order on every pixel, so the same bits.
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "conv_dma.h"
#include "conv_rows.h"

namespace paif_conv_dma {
namespace {

using namespace paif_rows;
typedef Ring<2> R;
constexpr int RW = R::RW, DPS = R::DPS, SLOT = R::SLOT, NSLOT = R::NSLOT, PF = R::PF, WAVES = R::WAVES;
constexpr int MIN_RUN = MIN_RUN_ROWS;         // chain rows per wave at least

#ifndef CR_LD_AUX
#define CR_LD_AUX 2     // cache policy of the loads (LDS-DMA and residual maps): 2 = streaming (nt), 0 = default
#endif
#ifndef CR_ST_AUX
#define CR_ST_AUX 0     // cache policy of the output stores: 0 = default, 2 = streaming (nt); the choice conv_h16_dma_1x1 measured best
#endif

// F: 16-bit format of maps and weights (1 bf16, 2 fp16).  NRES: residual maps (16-bit, format F).  O32: the output is fp32.
// total = B * SX * H strip-rows (SX strips of 32 columns) in the order (image, strip, parity, chain row); wave g owns [g * run, (g + 1) * run)
// and splits it at chain boundaries.
template <int F, int NRES, bool O32>
__global__ __launch_bounds__(WAVES * 64, 2) void conv3x3_h16_dma_rows(Args a, int total, int SX, int run) {
  // residual loads run D rows ahead in a ring of D + 1 register sets (2 x NRES x 4 registers each)
  constexpr int D = NRES == 3 ? 1 : 2, NSETS = D + 1, RL = 2 * NRES;
  constexpr int N_ROW = PF * (RL + DPS);        // younger loads behind the DMAs of row t + 2 at the wait of step t
  constexpr int N_RES = DPS + D * (RL + DPS);   // younger loads behind the residual loads of row t
  static_assert(N_ROW <= 63 && N_RES <= 63, "vmcnt is 6 bits");
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
  const int n_even = (H + 1) >> 1;             // chain rows of parity 0; parity 1 has H - n_even

  constexpr int OPITCH = O32 ? 128 : 64;       // bytes per output pixel
  const int map_bytes = a.B * H * W * 64;
  const __amdgpu_buffer_rsrc_t rs_src = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.src[0]), 0, map_bytes, RSRC_W3);
  __amdgpu_buffer_rsrc_t rs_res[NRES > 0 ? NRES : 1];
#pragma unroll
  for (int r = 0; r < NRES; ++r) rs_res[r] = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.res[r]), 0, map_bytes, RSRC_W3);
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, a.B * H * W * OPITCH, RSRC_W3);

  u32x4 bw[9][2];
  ROWS_LOAD_BW(bw, a.wpk, l)
  // epilogue constants in the [pixel][8 channels] layout a lane stores: channels 8 (l & 3) + j
  float esc[8], esh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * (l & 3) + j;
    esc[j] = a.scale ? a.scale[c] : 1.f;
    esh[j] = a.shift ? a.shift[c] : 0.f;
  }
  // prelu_f with slope 1 is the identity, bit for bit: no branch on the activation inside the row loop
  const bool relu = a.act == 2;
  const float slope = a.act == 1 ? *a.prelu : 1.f;
  const float alpha = a.alpha;

  // ---- geometry of this lane ----
  int d_col[DPS];
  unsigned d_rel[DPS];
  ROWS_DMA_GEOMETRY(DPS, l, d_col, d_rel)
  const unsigned lds_w = (unsigned)(w * R::WAVE_LDS);                                      // this wave's ring; its park buffer behind it
  unsigned a_rd[3][2];
  ROWS_A_ADDRS(2, lds_w, p, hh, a_rd)
  const unsigned a_pw = ROWS_PARK_WR_ADDR(lds_w + NSLOT * SLOT, p, hh);
  const unsigned a_pr = ROWS_PARK_RD_ADDR(lds_w + NSLOT * SLOT, l);
  const unsigned e_lane = (unsigned)l * 16u;                                               // (pixel l >> 2, chunk l & 3) inside 16 pixels of a 16-bit map
  const unsigned o_lane = O32 ? (unsigned)((l >> 2) * 128 + (l & 3) * 32) : e_lane;        // the same in the output map

  u32x4 rr[NSETS][NRES > 0 ? NRES : 1][2];    // residual maps of a row: 2 x 16 B per lane and map
  f32x16 acc;

  while (pos < end) {
    // ---- the run: chain (image b, strip x0, parity par), chain rows i0 .. i0 + n - 1 (image rows 2 i + par) ----
    const int q = pos / H, rem = pos - q * H;
    const int par = rem >= n_even ? 1 : 0;
    const int i0 = rem - par * n_even;
    const int nch = par ? H - n_even : n_even;
    const int n = min(nch - i0, end - pos);
    const int b = q / SX, x0 = (q - b * SX) * RW;
    pos += n;
    bool colok[DPS];
    ROWS_COL_OK(R::RWH, 2, DPS, d_col, x0, W, colok)
    const bool xok0 = x0 + (l >> 2) < W, xok1 = x0 + 16 + (l >> 2) < W;
    // the DMAs of load m: chain row i0 - 1 + m into slot m % NSLOT (loads 0 .. n + 1 are the run; its first and last may lie outside the image)
    auto issue_row = [&](int m, int slot) {
      const int j = i0 - 1 + m;
      const unsigned dead = (j >= 0 && j < nch && m <= n + 1) ? 0u : OOB;
      const unsigned rowb = ROWS_ROW_BYTE(2, b * H + 2 * j + par, W, x0);
      ROWS_ISSUE_ROW(CR_LD_AUX, DPS, SLOT, rs_src, colok, d_rel, rowb, dead, lds_w, slot)
    };
    // the residual maps of output row t of the run
    auto issue_res = [&](auto settag, int t) {
      constexpr int SET = decltype(settag)::value;
      const bool live = t >= 0 && t < n;
      const unsigned rowb = (unsigned)((b * H + 2 * (i0 + t) + par) * W + x0) * 64u;
#pragma unroll
      for (int r = 0; r < NRES; ++r) {
        rr[SET][r][0] = __builtin_amdgcn_raw_buffer_load_b128(rs_res[r], (live && xok0) ? rowb + e_lane : OOB, 0, CR_LD_AUX);
        rr[SET][r][1] = __builtin_amdgcn_raw_buffer_load_b128(rs_res[r], (live && xok1) ? rowb + 1024u + e_lane : OOB, 0, CR_LD_AUX);
      }
    };
    // the vector-memory loads of step s, in issue order: residual maps of row s + D, then the DMAs of load s + 2 + PF
    auto issue_step = [&](auto settag, int s, int slot) {
      if constexpr (NRES > 0) issue_res(settag, s + D);
      asm volatile("" ::: "memory");                    // keep the residual loads in front of the DMAs in the vector-memory queue
      issue_row(s + 2 + PF, slot);
    };

    int cur = 0;             // ring slot of load t (the row above the output row)
    // Step t: output row t of the run from loads t, t + 1, t + 2.  SET: t % NSETS.
    auto step = [&](auto settag, int t) {
      constexpr int SET = decltype(settag)::value;
      const Slots<NSLOT> sl(cur);
      issue_step(std::integral_constant<int, (SET + D) % NSETS>{}, t, sl.fill);
      ROWS_VMWAIT(N_ROW);                                  // load t + 2 has landed (and every older one)
      const unsigned rb[3] = {(unsigned)(cur * SLOT), (unsigned)(sl.s1 * SLOT), (unsigned)(sl.s2 * SLOT)};
      conv_row<F>(acc, a_rd, rb, bw);

      // ---- the finished row: through the park buffer into [pixel][8 channels], epilogue, stores ----
      mfma_to_lds_wait();
      u32x4 tq[2][2];
      park_transpose(acc, a_pw, a_pr, tq);
      if constexpr (NRES > 0 && N_RES < N_ROW) {              // the row's residual maps were requested behind the DMAs waited for above
        ROWS_VMWAIT(N_RES);
      }
      __builtin_amdgcn_sched_barrier(0);
      const unsigned orow = (unsigned)((b * H + 2 * (i0 + t) + par) * W + x0) * (unsigned)OPITCH;
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        float ev[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = __builtin_fmaf(__uint_as_float(tq[it][j >> 2][j & 3]), esc[j], esh[j]);
          const float vp = paif::prelu_f(v, slope), vr = fmaxf(v, 0.f);
          v = relu ? vr : vp;
          if constexpr (NRES == 0) {
            v = v * alpha;
          } else {
#pragma unroll
            for (int r = 0; r < NRES; ++r) {
              const unsigned u = rr[SET][r][it][j >> 1];
              float rv;
              if constexpr (F == 2) rv = (float)__builtin_bit_cast(paif::f16x2_t, u)[j & 1];
              else rv = __uint_as_float((j & 1) ? (u & 0xffff0000u) : (u << 16));
              v = r == 0 ? __builtin_fmaf(v, alpha, rv) : v + rv;
            }
          }
          ev[j] = v;
        }
        const bool ok = it ? xok1 : xok0;
        if constexpr (O32) {
          u32x4 o0 = {__float_as_uint(ev[0]), __float_as_uint(ev[1]), __float_as_uint(ev[2]), __float_as_uint(ev[3])};
          u32x4 o1 = {__float_as_uint(ev[4]), __float_as_uint(ev[5]), __float_as_uint(ev[6]), __float_as_uint(ev[7])};
          const unsigned off = ok ? orow + (unsigned)(it * 16 * OPITCH) + o_lane : OOB;
          __builtin_amdgcn_raw_buffer_store_b128(o0, rs_out, off, 0, CR_ST_AUX);
          asm volatile("s_nop 2" : "+v"(o0));               // 128-bit store data: WAR hazard hipcc does not pad
          __builtin_amdgcn_raw_buffer_store_b128(o1, rs_out, ok ? off + 16u : OOB, 0, CR_ST_AUX);
          asm volatile("s_nop 2" : "+v"(o1));
        } else {
          const uint2 h0 = paif::f32_to_h4<F>(make_float4(ev[0], ev[1], ev[2], ev[3]));
          const uint2 h1 = paif::f32_to_h4<F>(make_float4(ev[4], ev[5], ev[6], ev[7]));
          u32x4 od = {h0.x, h0.y, h1.x, h1.y};
          __builtin_amdgcn_raw_buffer_store_b128(od, rs_out, ok ? orow + (unsigned)(it * 16 * OPITCH) + o_lane : OOB, 0, CR_ST_AUX);
          asm volatile("s_nop 2" : "+v"(od));
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      cur = sl.s1;
    };

    // ---- prologue: the loads of the virtual steps -(2 + PF) .. -1, in the pattern of a step (the residual maps of rows < 0 are dead) ----
    static_assert(PF == 2, "the prologue lists 2 + PF = 4 virtual steps");
    auto vstep = [&](auto stag) {
      constexpr int S = decltype(stag)::value;             // -(2 + PF) .. -1: load S + 2 + PF into slot S + 2 + PF
      issue_step(std::integral_constant<int, (((S + D) % NSETS) + NSETS) % NSETS>{}, S, S + 2 + PF);
    };
    vstep(std::integral_constant<int, -4>{});
    vstep(std::integral_constant<int, -3>{});
    vstep(std::integral_constant<int, -2>{});
    vstep(std::integral_constant<int, -1>{});
    for (int t = 0;; t += NSETS) {
      step(std::integral_constant<int, 0>{}, t);
      if (t + 1 >= n) break;
      step(std::integral_constant<int, 1 % NSETS>{}, t + 1);
      if (t + 2 >= n) break;
      if constexpr (NSETS > 2) {
        step(std::integral_constant<int, 2 % NSETS>{}, t + 2);
        if (t + 3 >= n) break;
      }
    }
    ROWS_VMWAIT(0);            // no LDS-DMA of this run may land in the next run's ring, or after the workgroup's LDS is released
  }
}

int env_rows() {             // PAIF_CONV_DMA_ROWS, read per call: -1 unset (the size rule), 0 never, 1 wherever the hard limits hold
  const char* d = getenv("PAIF_CONV_DMA");         // PAIF_CONV_DMA=0: no LDS-DMA kernel anywhere
  if (d && d[0] == '0') return 0;
  const char* e = getenv("PAIF_CONV_DMA_ROWS");
  if (!e || !e[0]) return -1;
  return e[0] == '0' ? 0 : 1;
}

template <int F, int NRES, bool O32>
void launch_rows_f(const Args& a, hipStream_t st) {
  const int SX = (a.W + RW - 1) / RW;
  const int total = a.B * SX * a.H;
  const Partition pt(total, MIN_RUN, R::MAX_WAVES);
  const int run = pt.run, waves = pt.waves;
  hipLaunchKernelGGL((conv3x3_h16_dma_rows<F, NRES, O32>), dim3((waves + WAVES - 1) / WAVES), dim3(WAVES * 64), 0, st, a, total, SX, run);
}

}  // namespace

// classify()'s ROWS (conv_dma.hip)
bool is_rows(const Args& a) {
  if (a.kh != 3 || a.dil != 2 || a.cout != 32) return false;
  const int sw = env_rows();
  // the forms built: one source without an input activation, 0-3 residual maps, no fused ChannelPool; fp32 output from fp16 sources only
  if (sw == 0 || a.nsrc != 1 || a.nres < 0 || a.nres > 3 || a.in_relu || a.cpool || (a.out_f32 && !a.f16)) return false;
  // 32-bit byte offsets, and the out-of-range marker above every one of them
  if ((long long)a.B * a.H * a.W * (a.out_f32 ? 128 : 64) >= (1ll << 31)) return false;
  if (sw == 1) return true;
  return fills_chip(a.B, a.H, a.W);
}

int launch_rows(const Args& a, hipStream_t st) {
#define CR_LAUNCH(NR)                                                              \
  case NR:                                                                         \
    if (a.out_f32) launch_rows_f<2, NR, true>(a, st);                              \
    else if (a.f16) launch_rows_f<2, NR, false>(a, st);                            \
    else launch_rows_f<1, NR, false>(a, st);                                       \
    break;
  switch (a.nres) {
    CR_LAUNCH(0)
    CR_LAUNCH(1)
    CR_LAUNCH(2)
    CR_LAUNCH(3)
    default: break;
  }
#undef CR_LAUNCH
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    paif::set_error("conv2d(h16 dma rows): launch failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace paif_conv_dma
