// The 3x3 dilation-2 conv over ONE 16-bit NHWC-32 source with plain 16-bit weights (32 -> 32), 0-3 residual maps, 16-bit or fp32 output,
// as a row-streaming LDS-DMA kernel.  Replaces conv_bf16x3_ws<3, 2, 4 | 12 | 15> (conv_mfma.hip) on large maps: the ResidualModule's
// composed conv is a pure stream (one source's worth of MFMA work under 2.5 times the bytes of conv3x3_h16_dma<1, 0>), and the
// persistent wave-specialised kernel stages it through registers (loader waves, VALU writes to LDS, two barriers per stage) although a
// stored 16-bit value IS the MFMA operand.  Same data path as conv_h16_dma_1x1 (conv_dma_1x1.hip), with the halo a 3x3 needs:
//   * PARITY CHAINS: the vertical taps of output row o are rows o - 2, o, o + 2, so even and odd rows are independent problems.  A chain is
//     (image, 32-column strip, row parity); a wave walks a RUN of consecutive chain rows downward and shares nothing with any other wave:
//     a wave-private LDS ring, no s_barrier anywhere.  A run costs one warm-up row at each end;
//   * a ring slot is one source row piece, 36 pixels x 64 B, fetched by 3 DMA instructions (buffer_load_dwordx4 ... lds; the lanes past
//     the 36th pixel are dead); 5 slots: rows o - 2, o, o + 2 resident, 2 in flight.  Two workgroups of 4 waves per CU (the B operand is
//     72 registers): 8 waves x 19 KB = 152 KB of LDS;
//   * the 16-byte chunk a lane fetches is XOR-swizzled on the source side exactly as in conv3x3_h16_dma, so the A-operand ds_read_b128 of
//     32 consecutive pixels at column shifts 0 / 2 / 4 is conflict-free; zero padding is the buffer descriptor's range check;
//   * the vector-memory pattern of a step is fixed (residual loads of row t + D, 3 DMAs of row t + 2 + PF, the row's stores; dead ones
//     carry an out-of-range offset), so every s_waitcnt vmcnt(N) is a compile-time count of YOUNGER LOADS (stores do not retire in order
//     with loads, conv_dma.hip Sched); every LDS access is inline asm;
//   * arithmetic as conv_ws_body<3, 2, ST> runs it: paif::mfma16<F> 32x32x16, tap = dy * 3 + dx ascending, k-step inner, fp32
//     accumulation from zero; epilogue fma(acc, scale, shift) -> activation -> * alpha (fused into the first residual add, as hipcc
//     contracts the storers' expression) -> + res[1] + res[2] -> f32_to_h4<F> or an fp32 store: the same operations in the same
//     order on every pixel, so the same bits.
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "conv_dma.h"
#include "paif_common.h"

namespace paif_conv_dma {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr int RW = 32;                        // output columns of a strip
constexpr int RWH = RW + 4;                   // source columns of a row piece (dilation 2: two halo columns each side)
constexpr int DPS = 3;                        // DMA instructions per row piece (64 lanes x 16 B each: 48 pixels, 36 live)
constexpr int SLOT = DPS * 1024;
constexpr int NSLOT = 5, PF = NSLOT - 3;      // ring slots: 3 resident rows + PF in flight
constexpr int PARK = 32 * 32 * 4;             // per-wave [32 px][32 ch] fp32 transposition buffer
constexpr int WAVE_LDS = NSLOT * SLOT + PARK; // 19 KB
constexpr int WAVES = 4;
constexpr int LDS_BYTES = WAVES * WAVE_LDS;   // 76 KB: two workgroups per CU
constexpr int MAX_WAVES = 2048;               // 2 workgroups on each of 256 CUs
constexpr int MIN_RUN = 16;                   // chain rows per wave at least: the two warm-up rows cost at most 1/8
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU do not fit LDS");
static_assert(RWH * 4 <= DPS * 64, "DMA instructions do not cover the row piece");
constexpr unsigned RSRC_W3 = 0x00020000u;
constexpr unsigned OOB = 0x80000000u;         // a byte offset no map reaches (checked at launch): the hardware returns 0 / drops the store

#ifndef CR_LD_AUX
#define CR_LD_AUX 2     // cache policy of the loads (LDS-DMA and residual maps): 2 = streaming (nt), 0 = default
#endif
#ifndef CR_ST_AUX
#define CR_ST_AUX 0     // cache policy of the output stores: 0 = default, 2 = streaming (nt); the choice conv_h16_dma_1x1 measured best
#endif
#define CR_VMWAIT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define CR_RD128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#define CR_WR32(addr, val, off) asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "v"(val), "n"(off) : "memory")

__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned lds_off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(uintptr_t)lds_off, 16, voff, 0, 0, CR_LD_AUX);
}

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
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
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

  // ---- B operand: [tap][k-step], lane (n = l & 31, k = 8 (l >> 5) + j) -- the hi halves of the pack [tap][ks][hi|lo][64 lanes][16 B] ----
  u32x4 bw[9][2];
  {
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wpk), 0, 9 * 2 * 2 * 1024, RSRC_W3);
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) bw[tap][ks] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (unsigned)l * 16u, ((tap * 2 + ks) * 2) * 1024, 0);
  }
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
  // DMA instruction i moves chunk n = 64 i + l of the slot: piece column c = n >> 2, physical 16-byte chunk n & 3 = logical chunk ^ ((c >> 2) & 3)
  int d_col[DPS];
  unsigned d_rel[DPS];
#pragma unroll
  for (int i = 0; i < DPS; ++i) {
    const int n = 64 * i + l, c = n >> 2;
    d_col[i] = c;
    d_rel[i] = (unsigned)(c * 64 + (((n & 3) ^ ((c >> 2) & 3)) * 16));
  }
  const unsigned lds_w = (unsigned)(w * WAVE_LDS);                                        // this wave's ring; its park buffer behind it
  // A operand of output pixel p, horizontal tap dx, k-step ks: lane (pixel p, k half hh) reads piece column p + 2 dx
  unsigned a_rd[3][2];
#pragma unroll
  for (int dx = 0; dx < 3; ++dx)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      const int c = p + 2 * dx;
      a_rd[dx][ks] = lds_w + (unsigned)(c * 64 + (((2 * ks + hh) ^ ((c >> 2) & 3)) * 16));
    }
  const unsigned a_pw = lds_w + NSLOT * SLOT + (unsigned)((4 * hh * 32 + p) * 4);          // + ((r & 3) + 8 (r >> 2)) * 128
  const unsigned a_pr = lds_w + NSLOT * SLOT + (unsigned)((l >> 2) * 128 + (l & 3) * 32);  // + it * 2048 (+ 16): pixel 16 it + (l >> 2), 8 channels
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
#pragma unroll
    for (int i = 0; i < DPS; ++i) colok[i] = d_col[i] < RWH && (unsigned)(x0 - 2 + d_col[i]) < (unsigned)W;
    const bool xok0 = x0 + (l >> 2) < W, xok1 = x0 + 16 + (l >> 2) < W;
    // the DMAs of load m: chain row i0 - 1 + m into slot m % NSLOT (loads 0 .. n + 1 are the run; its first and last may lie outside the image)
    auto issue_row = [&](int m, int slot) {
      const int j = i0 - 1 + m;
      const unsigned dead = (j >= 0 && j < nch && m <= n + 1) ? 0u : OOB;              // (a scalar OR, not a branch around the DMAs)
      const unsigned rowb = (unsigned)((b * H + 2 * j + par) * W + x0 - 2) * 64u;
#pragma unroll
      for (int i = 0; i < DPS; ++i) dma16(rs_src, (colok[i] ? rowb + d_rel[i] : OOB) | dead, lds_w + (unsigned)(slot * SLOT + i * 1024));
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
      const int s1 = cur + 1 >= NSLOT ? cur + 1 - NSLOT : cur + 1, s2 = cur + 2 >= NSLOT ? cur + 2 - NSLOT : cur + 2;
      const int fill = cur == 0 ? NSLOT - 1 : cur - 1;   // = (t + 2 + PF) % NSLOT: the slot of load t - 1, read one step ago
      issue_step(std::integral_constant<int, (SET + D) % NSETS>{}, t, fill);
      CR_VMWAIT(N_ROW);                                  // load t + 2 has landed (and every older one)
      const unsigned rb[3] = {(unsigned)(cur * SLOT), (unsigned)(s1 * SLOT), (unsigned)(s2 * SLOT)};
      u32x4 A[2][3][2];       // [buffer][dx][ks]: the fragments of one vertical tap
      auto read = [&](int buf, int dy) {
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            const unsigned ad = a_rd[dx][ks] + rb[dy];
            CR_RD128(A[buf][dx][ks], ad, 0);
          }
      };
      auto mma = [&](auto dytag) {
        constexpr int dy = decltype(dytag)::value, buf = dy & 1;
#pragma unroll
        for (int dx = 0; dx < 3; ++dx)
#pragma unroll
          for (int ks = 0; ks < 2; ++ks) {
            if (dy == 0 && dx == 0 && ks == 0) {         // first product of a row: C = 0
              const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
              acc = paif::mfma16<F>(A[buf][dx][ks], bw[dy * 3 + dx][ks], z);
            } else {
              acc = paif::mfma16<F>(A[buf][dx][ks], bw[dy * 3 + dx][ks], acc);
            }
          }
      };
      read(0, 0);
      read(1, 1);
      asm volatile("s_waitcnt lgkmcnt(6)"
                   : "+v"(A[0][0][0]), "+v"(A[0][0][1]), "+v"(A[0][1][0]), "+v"(A[0][1][1]), "+v"(A[0][2][0]), "+v"(A[0][2][1])::"memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(std::integral_constant<int, 0>{});
      __builtin_amdgcn_sched_barrier(0);
      read(0, 2);
      asm volatile("s_waitcnt lgkmcnt(6)"
                   : "+v"(A[1][0][0]), "+v"(A[1][0][1]), "+v"(A[1][1][0]), "+v"(A[1][1][1]), "+v"(A[1][2][0]), "+v"(A[1][2][1])::"memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(std::integral_constant<int, 1>{});
      __builtin_amdgcn_sched_barrier(0);
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(A[0][0][0]), "+v"(A[0][0][1]), "+v"(A[0][1][0]), "+v"(A[0][1][1]), "+v"(A[0][2][0]), "+v"(A[0][2][1])::"memory");
      __builtin_amdgcn_sched_barrier(0);
      mma(std::integral_constant<int, 2>{});
      __builtin_amdgcn_sched_barrier(0);

      // ---- the finished row: through the park buffer into [pixel][8 channels], epilogue, stores ----
      asm volatile("s_nop 15\n\ts_nop 7" ::: "memory");       // MFMA result -> LDS-store data: wait states inline asm does not get
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float v = acc[r];
        CR_WR32(a_pw, v, ((r & 3) + 8 * (r >> 2)) * 128);
      }
      u32x4 tq[2][2];
      CR_RD128(tq[0][0], a_pr, 0);                            // (LDS operations of a wave complete in order: the writes are in)
      CR_RD128(tq[0][1], a_pr, 16);
      CR_RD128(tq[1][0], a_pr, 2048);
      CR_RD128(tq[1][1], a_pr, 2048 + 16);
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(tq[0][0]), "+v"(tq[0][1]), "+v"(tq[1][0]), "+v"(tq[1][1])::"memory");
      if constexpr (NRES > 0 && N_RES < N_ROW) {              // the row's residual maps were requested behind the DMAs waited for above
        CR_VMWAIT(N_RES);
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
      cur = s1;
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
    CR_VMWAIT(0);            // no LDS-DMA of this run may land in the next run's ring, or after the workgroup's LDS is released
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
  const int per = (total + MAX_WAVES - 1) / MAX_WAVES;
  const int run = per > MIN_RUN ? per : MIN_RUN;
  const int waves = (total + run - 1) / run;
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
  // the size rule: runs of at least MIN_RUN chain rows on every one of the 2048 waves, and chains long enough to hold them
  return a.H >= 64 && (long long)a.B * a.H * ((a.W + RW - 1) / RW) >= (long long)MIN_RUN * MAX_WAVES;
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
