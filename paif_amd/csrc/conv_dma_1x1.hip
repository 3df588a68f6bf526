// The folded decomposition 1x1 (96 -> 32 over the virtual concat [x, HF1, HF2]) on 16-bit NHWC maps with plain 16-bit weights, as a
// streaming LDS-DMA kernel.  Replaces conv_bf16x3_ws<1, 1, 4 | 12> (conv_mfma.hip) for that form: the persistent wave-specialised kernel
// stages its input through registers (loader waves, VALU writes to LDS, two barriers per stage) although a stored 16-bit value IS the
// MFMA operand.  The wave-private data path of conv_rows.h (its rules on vmcnt and inline-asm LDS access, its operand swizzle and
// park step), minus everything a 1x1 does not need:
//   * no halo: a map is a run of B*H*W pixels x 64 B, a TILE is 64 consecutive pixels, and every wave streams its own tiles;
//   * a ring slot is one source of one tile (4 KB = 4 DMA instructions); 4 slots, 3 in flight behind the one being read.  Two workgroups of
//     4 waves per CU (two waves per SIMD: the B operand is 24 registers): 8 waves x 12 KB = 96 KB in flight per CU;
//   * the vector-memory pattern: 4 DMAs per stage, 4 stores per tile;
//   * arithmetic as conv_ws_body<1, 1, ST> runs it: paif::mfma16<F> 32x32x16, sources in order, k-step 0 then 1, fp32 accumulation from
//     zero; epilogue fma(acc, scale, shift) -> activation -> * alpha -> f32_to_h4<F>: the same instructions in the same order, so the
//     same bits.
// The ragged end of the map is the buffer descriptor's range check (out-of-range lanes read 0, their stores are dropped) plus an
// explicit compare on every offset.
#include <stdint.h>
#include <stdlib.h>

#include <type_traits>

#include "conv_dma.h"
#include "conv_rows.h"

namespace paif_conv_dma {
namespace {

using namespace paif_rows;

constexpr int TP = 64;                        // pixels per tile
constexpr int SLOT = TP * 64;                 // one source of a tile: 4 KB
constexpr int DPS = SLOT / 1024;              // DMA instructions per stage (64 lanes x 16 B each)
constexpr int NSLOT = 4, PF = NSLOT - 1;      // ring slots; stages in flight behind the one being read
constexpr int WAVE_LDS = NSLOT * SLOT + PARK; // 20 KB
constexpr int WAVES = 4;
constexpr int LDS_BYTES = WAVES * WAVE_LDS;   // 80 KB: two workgroups per CU
constexpr int GRID = 512;                     // persistent: 2 workgroups on each of 256 CUs
static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU do not fit LDS");
static_assert(PF == 3, "a stage's DMA target is the same source of the next tile: PF must equal the source count");

#ifndef C1_LD_AUX
#define C1_LD_AUX 2     // cache policy of the LDS-DMA loads: 2 = streaming (nt): every input byte is read exactly once; 0 = default
#endif
#ifndef C1_ST_AUX
#define C1_ST_AUX 0     // cache policy of the output stores: 0 = default, 2 = streaming (nt).  No halo is re-read here, so there is nothing a
                        // cached output line could evict; measured inside the forward (same box, three profiled runs each, us per launch):
                        // loads default / stores nt 115, loads nt / stores nt 110, loads nt / stores default 102, and the sum over
                        // all kernels of the step falls with it
#endif

// F: 16-bit format of maps and weights (1 bf16, 2 fp16)
template <int F>
// pair (conv_dma.h Prob): the second half of the grid runs problem 1; ntiles is per problem
__global__ __launch_bounds__(WAVES * 64, 2) void conv_h16_dma_1x1(Args a, int ntiles, Prob p1, int pair) {
  __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
  asm volatile("" ::"v"((unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)smem) : "memory");   // only asm touches it

  const int tid = threadIdx.x, l = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int p = l & 31, hh = l >> 5;
  // this wave's tiles: gw, gw + nw, gw + 2 nw, ... (neighbouring waves stream neighbouring 4 KB runs of each map)
  int bid = blockIdx.x, nblk = gridDim.x;      // workgroup-uniform
  if (pair) {
    nblk >>= 1;
    if (bid >= nblk) {
      bid -= nblk;
#pragma unroll
      for (int s = 0; s < 3; ++s) a.src[s] = p1.src[s];
      a.wpk = p1.wpk; a.scale = p1.scale; a.shift = p1.shift; a.prelu = p1.prelu; a.out = p1.out; a.alpha = p1.alpha;
    }
  }
  const int gw = bid * WAVES + w, nw = nblk * WAVES;
  if (gw >= ntiles) return;                    // (no barrier anywhere: a wave may leave on its own)
  const int cnt = (ntiles - gw + nw - 1) / nw;

  const unsigned map_bytes = (unsigned)(a.B * a.H * a.W) * 64u;
  __amdgpu_buffer_rsrc_t rs_src[3];
#pragma unroll
  for (int s = 0; s < 3; ++s) rs_src[s] = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.src[s]), 0, (int)map_bytes, RSRC_W3);
  const __amdgpu_buffer_rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc(a.out, 0, (int)map_bytes, RSRC_W3);

  // ---- B operand: [source][k-step], lane (n = l & 31, k = 8 (l >> 5) + j) -- the hi halves of the pack [src][tap][ks][hi|lo][64 lanes][16 B] ----
  u32x4 bw[3][2];
  {
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(a.wpk), 0, 3 * 2 * 2 * 1024, RSRC_W3);
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) bw[s][ks] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (unsigned)l * 16u, ((s * 2 + ks) * 2) * 1024, 0);
  }
  // epilogue constants in the [pixel][8 channels] layout a lane stores: channels 8 (l & 3) + j
  float esc[8], esh[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = 8 * (l & 3) + j;
    esc[j] = a.scale ? a.scale[c] : 1.f;
    esh[j] = a.shift ? a.shift[c] : 0.f;
  }
  const int act = a.act;
  const float slope = act == 1 ? *a.prelu : 0.f;
  const float alpha = a.alpha;

  // ---- geometry of this lane ----
  // DMA instruction i of a stage moves chunk n = 64 i + l of the slot: pixel n >> 2, physical 16-byte chunk n & 3 = logical chunk ^ ((pixel >> 2) & 3)
  const unsigned d_rel = ROWS_SWIZZLED(l >> 2, l & 3);                                    // + 1024 i
  const unsigned lds_w = (unsigned)(w * WAVE_LDS);                                        // this wave's ring; its park buffer behind it
  // A operand of pixel 32 sg + p, k-step ks: lane (pixel p, k half hh); (32 sg + p) >> 2 and p >> 2 agree mod 4: sg is an immediate offset
  unsigned a_rd[2];
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) a_rd[ks] = lds_w + ROWS_SWIZZLED(p, 2 * ks + hh);
  const unsigned a_pw = ROWS_PARK_WR_ADDR(lds_w + NSLOT * SLOT, p, hh);
  const unsigned a_pr = ROWS_PARK_RD_ADDR(lds_w + NSLOT * SLOT, l);
  const unsigned e_lane = (unsigned)l * 16u;                                               // (pixel l >> 2, chunk l & 3) inside 16 pixels

  auto tile_byte = [&](int k) -> unsigned { return (unsigned)(gw + k * nw) * (unsigned)SLOT; };   // < 2^32: ntiles + nw tiles of 4 KB
  unsigned d_voff[DPS];    // DMA offsets of the tile the DMAs currently target
  auto target = [&](int k) {
    const unsigned tb = tile_byte(k);
#pragma unroll
    for (int i = 0; i < DPS; ++i) {
      const unsigned off = tb + d_rel + 1024u * i;
      d_voff[i] = (k < cnt && off < map_bytes) ? off : OOB;
    }
  };
  int cur = 0;             // ring slot of the current stage
  auto issue = [&](auto stag, int slot) {
    constexpr int S = decltype(stag)::value;
#pragma unroll
    for (int i = 0; i < DPS; ++i) dma16<C1_LD_AUX>(rs_src[S], d_voff[i], lds_w + (unsigned)(slot * SLOT + i * 1024));
  };

  f32x16 acc[2];
  // One stage = one source of a tile.  Its first act is the DMA of the same source of the NEXT tile (stage g + 3) into the slot that was
  // read one stage ago (those reads were waited for in front of that stage's MFMAs); then the 12 younger loads may stay outstanding.
  auto stage = [&](auto stag) {
    constexpr int S = decltype(stag)::value;
    issue(stag, (cur + PF) & (NSLOT - 1));
    ROWS_VMWAIT(PF * DPS);
    const unsigned sb = (unsigned)cur * SLOT;
    u32x4 A[2][2];
    const unsigned ad0 = a_rd[0] + sb, ad1 = a_rd[1] + sb;
    ROWS_RD128(A[0][0], ad0, 0);
    ROWS_RD128(A[1][0], ad0, 32 * 64);
    ROWS_RD128(A[0][1], ad1, 0);
    ROWS_RD128(A[1][1], ad1, 32 * 64);
    ROWS_LGKMWAIT(0, "+v"(A[0][0]), "+v"(A[1][0]), "+v"(A[0][1]), "+v"(A[1][1]));
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int sg = 0; sg < 2; ++sg) {
        if constexpr (S == 0) {
          if (ks == 0) {                                    // first product of a tile: C = 0
            const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            acc[sg] = paif::mfma16<F>(A[sg][ks], bw[S][ks], z);
            continue;
          }
        }
        acc[sg] = paif::mfma16<F>(A[sg][ks], bw[S][ks], acc[sg]);
      }
    __builtin_amdgcn_sched_barrier(0);
    cur = (cur + 1) & (NSLOT - 1);
  };
  // the finished tile k: each accumulator through the park buffer into [pixel][8 channels], epilogue, two 16-byte stores
  auto finish = [&](int k) {
    const unsigned tb = tile_byte(k);
    mfma_to_lds_wait();
#pragma unroll
    for (int sg = 0; sg < 2; ++sg) {
      u32x4 t[2][2];
      park_transpose(acc[sg], a_pw, a_pr, t);
#pragma unroll
      for (int it = 0; it < 2; ++it) {
        float ev[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          float v = __builtin_fmaf(__uint_as_float(t[it][j >> 2][j & 3]), esc[j], esh[j]);
          if (act == 1) v = paif::prelu_f(v, slope);
          else if (act == 2) v = fmaxf(v, 0.f);
          ev[j] = v * alpha;
        }
        const uint2 o0 = paif::f32_to_h4<F>(make_float4(ev[0], ev[1], ev[2], ev[3]));
        const uint2 o1 = paif::f32_to_h4<F>(make_float4(ev[4], ev[5], ev[6], ev[7]));
        u32x4 od = {o0.x, o0.y, o1.x, o1.y};
        const unsigned off = tb + (unsigned)(sg * 2048 + it * 1024) + e_lane;
        __builtin_amdgcn_raw_buffer_store_b128(od, rs_out, off < map_bytes ? off : OOB, 0, C1_ST_AUX);
        asm volatile("s_nop 2" : "+v"(od));                 // 128-bit store data: WAR hazard hipcc does not pad
      }
    }
  };

  typedef std::integral_constant<int, 0> S0;
  typedef std::integral_constant<int, 1> S1;
  typedef std::integral_constant<int, 2> S2;
  // prologue: tile 0 -> slots 0, 1, 2
  target(0);
  issue(S0{}, 0);
  issue(S1{}, 1);
  issue(S2{}, 2);
  for (int k = 0; k < cnt; ++k) {
    target(k + 1);
    stage(S0{});
    stage(S1{});
    stage(S2{});
    finish(k);
  }
  ROWS_VMWAIT(0);            // no LDS-DMA may land after the workgroup's LDS is released
}

}  // namespace

// classify()'s ONE_BY_ONE (conv_dma.hip)
bool is_1x1(const Args& a) {
  static const bool on = [] {
    const char* e = getenv("PAIF_CONV_DMA1X1");   // PAIF_CONV_DMA1X1=0: the persistent register-staged kernel (conv_bf16x3_ws) as before (A/B runs)
    const char* d = getenv("PAIF_CONV_DMA");      // PAIF_CONV_DMA=0: no LDS-DMA kernel anywhere
    return !(e && e[0] == '0') && !(d && d[0] == '0');
  }();
  // the form built: 3 sources, no residual maps, 32 output channels, 16-bit output; 32-bit byte offsets, and the out-of-range marker above
  // every one of them
  return on && a.kh == 1 && a.dil == 1 && a.cout == 32 && !a.in_relu && !a.out_f32 && a.nsrc == 3 && a.nres == 0 &&
         (long long)a.B * a.H * a.W * 64 < (1ll << 31);
}

int launch_1x1(const Args& a, hipStream_t st) {
  const long long px = (long long)a.B * a.H * a.W;
  const int ntiles = (int)((px + TP - 1) / TP);
  if (a.f16) hipLaunchKernelGGL(conv_h16_dma_1x1<2>, dim3(GRID), dim3(WAVES * 64), 0, st, a, ntiles, Prob{}, 0);
  else hipLaunchKernelGGL(conv_h16_dma_1x1<1>, dim3(GRID), dim3(WAVES * 64), 0, st, a, ntiles, Prob{}, 0);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    paif::set_error("conv2d(h16 dma 1x1): launch failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

// two problems of one geometry: the same grid, half of it per problem
int launch_1x1_pair(const Args& a, const Prob& p1, hipStream_t st) {
  const long long px = (long long)a.B * a.H * a.W;
  const int ntiles = (int)((px + TP - 1) / TP);
  if (a.f16) hipLaunchKernelGGL(conv_h16_dma_1x1<2>, dim3(GRID), dim3(WAVES * 64), 0, st, a, ntiles, p1, 1);
  else hipLaunchKernelGGL(conv_h16_dma_1x1<1>, dim3(GRID), dim3(WAVES * 64), 0, st, a, ntiles, p1, 1);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    paif::set_error("conv2d(h16 dma 1x1, pair): launch failed: %s", hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

}  // namespace paif_conv_dma
