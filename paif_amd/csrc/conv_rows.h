// What the LDS-DMA convs share.  The PRIMITIVES (types, the buffer-descriptor constants, the inline-asm memory operations, dma16) serve all
// four files: conv_dma.hip, conv_dma_1x1.hip, conv_dma_rows.hip, conv_eca_rows.hip.  The rest is the ROW-STREAMING BODY of the last two
// (conv_dma_1x1.hip takes its operand swizzle and park step):
//   * a wave walks a RUN of consecutive rows of one 32-column strip downward and shares nothing with any other wave: a wave-private LDS ring
//     with a park buffer behind it, no s_barrier anywhere, so a wave may leave on its own.  A run costs one warm-up row at each end;
//   * a ring slot is one source row piece, (32 + 2 DIL) pixels x 64 B, fetched by 3 DMA instructions (buffer_load_dwordx4 ... lds; the
//     lanes past the last pixel are dead); 5 slots: 3 resident rows, 2 in flight.  Two workgroups of 4 waves per CU (the B operand is
//     72 registers): 8 waves x 19 KB = 152 KB of LDS;
//   * the 16-byte chunk a lane fetches is XOR-swizzled on the SOURCE side (the DMA writes LDS linearly in lane order, so any permutation
//     of what is fetched is free): the A-operand ds_read_b128 of 32 consecutive pixels at column shifts 0, DIL, 2 DIL is conflict-free;
//     zero padding is the buffer descriptor's range check;
//   * the vector-memory pattern of a step is fixed (dead accesses carry an out-of-range offset), so every s_waitcnt vmcnt(N) is a
//     compile-time count of YOUNGER LOADS (stores do not retire in order with loads, conv_dma.hip Sched); every LDS access is inline
//     asm (hipcc drains vmcnt in front of every LDS access it can see while an LDS-DMA is in flight), and a register an asm statement
//     loads is waited for, as a "+v" operand of the s_waitcnt, in the block that loads it; a 128-bit buffer store is followed by
//     `s_nop 2` on its data registers (a WAR hazard hipcc does not pad);
//   * arithmetic: paif::mfma16<F> 32x32x16, tap = dy * 3 + dx ascending, k-step inner, fp32 accumulation from zero.
// A new row-streaming kernel supplies its halo (DIL), its run decoding (which image rows a run walks), the hooks of conv_row() and its
// epilogue behind park_transpose(); everything below it takes as it is.
#pragma once
#include <stdint.h>

#include <type_traits>

#include "paif_common.h"

namespace paif_rows {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned RSRC_W3 = 0x00020000u;
constexpr unsigned OOB = 0x80000000u;         // a byte offset no map reaches (checked at launch): the hardware returns 0 / drops the store

#define ROWS_VMWAIT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define ROWS_RD128(dst, addr, off) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(off) : "memory")
#define ROWS_WR32(addr, val, off) asm volatile("ds_write_b32 %0, %1 offset:%2" ::"v"(addr), "v"(val), "n"(off) : "memory")
#define ROWS_WR128(addr, val, off) asm volatile("ds_write_b128 %0, %1 offset:%2" ::"v"(addr), "v"(val), "n"(off) : "memory")
// s_waitcnt lgkmcnt(n) on the registers that the LDS reads in front of it load: n = the LDS operations issued BEHIND those reads
// (LDS operations of a wave complete in order)
#define ROWS_LGKMWAIT(n, ...) asm volatile("s_waitcnt lgkmcnt(%[cnt])" : __VA_ARGS__ : [cnt] "n"(n) : "memory")
#define ROWS_FRAGS(A, b) "+v"(A[b][0][0]), "+v"(A[b][0][1]), "+v"(A[b][1][0]), "+v"(A[b][1][1]), "+v"(A[b][2][0]), "+v"(A[b][2][1])

// 16 B per lane HBM -> LDS, linear in lane order from lds_off.  AUX: cache policy (0 default, 2 streaming)
template <int AUX>
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned lds_off) {
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(uintptr_t)lds_off, 16, voff, 0, 0, AUX);
}

constexpr int PARK = 32 * 32 * 4;             // per-wave [32 px][32 ch] fp32 transposition buffer (one accumulator at a time)

// ---- the ring of one wave, by halo width (= dilation) ----
template <int DIL>
struct Ring {
  static constexpr int RW = 32;                        // output columns of a strip
  static constexpr int RWH = RW + 2 * DIL;             // source columns of a row piece
  static constexpr int DPS = 3;                        // DMA instructions per row piece (64 lanes x 16 B each: 48 pixels, RWH live)
  static constexpr int SLOT = DPS * 1024;
  static constexpr int NSLOT = 5, PF = NSLOT - 3;      // ring slots: 3 resident rows + PF in flight
  static constexpr int WAVE_LDS = NSLOT * SLOT + PARK; // 19 KB: the park buffer behind the ring
  static constexpr int WAVES = 4;
  static constexpr int LDS_BYTES = WAVES * WAVE_LDS;   // 76 KB: two workgroups per CU
  static constexpr int MAX_WAVES = 2048;               // 2 workgroups on each of 256 CUs
  static_assert(2 * LDS_BYTES <= 160 * 1024, "two workgroups per CU do not fit LDS");
  static_assert(RWH * 4 <= DPS * 64, "DMA instructions do not cover the row piece");
};

// ---- lane arithmetic ----
// MACROS on purpose.  As __forceinline__ functions, however small, these change the order in which hipcc simplifies the lane arithmetic
// of the calling kernel and with it instruction selection, schedule and register allocation of the whole kernel (tried: 1,500 to 5,000
// differing instructions over the 12 row kernels), and the kernels built on this header sit at 240 registers with no room to lose.  A
// macro hands the compiler the tokens it had when each kernel carried its own copy.  The caller declares what a macro fills.
//
// byte offset, inside a row piece, of the logical 16-byte chunk `chunk` (8 channels) of piece column c: the physical chunk is
// chunk ^ ((c >> 2) & 3), so ds_read_b128 of 32 consecutive columns hits every 16-byte bank group equally often
#define ROWS_SWIZZLED(c, chunk) ((unsigned)((c) * 64 + (((chunk) ^ (((c) >> 2) & 3)) * 16)))
// DMA instruction i of a row piece moves chunk n = 64 i + l of the slot: piece column d_col[i] = n >> 2, and from byte d_rel[i] of the
// source row piece (the swizzle is on the source side: the DMA writes LDS linearly in lane order)
#define ROWS_DMA_GEOMETRY(DPS, l, d_col, d_rel)    \
  _Pragma("unroll") for (int i = 0; i < (DPS); ++i) { \
    const int n = 64 * i + (l), c = n >> 2;        \
    (d_col)[i] = c;                                \
    (d_rel)[i] = ROWS_SWIZZLED(c, n & 3);          \
  }
// A operand of output pixel p, horizontal tap dx, k-step ks: lane (pixel p, k half hh) reads piece column p + dx * DIL
#define ROWS_A_ADDRS(DIL, lds_w, p, hh, a_rd)                    \
  _Pragma("unroll") for (int dx = 0; dx < 3; ++dx)               \
    _Pragma("unroll") for (int ks = 0; ks < 2; ++ks) {           \
      const int c = (p) + (DIL) * dx;                            \
      (a_rd)[dx][ks] = (lds_w) + ROWS_SWIZZLED(c, 2 * ks + (hh)); \
    }
// park buffer at LDS byte `park`: where lane (p, hh) writes accumulator register r (+ ((r & 3) + 8 (r >> 2)) * 128), and where lane l
// re-reads in the store layout (+ it * 2048 (+ 16): pixel 16 it + (l >> 2), channels 8 (l & 3) ..)
#define ROWS_PARK_WR_ADDR(park, p, hh) ((park) + (unsigned)((4 * (hh) * 32 + (p)) * 4))
#define ROWS_PARK_RD_ADDR(park, l) ((park) + (unsigned)(((l) >> 2) * 128 + ((l) & 3) * 32))
// which of this lane's DMA chunks of a piece of the strip at column x0 lie inside the piece (RWH columns, halo DIL) and the image
#define ROWS_COL_OK(RWH, DIL, DPS, d_col, x0, W, colok) \
  _Pragma("unroll") for (int i = 0; i < (DPS); ++i) (colok)[i] = (d_col)[i] < (RWH) && (unsigned)((x0) - (DIL) + (d_col)[i]) < (unsigned)(W);
// byte offset of the row piece of map row `row` (= image * H + image row), strip column x0: the piece starts DIL columns to the left
#define ROWS_ROW_BYTE(DIL, row, W, x0) ((unsigned)((row) * (W) + (x0) - (DIL)) * 64u)
// The DMAs of one row piece at source byte rowb into ring slot `slot` of the ring at lds_w.  A dead row (outside the image or the run)
// keeps its place in the vector-memory queue: its mask is OR-ed in (a scalar OR, not a branch around the DMAs) and never added -- an
// offset added to OOB wraps back into the map.
#define ROWS_ISSUE_ROW(AUX, DPS, SLOT, rs_src, colok, d_rel, rowb, dead, lds_w, slot) \
  _Pragma("unroll") for (int i = 0; i < (DPS); ++i)                                   \
    paif_rows::dma16<AUX>(rs_src, ((colok)[i] ? (rowb) + (d_rel)[i] : paif_rows::OOB) | (dead), (lds_w) + (unsigned)((slot) * (SLOT) + i * 1024));
// B operand of a 3x3: bw[tap][k-step], lane (n = l & 31, k = 8 (l >> 5) + j) -- the hi halves of the pack [tap][ks][hi|lo][64 lanes][16 B]
#define ROWS_LOAD_BW(bw, wpk, l)                                                                                                             \
  {                                                                                                                                          \
    const __amdgpu_buffer_rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(wpk), 0, 9 * 2 * 2 * 1024, paif_rows::RSRC_W3); \
    _Pragma("unroll") for (int tap = 0; tap < 9; ++tap)                                                                                      \
      _Pragma("unroll") for (int ks = 0; ks < 2; ++ks)                                                                                       \
        (bw)[tap][ks] = __builtin_amdgcn_raw_buffer_load_b128(rs_w, (unsigned)(l) * 16u, ((tap * 2 + ks) * 2) * 1024, 0);                    \
  }

// the ring slots of step t, from cur = the slot of load t (the row above the output row): loads t + 1, t + 2, and the slot to fill =
// (t + 2 + PF) % NSLOT: the slot of load t - 1, read one step ago
template <int NSLOT>
struct Slots {
  int s1, s2, fill;
  __device__ __forceinline__ explicit Slots(int cur)
      : s1(cur + 1 >= NSLOT ? cur + 1 - NSLOT : cur + 1), s2(cur + 2 >= NSLOT ? cur + 2 - NSLOT : cur + 2), fill(cur == 0 ? NSLOT - 1 : cur - 1) {}
};

struct NoHook {
  __device__ __forceinline__ void operator()() const {}
};

// One output row: acc = the 18 products of the row pieces at ring byte offsets rb[0..2] (vertical taps 0..2), fragments double-buffered
// by vertical tap.  Hooks, for a kernel that works on the newest piece (rb[2]) while it is first used:
//   landed(): behind the 12 reads of taps 0 and 1 -- the wait for LDS reads the caller issued in front of this call (12 younger reads);
//   shadow(): VALU work free to interleave with the first six MFMAs;
//   mid():    MID_LDS LDS operations in front of the tap-2 reads (LDS operations complete in order: those reads see what mid() writes).
// The wait for tap 1 leaves the 6 tap-2 reads outstanding and, with them, nothing older: mid()'s operations sit between the tap-1 and
// the tap-2 reads, so the count that still covers tap 1 is 6 + MID_LDS.
template <int F, int MID_LDS = 0, class Landed = NoHook, class Shadow = NoHook, class Mid = NoHook>
__device__ __forceinline__ void conv_row(f32x16& acc, const unsigned (&a_rd)[3][2], const unsigned (&rb)[3], const u32x4 (&bw)[9][2],
                                         Landed landed = Landed(), Shadow shadow = Shadow(), Mid mid = Mid()) {
  u32x4 A[2][3][2];       // [buffer][dx][ks]: the fragments of one vertical tap
  auto read = [&](int buf, int dy) {
#pragma unroll
    for (int dx = 0; dx < 3; ++dx)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const unsigned ad = a_rd[dx][ks] + rb[dy];
        ROWS_RD128(A[buf][dx][ks], ad, 0);
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
  landed();
  ROWS_LGKMWAIT(6, ROWS_FRAGS(A, 0));
  __builtin_amdgcn_sched_barrier(0);
  mma(std::integral_constant<int, 0>{});
  shadow();
  __builtin_amdgcn_sched_barrier(0);
  mid();
  read(0, 2);
  ROWS_LGKMWAIT(6 + MID_LDS, ROWS_FRAGS(A, 1));
  __builtin_amdgcn_sched_barrier(0);
  mma(std::integral_constant<int, 1>{});
  __builtin_amdgcn_sched_barrier(0);
  ROWS_LGKMWAIT(0, ROWS_FRAGS(A, 0));
  __builtin_amdgcn_sched_barrier(0);
  mma(std::integral_constant<int, 2>{});
  __builtin_amdgcn_sched_barrier(0);
}

// ---- the park step: a finished accumulator [32 ch][32 px] through the wave's park buffer into the store layout ----
// MFMA result -> LDS-store data: wait states inline asm does not get
__device__ __forceinline__ void mfma_to_lds_wait() { asm volatile("s_nop 15\n\ts_nop 7" ::: "memory"); }
__device__ __forceinline__ void park_write(const f32x16& acc, unsigned a_pw) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const float v = acc[r];
    ROWS_WR32(a_pw, v, ((r & 3) + 8 * (r >> 2)) * 128);
  }
}
// tq[it][half]: pixel 16 it + (l >> 2), channels 8 (l & 3) + 4 half ..  (LDS operations of a wave complete in order: the writes are in)
__device__ __forceinline__ void park_read(u32x4 (&tq)[2][2], unsigned a_pr) {
  ROWS_RD128(tq[0][0], a_pr, 0);
  ROWS_RD128(tq[0][1], a_pr, 16);
  ROWS_RD128(tq[1][0], a_pr, 2048);
  ROWS_RD128(tq[1][1], a_pr, 2048 + 16);
}
#define ROWS_PARKED(tq) "+v"(tq[0][0]), "+v"(tq[0][1]), "+v"(tq[1][0]), "+v"(tq[1][1])
__device__ __forceinline__ void park_transpose(const f32x16& acc, unsigned a_pw, unsigned a_pr, u32x4 (&tq)[2][2]) {
  park_write(acc, a_pw);
  park_read(tq, a_pr);
  ROWS_LGKMWAIT(0, ROWS_PARKED(tq));
}

// ---- the swap step: the same transposition without LDS, for a PIXEL-PER-LANE accumulator ----
// Both operands of a 32x32x16 MFMA have the same fragment layout (lane (l & 31, 8 (l >> 5) + j)), so which of the two maps is "lane =
// l & 31" in the RESULT is the order of the two arguments and nothing else:
//   mfma16<F>(pixels, weights, acc): lane (c = l & 31, hh = l >> 5), register r = 4 g + i holds pixel 8 g + 4 hh + i, channel c -- the
//                                    layout the park step takes ([px][ch] in LDS, park_write's address);
//   mfma16<F>(weights, pixels, acc): lane (p = l & 31, hh = l >> 5), register r = 4 g + i holds pixel p, channel 8 g + 4 hh + i -- the
//                                    transposed result, element for element the same dot product in the same k order.
// In the second layout a lane's 4 channels of a group g are 16 contiguous bytes of an fp32 map (byte 32 g + 16 hh of the pixel: an fp32
// output needs no swap), and packed to 16 bits they are 2 dwords, 8 bytes at byte 16 g + 8 hh.  For a pair of groups (2 k, 2 k + 1)
// one v_permlane32_swap per dword -- vdst = the dword of group 2 k, src = the dword of group 2 k + 1; the instruction exchanges lanes
// 32-63 of vdst with lanes 0-31 of src -- leaves in {vdst0, vdst1, src0, src1}
//   lanes  0-31: own group 2 k | the upper lane's group 2 k         = channels 16 k     .. 16 k + 7,  byte 32 k      of the pixel,
//   lanes 32-63: the lower lane's group 2 k + 1 | own group 2 k + 1 = channels 16 k + 8 .. 16 k + 15, byte 32 k + 16 of the pixel:
// one 16-byte store per pair, lane l at pixel l & 31, byte 32 k + 16 (l >> 5).  (The other operand order, or + 8 for the upper half,
// gives a wrong image, not a fault.)  The swap is its own inverse: 16 bytes LOADED at that place (a residual map in the stored layout)
// become {group 2 k, group 2 k + 1} of the lane's own channels by half_swap(v[0], v[2]), half_swap(v[1], v[3]).
// The builtin, not inline asm: hipcc pads the VALU-write -> permlane-read hazard.
__device__ __forceinline__ void half_swap(unsigned& lo, unsigned& hi) {
  const auto r = __builtin_amdgcn_permlane32_swap(lo, hi, false, false);
  lo = r[0];
  hi = r[1];
}
// {packed group 2 k, packed group 2 k + 1} of the lane's pixel -> the 16 bytes the lane stores; and back: 16 bytes loaded in the stored
// layout -> {group 2 k, group 2 k + 1} of the lane's own channels
__device__ __forceinline__ u32x4 swap_unpack(u32x4 v) {
  unsigned a = v.x, b = v.y, c = v.z, d = v.w;
  half_swap(a, c);
  half_swap(b, d);
  const u32x4 o = {a, b, c, d};
  return o;
}
// The two swapped pieces of a pixel row (q0: bytes 0-31 of the 32 pixels, lane l at pixel l & 31, byte 16 (l >> 5); q1: bytes 32-63)
// -> whole 64-byte pixels per store instruction.  v_permlane16_swap exchanges the odd 16-lane rows of vdst with the even rows of src;
// with vdst = q0 and src = q1, dword by dword, row r of the wave then holds
//   q0: pixel l & 15,        byte 32 (r & 1) + 16 (r >> 1)        q1: pixel 16 + (l & 15), the same bytes:
// 16 pixels x 64 B per store, the lines a store of the park epilogue writes.
__device__ __forceinline__ void line_swap(u32x4& q0, u32x4& q1) {
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    unsigned a = q0[d], b = q1[d];
    const auto r = __builtin_amdgcn_permlane16_swap(a, b, false, false);
    q0[d] = r[0];
    q1[d] = r[1];
  }
}
// one 16-bit pair, converted as f32_to_h4<F> converts each of its two pairs
template <int F>
__device__ __forceinline__ unsigned f32_to_h2(float a, float b) {
  return paif::f32_to_h4<F>(make_float4(a, b, 0.f, 0.f)).x;
}
// the lane's 16 epilogue constants in accumulator-register order: channel 8 (r >> 2) + 4 hh + (r & 3)
#define ROWS_ACC_CHANNEL(r, hh) (8 * ((r) >> 2) + 4 * (hh) + ((r) & 3))

// ---- host side ----
// `total` units in runs of at least min_run on at most max_waves waves: wave g owns [g * run, (g + 1) * run)
struct Partition {
  int run, waves;
  Partition(int total, int min_run, int max_waves) {
    const int per = (total + max_waves - 1) / max_waves;
    run = per > min_run ? per : min_run;
    waves = (total + run - 1) / run;
  }
};
constexpr int MIN_RUN_ROWS = 16;   // rows per wave at least: the two warm-up rows cost at most 1/8
// the size rule: runs of at least MIN_RUN_ROWS rows on every one of the MAX_WAVES waves, and chains long enough to hold them
inline bool fills_chip(int B, int H, int W) {
  typedef Ring<1> R;
  return H >= 64 && (long long)B * H * ((W + R::RW - 1) / R::RW) >= (long long)MIN_RUN_ROWS * R::MAX_WAVES;
}

}  // namespace paif_rows
