// Interface between the dense-conv dispatcher (conv_mfma.hip) and the LDS-DMA kernels: 16-bit maps (bf16 / fp16), plain 16-bit weights.
// The dispatcher fills an Args per launch and asks classify() which form, if any, is built for it; launch() runs that form.
#pragma once
#include <hip/hip_runtime.h>

namespace paif_conv_dma {

struct Args {
  const void* src[3];   // NHWC-32 bf16 maps (the virtual concat)
  const void* res[3];   // NHWC-32 bf16 residual maps
  const void* wpk;      // split-bf16 weight pack [src][tap][ks][hi|lo][64 lanes][8 bf16]: the hi halves are used
  const float* scale;   // per-cout (NULL = 1)
  const float* shift;   // per-cout (NULL = 0)
  const float* prelu;   // 1 float (act == 1)
  void* out;            // NHWC-32 bf16
  float alpha;
  int nsrc, nres, act, kh;   // kh: 3 or 7
  int cout;                  // 32, or 16 (3x3, one source, no residual maps)
  int B, H, W, reverse;
  float* cpool;              // optional: fused ChannelPool of the output (paif_conv_desc.cpool); built for (3 sources, 1 or 3 residual maps)
  int f16;                   // 1: the maps and weights are IEEE fp16 (PAIF_ST_F16 / PAIF_CONV_F16; the fp16 hi pieces of the F16X2 pack), else bf16
  int dil;                   // 1, or 2 (3x3, one source, input ReLU: the composed DilConv)
  int in_relu;               // 1: ReLU on the source as it is read (dilation 2 only)
  int out_f32;               // 1: `out` is fp32 (fp16 sources and residual maps; conv_dma_rows.hip only)
};

// The forms.  Each kernel file holds its own part of the rule and reads its own switches:
//   TILE        conv_dma.hip: persistent 8x32-tile kernels.  3x3 dilation 1 (1-3 sources, 0-3 residual maps, one source at most one; 16 output
//               channels with one source and no residual map), 7x7 (one source, no residual maps), 3x3 dilation 2 behind an input ReLU (one
//               source, 1 or 3 residual maps); alpha > 0; 1,024 to 32,768 tiles, B < 1024, 2^31 bytes per map.  Switches PAIF_CONV_DMA=0
//               (no LDS-DMA kernel anywhere), PAIF_CONV_DMA_D2=0 (the dilation-2 form), read once.
//   ONE_BY_ONE  conv_dma_1x1.hip: the 1x1 over three sources without residual maps (the folded decomposition conv) as a streaming kernel;
//               2^31 bytes per map.  Switch PAIF_CONV_DMA1X1=0, read once.
//   ROWS        conv_dma_rows.hip: the 3x3 dilation-2 conv over one source without an input activation (0-3 residual maps, 16-bit output, or
//               fp32 from fp16 sources; no fused ChannelPool) as a row-streaming kernel.  Taken from 32,768 strip-rows (B * H * ceil(W / 32))
//               and H >= 64.  Switch PAIF_CONV_DMA_ROWS, read per call: unset = that size rule, 0 = never, 1 = wherever the 32-bit addressing holds.
enum Form { NONE, TILE, ONE_BY_ONE, ROWS };

// The PAIR form: one launch runs two problems of one geometry (Args::B, H, W, source and residual counts, activation kind, format,
// tile order are common); what differs per problem is this block.  The kernels that have it take the second problem's block as a
// further kernel argument: a workgroup of the second half (of every XCD's workgroups in the tile kernel, of the grid in the 1x1)
// copies it over its Args before anything else -- scalar moves of kernel arguments, nothing inside a stage or tile loop.
struct Prob {
  const void* src[3];
  const void* res[3];
  const void* wpk;
  const float* scale;
  const float* shift;
  const float* prelu;
  void* out;
  float alpha;
};
// the forms with a pair kernel: ONE_BY_ONE; TILE 3x3 dilation 1 with 32 output channels and no fused ChannelPool for (sources, residual
// maps) = (1, 0), (2, 0), (3, 1), up to 16,384 tiles per problem (the tile table holds 128 tiles of a workgroup, a problem has 128 workgroups)
bool pair_capable(const Args& a);
int launch_pair(const Args& a0, const Args& a1, hipStream_t st);   // both pair_capable() and alike in everything but Prob's fields (the caller checks)
Form classify(const Args& a);
bool can_cpool(const Args& a);             // the TILE instantiations that write Args::cpool
int launch(const Args& a, hipStream_t st);   // the form classify() names; PAIF_ENOSUP for NONE

}  // namespace paif_conv_dma
