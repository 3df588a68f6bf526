// Interface between the dense-conv dispatcher (conv_mfma.hip) and the LDS-DMA kernels (conv_dma.hip: 3x3, 7x7; conv_dma_1x1.hip: 1x1;
// conv_dma_rows.hip: 3x3 dilation 2 without an input activation).
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

// true if the kernel is built for this source / residual count and the tensors fit its 32-bit addressing
bool eligible(int nsrc, int nres, int B, int H, int W, float alpha);
bool eligible16(int nsrc, int nres, int B, int H, int W, float alpha);  // 3x3 with 16 output channels: one source, no residual maps
bool eligible7(int nsrc, int nres, int B, int H, int W, float alpha);   // the 7x7 form: one source, no residual maps
bool eligible_d2(int nsrc, int nres, int B, int H, int W, float alpha);  // 3x3 dilation 2 behind an input ReLU: one source, 1 or 3 residual maps
bool can_cpool(int nsrc, int nres, int kh, int cout, int dil);   // the instantiations that write Args::cpool
int launch(const Args& a, hipStream_t st);

// conv_dma_1x1.hip: the 1x1 over three 32-channel sources without residual maps (the folded decomposition conv) as a streaming kernel;
// launch() hands it every Args with kh == 1.  Switch: PAIF_CONV_DMA1X1=0 (read once).
bool eligible_1x1(int nsrc, int nres, int B, int H, int W);
int launch_1x1(const Args& a, hipStream_t st);

// conv_dma_rows.hip: the 3x3 dilation-2 conv over one 16-bit source without an input activation (0-3 residual maps, 16-bit output, or
// fp32 from fp16 sources; no fused ChannelPool) as a row-streaming kernel.  Taken from 32,768 strip-rows (B * H * ceil(W / 32)) and
// H >= 64.  Switch PAIF_CONV_DMA_ROWS, read per call: unset = that size rule, 0 = never, 1 = wherever the 32-bit addressing holds.
bool eligible_rows(int nsrc, int nres, int in_relu, int cpool, int f16, int out_f32, int B, int H, int W);
int launch_rows(const Args& a, hipStream_t st);

}  // namespace paif_conv_dma
