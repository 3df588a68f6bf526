"""BFFusion baseline -- MI355X-native counterpart of the reference's fusion_model/BFFusion.py (class BFFR): same constructors, forward
signature, module tree and state_dict keys (386 entries, 1,717,409 parameters; a checkpoint of the reference class loads with
strict=True); forward and the reverse pass (input gradients) launch the kernels of csrc/bffusion.hip: every 3 x 3 and 1 x 1 conv with
>= 16 input channels and its transpose on the f32 matrix instruction over NHWC concat slabs (csrc/conv_slab.h), stem, head, pooling,
upsampling, the gate, LayerNorm and the channel attention's context reduction on the vector unit.

The network: two encoder streams (a 1 x 1 stem 1 -> 16 WITHOUT activation -- `ConvLayer(1, 16, 1, stride)` puts the stride into `is_last`
-- then four DenseBlocks with MaxPool2d(2, 2) between them), per level a FusionBlock_res of two SelfAttention blocks (reflection-padded
f_ConvLayers with BatchNorm and ReLU around a channel attention whose d x d context matrices are sums over all pixels of an image), a
UNet++ decoder of six ConvLayers over concats of fused and upsampled maps, and conv_out with tanh / 2 + 0.5.

BatchNorm is the EVAL-MODE one, folded into the weight pack on the device, for the 32 f_ConvLayers only: `ConvLayer.bn` exists in the
state_dict (8 modules) but the reference never applies it, so it loads and has no effect, and it is not part of the pack's key.  A forward
in .train() mode raises: batch-statistics BatchNorm is not built.  The used BatchNorms' four tensors and the LayerNorm affine are part of
the pack's key (an in-place change rebuilds the pack); the BatchNorm and LayerNorm eps floats are compared per call.

The composite calls the reference's forward(image_vis_y, image_ir) positionally as forward(ir[:, 0:1], Y[:, 0:1]): the infrared plane
runs through conv1_vi / DB*_vi (and attn2), Y through conv1_ir / DB*_ir (and attn1).

The composite protocol, what is not built and the settings that do not apply: fusion_model/_native.py.  Built: fp32 planes with
H, W >= 16 (the level-4 map is (H // 8) x (W // 8) and takes reflection padding by 1).  Not built either: .train() mode.  Sobelxy,
DenseBlock_light, conv1x1 and qkv_transform are carried as the reference carries them: names without a use."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache
from ._native import NativeFusion

_NO_TRAIN = ("BFFusion: training-mode BatchNorm (batch statistics) is not built -- call .eval(), as every reference flow does; the running "
             "statistics are not used in its place")
MIN_SIZE = 16


# ---- the reference's member classes, as parameter containers: BFFR's kernels do the arithmetic ----------------------------------------
class ConvLeakyRelu2d(nn.Module):
    """3 x 3 conv, zero pad 1, LeakyReLU 0.2."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, stride=1, dilation=1, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                              groups=groups)


class Sobelxy(nn.Module):
    """Depthwise Sobel pair; not used by BFFR."""

    def __init__(self, channels, kernel_size=3, padding=1, stride=1, dilation=1, groups=1):
        super().__init__()
        sobel = torch.tensor([[1., 0., -1.], [2., 0., -2.], [1., 0., -1.]])
        self.convx = nn.Conv2d(channels, channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                               groups=channels, bias=False)
        self.convx.weight.data.copy_(sobel)
        self.convy = nn.Conv2d(channels, channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                               groups=channels, bias=False)
        self.convy.weight.data.copy_(sobel.t())


class ConvLayer(nn.Module):
    """Reflection pad, conv, LeakyReLU 0.01 unless `is_last is False` fails; `bn` is a member the reference never applies."""

    def __init__(self, in_channels, out_channels, kernel_size, is_last=False):
        super().__init__()
        self.reflection_pad = nn.ReflectionPad2d(int(np.floor(kernel_size / 2)))
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size)
        self.bn = nn.BatchNorm2d(out_channels)
        self.is_last = is_last


class DenseBlock_light(nn.Module):
    """Two ConvLayers; not used by BFFR."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1):
        super().__init__()
        mid = int(in_channels / 2)
        self.denseblock = nn.Sequential(ConvLayer(in_channels, mid, kernel_size, stride), ConvLayer(mid, out_channels, 1, stride))


class DenseBlock(nn.Module):
    """conv1 c -> c and conv2 2c -> c over the concat so far (LeakyReLU 0.2), conv_down 1 x 1 3c -> out (LeakyReLU 0.1)."""

    def __init__(self, in_channels, out_channels, kernel_size):
        super().__init__()
        self.conv1 = ConvLeakyRelu2d(in_channels, in_channels, kernel_size=kernel_size)
        self.conv2 = ConvLeakyRelu2d(2 * in_channels, in_channels, kernel_size=kernel_size)
        self.conv_down = nn.Conv2d(3 * in_channels, out_channels, 1)


class ConvLayerLast(nn.Module):
    """Reflection pad, conv, tanh / 2 + 0.5."""

    def __init__(self, in_channels, out_channels, kernel_size, stride):
        super().__init__()
        self.reflection_pad = nn.ReflectionPad2d(int(np.floor(kernel_size / 2)))
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, stride)


class UpsampleReshape_eval(nn.Module):
    """Nearest x 2, then ReflectionPad2d([0, 1, 0, 1]) on the sides where the target is one larger."""

    def __init__(self):
        super().__init__()
        self.up = nn.Upsample(scale_factor=2)


def conv1x1(in_planes, out_planes, stride=1):
    """1 x 1 convolution without bias; not used by BFFR."""
    return nn.Conv2d(in_planes, out_planes, kernel_size=1, stride=stride, bias=False)


class qkv_transform(nn.Conv1d):
    """Conv1d for qkv_transform; not used by BFFR."""


class f_ConvLayer(nn.Module):
    """Reflection pad, conv, BatchNorm, ReLU."""

    def __init__(self, in_channels, out_channels, kernel_size, stride, is_last=False):
        super().__init__()
        self.reflection_pad = nn.ReflectionPad2d(int(np.floor(kernel_size / 2)))
        self.conv2d = nn.Conv2d(in_channels, out_channels, kernel_size, stride)
        self.batch_norm = nn.BatchNorm2d(out_channels)
        self.is_last = is_last


class SelfAttention(nn.Module):
    """conv_pre, channel attention (tokens = pixels, a d x d context per head and image, softmax over its rows), end_proj1, LayerNorm,
    ffn, skip + skip * x."""

    def __init__(self, dim, num_heads=4, qkv_bias=False, qk_scale=None):
        super().__init__()
        assert dim % num_heads == 0, f"dim {dim} should be divided by num_heads {num_heads}."
        self.conv_pre = nn.Sequential(f_ConvLayer(dim, dim, 3, 1), f_ConvLayer(dim, dim, 3, 1))
        self.ffn = nn.Sequential(f_ConvLayer(dim, dim, 3, 1), f_ConvLayer(dim, dim, 3, 1))
        self.norm1 = nn.LayerNorm(dim)
        self.dim = dim
        self.num_heads = num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.wq1 = nn.Linear(dim, dim, bias=qkv_bias)
        self.wk1 = nn.Linear(dim, dim, bias=qkv_bias)
        self.wv1 = nn.Linear(dim, dim, bias=qkv_bias)
        self.end_proj1 = nn.Linear(dim, dim)


class FusionBlock_res(nn.Module):
    """(attn1(x_ir) + attn2(x_vi)) / 2."""

    def __init__(self, channels, num_heads, index):
        super().__init__()
        self.attn1 = SelfAttention(channels, num_heads)
        self.attn2 = SelfAttention(channels, num_heads)


class BFFR(NativeFusion):
    """fusion_model/BFFusion.py, class BFFR."""
    NAME = "BFFusion"

    def __init__(self, device=None):
        super().__init__()
        self.device = device
        nb, heads = ops.BFF_NB, ops.BFF_HEADS
        self.pool = nn.MaxPool2d(2, 2)
        self.up = nn.Upsample(scale_factor=2)
        self.up_eval = UpsampleReshape_eval()
        for tag in ("vi", "ir"):
            setattr(self, "conv1_" + tag, ConvLayer(1, 16, 1, 1))     # the 1 lands in is_last: no activation
            setattr(self, "DB1_" + tag, DenseBlock(16, nb[0], 3))
            setattr(self, "DB2_" + tag, DenseBlock(nb[0], nb[1], 3))
            setattr(self, "DB3_" + tag, DenseBlock(nb[1], nb[2], 3))
            setattr(self, "DB4_" + tag, DenseBlock(nb[2], nb[3], 3))
        for l in range(4):
            setattr(self, "fusion_block%d" % (l + 1), FusionBlock_res(nb[l], heads[l], l))
        self.DB1_1 = ConvLayer(nb[0] + nb[1], nb[0], 3)
        self.DB2_1 = ConvLayer(nb[1] + nb[2], nb[1], 3)
        self.DB3_1 = ConvLayer(nb[2] + nb[3], nb[2], 3)
        self.DB1_2 = ConvLayer(nb[0] * 2 + nb[1], nb[0], 3)
        self.DB2_2 = ConvLayer(nb[1] * 2 + nb[2], nb[1], 3)
        self.DB1_3 = ConvLayer(nb[0] * 3 + nb[1], nb[0], 3)
        self.conv_out = ConvLayerLast(nb[0], 1, 1, 1)
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _attn(self, level, stream):
        """Stream 0 (the `_vi` modules) feeds attn2, stream 1 (the `_ir` modules) attn1."""
        fb = getattr(self, "fusion_block%d" % (level + 1))
        return fb.attn1 if stream else fb.attn2

    def _pack_spec(self):
        """-> (spec of ops.bffusion_pack, the tensors it holds = the pack's key, the eps floats)."""
        key, eps = [], []

        def cb(conv):
            key.extend((conv.weight, conv.bias))
            return conv.weight, conv.bias

        spec = dict(stem=[], dense=[], attn=[], dec=[])
        for tag in ("vi", "ir"):
            spec["stem"].append(cb(getattr(self, "conv1_" + tag).conv2d))
            row = []
            for l in range(4):
                db = getattr(self, "DB%d_%s" % (l + 1, tag))
                row.append(cb(db.conv1.conv) + cb(db.conv2.conv) + cb(db.conv_down))
            spec["dense"].append(row)
        for l in range(4):
            row = []
            for s in range(2):
                at = self._attn(l, s)
                convs = []
                for f in list(at.conv_pre) + list(at.ffn):
                    bn = f.batch_norm
                    convs.append(cb(f.conv2d) + (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps))
                    key.extend((bn.weight, bn.bias, bn.running_mean, bn.running_var))
                    eps.append(float(bn.eps))
                key.extend((at.wq1.weight, at.wk1.weight, at.wv1.weight, at.end_proj1.weight, at.end_proj1.bias, at.norm1.weight, at.norm1.bias))
                eps.append(float(at.norm1.eps))
                row.append(dict(convs=convs, wq=at.wq1.weight, wk=at.wk1.weight, wv=at.wv1.weight, wp=at.end_proj1.weight,
                                bp=at.end_proj1.bias, ln_w=at.norm1.weight, ln_b=at.norm1.bias, ln_eps=at.norm1.eps))
            spec["attn"].append(row)
        for name in ("DB1_1", "DB2_1", "DB1_2", "DB3_1", "DB2_2", "DB1_3"):     # ops.BFF_DEC order
            spec["dec"].append(cb(getattr(self, name).conv2d))
        spec["head"] = cb(self.conv_out.conv2d)
        return spec, key, tuple(eps)

    def _pack(self):
        spec, key, eps = self._pack_spec()
        for at in (self._attn(l, s) for l in range(4) for s in range(2)):
            if at.wq1.bias is not None or at.wk1.bias is not None or at.wv1.bias is not None:
                raise NotImplementedError("BFFusion: qkv_bias=True is not built (BFFR never sets it)")
        if self.__dict__.setdefault("_pack_eps", eps) != eps:    # Python floats on the modules, folded into the pack: a new cache
            self._packs, self._pack_eps = _PackCache(), eps
        return self._packs.get("bffusion", key, lambda: ops.bffusion_pack(spec))

    @classmethod
    def _check_planes(cls, x0, x1):
        super()._check_planes(x0, x1)
        if x0.shape[2] < MIN_SIZE or x0.shape[3] < MIN_SIZE:
            raise ValueError("BFFusion: H, W >= 16 are needed (the level-4 map is (H // 8) x (W // 8) and takes reflection padding by 1), "
                             "got [B,1,H,W] = %s" % (tuple(x0.shape),))

    def _check_mode(self):
        if self.training:
            raise NotImplementedError(_NO_TRAIN)

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, image_vis_y, image_ir):
        """-> the fused plane [B,1,H,W] in (0, 1).  image_vis_y runs through the `_vi` modules, image_ir through the `_ir` modules."""
        return self._gate(image_vis_y, image_ir)

    def _run(self, x0, x1, tape):
        maps, fused = ops.bffusion_forward(x0, x1, self._pack())
        if tape is not None:
            tape.update(maps=maps, out=fused)   # every map and the fused plane: nothing but the LayerNorm statistics is recomputed
        return fused

    @staticmethod
    def _map_list(maps):
        """The 94 taped maps in forward order as NHWC views.  Per stream (the `_vi` modules first) and level: the DenseBlock's conv1 and
        conv2 outputs and the block's output (24); per level and stream: p1, p2, qkv, y, z, f1, f2 of the attention block (56); the four
        fused maps; x1_1, x2_1, x1_2, x3_1, x2_2, x1_3 (6); then the eight context matrices [B,dim,d] as [B,1,dim,d]."""
        out = []
        for s in range(2):
            for l in range(4):
                c = ops.BFF_CIN[l]
                out += [maps["E"][s][l][..., c:2 * c], maps["E"][s][l][..., 2 * c:3 * c], maps["EN"][s][l]]
        for l in range(4):
            for s in range(2):
                out += [maps["A"][l][s][k] for k in ("p1", "p2", "qkv", "y", "z", "f1", "f2")]
        out += [maps["D"][l][..., ops.BFF_FOFF[l]:ops.BFF_FOFF[l] + ops.BFF_NB[l]] for l in range(4)]
        out += [maps["D"][lvl][..., off:off + m] for (lvl, _, _, _, _, off, m) in ops.BFF_DEC]
        return out + [maps["A"][l][s]["ctx"][:, None] for l in range(4) for s in range(2)]

    def _reverse(self, d_fused, tape):
        """d/d(fused) -> (d/d(image_vis_y), d/d(image_ir)): inside the composite, (d/d(ir), d/d(Y))."""
        return ops.bffusion_backward(tape["maps"], tape["out"], d_fused, self._pack())
