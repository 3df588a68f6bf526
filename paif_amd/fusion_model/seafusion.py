"""SeAFusion baseline -- MI355X-native counterpart of the reference's fusion_model/SeaFusion.py: same constructor, forward signature,
module tree and state_dict keys (72 entries; a checkpoint of the reference class loads with strict=True); forward and the reverse pass
(input gradients) launch the kernels of csrc/seafusion.hip, 22 launches each, the 3x3 and 1x1 convs and their transposes on the f32
matrix instruction over NHWC slabs (csrc/conv_slab.h).

Three things of the reference are kept as they are: the decoder's BatchNorm modules exist (and load) but are never applied, in .eval()
and .train() alike; the Sobel filters are parameters -- initialised to the stencil, read from the weight pack like any other weight; and
inside the composite models the INFRARED plane enters `image_vis` (Network_MM_CompModel calls forward(ir[:, 0:1], Y[:, 0:1])).

The composite protocol, what is not built and the settings that do not apply: fusion_model/_native.py.  Built: fp32 planes of any size."""
import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache
from ._native import NativeFusion


# ---- the reference's member classes, as parameter containers: SeaFusion's kernels do the arithmetic ---------------------------------
class ConvBnLeakyRelu2d(nn.Module):
    """fusion_model/SeaFusion.py:7-16 -- `bn` is owned and never applied."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, stride=1, dilation=1, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                              groups=groups)
        self.bn = nn.BatchNorm2d(out_channels)


class ConvBnTanh2d(nn.Module):
    """fusion_model/SeaFusion.py:18-24 -- `bn` is owned and never applied."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, stride=1, dilation=1, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                              groups=groups)
        self.bn = nn.BatchNorm2d(out_channels)


class ConvLeakyRelu2d(nn.Module):
    """fusion_model/SeaFusion.py:26-35."""

    def __init__(self, in_channels, out_channels, kernel_size=3, padding=1, stride=1, dilation=1, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                              groups=groups)


class Sobelxy(nn.Module):
    """fusion_model/SeaFusion.py:37-51: two depthwise 3x3 convs without bias, initialised to the Sobel stencil and its transpose."""

    def __init__(self, channels, kernel_size=3, padding=1, stride=1, dilation=1, groups=1):
        super().__init__()
        sobel_filter = np.array([[1, 0, -1], [2, 0, -2], [1, 0, -1]])
        self.convx = nn.Conv2d(channels, channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                               groups=channels, bias=False)
        self.convx.weight.data.copy_(torch.from_numpy(sobel_filter))
        self.convy = nn.Conv2d(channels, channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                               groups=channels, bias=False)
        self.convy.weight.data.copy_(torch.from_numpy(sobel_filter.T))


class Conv1(nn.Module):
    """fusion_model/SeaFusion.py:53-58."""

    def __init__(self, in_channels, out_channels, kernel_size=1, padding=0, stride=1, dilation=1, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding, stride=stride, dilation=dilation,
                              groups=groups)


class DenseBlock(nn.Module):
    """fusion_model/SeaFusion.py:60-70."""

    def __init__(self, channels):
        super().__init__()
        self.conv1 = ConvLeakyRelu2d(channels, channels)
        self.conv2 = ConvLeakyRelu2d(2 * channels, channels)


class RGBD(nn.Module):
    """fusion_model/SeaFusion.py:72-84."""

    def __init__(self, in_channels, out_channels):
        super().__init__()
        self.dense = DenseBlock(in_channels)
        self.convdown = Conv1(3 * in_channels, out_channels)
        self.sobelconv = Sobelxy(in_channels)
        self.convup = Conv1(in_channels, out_channels)


class SeaFusion(NativeFusion):
    """fusion_model/SeaFusion.py:86-125."""
    NAME = "SeaFusion"
    SHAPE_NOTE = " (image_vis[:, :1] and a one-channel image_ir)"

    def __init__(self):
        super().__init__()
        vis_ch = [16, 32, 48]
        inf_ch = [16, 32, 48]
        output = 1
        self.vis_conv = ConvLeakyRelu2d(1, vis_ch[0])
        self.vis_rgbd1 = RGBD(vis_ch[0], vis_ch[1])
        self.vis_rgbd2 = RGBD(vis_ch[1], vis_ch[2])
        self.inf_conv = ConvLeakyRelu2d(1, inf_ch[0])
        self.inf_rgbd1 = RGBD(inf_ch[0], inf_ch[1])
        self.inf_rgbd2 = RGBD(inf_ch[1], inf_ch[2])
        self.decode4 = ConvBnLeakyRelu2d(vis_ch[2] + inf_ch[2], vis_ch[1] + vis_ch[1])
        self.decode3 = ConvBnLeakyRelu2d(vis_ch[1] + inf_ch[1], vis_ch[0] + inf_ch[0])
        self.decode2 = ConvBnLeakyRelu2d(vis_ch[0] + inf_ch[0], vis_ch[0])
        self.decode1 = ConvBnTanh2d(vis_ch[0], output)
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _convs(self):
        """The thirty Conv2d in paif_amd.synthetic.SEAFUSION_CONVS order."""
        out = []
        for stem, r1, r2 in ((self.vis_conv, self.vis_rgbd1, self.vis_rgbd2), (self.inf_conv, self.inf_rgbd1, self.inf_rgbd2)):
            out.append(stem.conv)
            for r in (r1, r2):
                out += [r.dense.conv1.conv, r.dense.conv2.conv, r.convdown.conv, r.sobelconv.convx, r.sobelconv.convy, r.convup.conv]
        return out + [self.decode4.conv, self.decode3.conv, self.decode2.conv, self.decode1.conv]

    def _pack(self):
        convs = [(c.weight, c.bias) for c in self._convs()]
        params = [t for c in convs for t in c if t is not None]
        return self._packs.get("seafusion", params, lambda: ops.seafusion_pack(convs))

    @staticmethod
    def _first_channel(image_vis):
        """image_vis[:, :1] of the reference: any channel count >= 1."""
        if image_vis.dim() == 4 and image_vis.shape[1] > 1:
            return image_vis[:, 0:1, :, :]
        return image_vis

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, image_vis, image_ir):
        """fusion_model/SeaFusion.py:105-125 -> the fused plane [B,1,H,W] in (0, 1)."""
        return self._gate(self._first_channel(image_vis), image_ir)

    def _run(self, x_vis, x_inf, tape):
        maps, fused = ops.seafusion_forward(x_vis, x_inf, self._pack())
        if tape is not None:
            tape.update(maps=maps, out=fused)   # every map, the sign tapes and the fused plane: nothing is recomputed
        return fused

    @staticmethod
    def _map_list(maps):
        """The 21 taped maps in forward order as NHWC views: per stream (vis, inf) the first conv's map (16), RGBD1's conv1, conv2 and
        |convx| + |convy| (16 each), RGBD1's output (32), RGBD2's conv1, conv2, |convx| + |convy| (32 each) and output (48); then decode4,
        decode3, decode2 (64, 32, 16): 592 channels."""
        out = []
        for s in range(2):
            s1, s2 = maps["slab1"][s], maps["slab2"][s]
            out += [s1[..., 16 * k:16 * (k + 1)] for k in range(4)] + [s2[..., 32 * k:32 * (k + 1)] for k in range(4)]
            out.append(maps["enc"][..., 48 * s:48 * (s + 1)])
        return out + [maps["dec4"], maps["dec3"], maps["dec2"]]

    def _features(self, image_vis, image_ir):
        return super()._features(self._first_channel(image_vis), image_ir)

    def _reverse(self, d_fused, tape):
        """d/d(fused) -> (d/d(image_vis), d/d(image_ir)): inside the composite, where the infrared plane enters image_vis (the vis_*
        stream) and Y enters image_ir (the inf_* stream), (d/d(ir), d/d(Y))."""
        return ops.seafusion_backward(tape["maps"], tape["out"], d_fused, self._pack())
