"""U2Fusion baseline -- MI355X-native counterpart of the reference's fusion_model/U2Fusion.py: same constructor, forward signature,
module tree and state_dict keys (a checkpoint of the reference class loads with strict=True); forward and the reverse pass (input
gradients) launch the kernels of csrc/u2fusion.hip, one launch per layer, the eight wide convs and their transposes on the f32 matrix
instruction over one 264-channel NHWC slab.

The composite protocol, what is not built and the settings that do not apply: fusion_model/_native.py.  Built: fp32 planes of any size.
Not built either: the reference's `features_grad` helper."""
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache
from ._native import NativeFusion


def _conv_block(cin, cout):
    """fusion_model/U2Fusion.py:78-90 with act_type='lrelu', norm_type=None: Sequential(Conv2d 3x3 pad 1, LeakyReLU(0.2))."""
    return nn.Sequential(nn.Conv2d(cin, cout, 3, stride=1, padding=1), nn.LeakyReLU(negative_slope=0.2, inplace=True))


class DenseLayer(nn.Module):
    """fusion_model/U2Fusion.py:91-99 -- a parameter container here: U2Fusion's kernels append the layer's map to the concat slab."""

    def __init__(self, num_channels, growth):
        super().__init__()
        self.conv = _conv_block(num_channels, growth)


class U2Fusion(NativeFusion):
    """fusion_model/U2Fusion.py:102-125."""
    NAME = "U2Fusion"
    TAPED = ("cat", "s1", "s2", "s3")

    def __init__(self):
        super().__init__()
        self.num_channels = 2
        self.num_features = 44
        self.growth = 44
        self.conv_1 = _conv_block(self.num_channels, self.num_features)
        modules = []
        for _ in range(5):
            modules.append(DenseLayer(self.num_features, self.growth))
            self.num_features += self.growth
        self.dense_layers = nn.Sequential(*modules)
        self.sub = nn.Sequential(_conv_block(self.num_features, 128), _conv_block(128, 64), _conv_block(64, 32),
                                 nn.Conv2d(32, 1, kernel_size=3, stride=1, padding=1), nn.Tanh())
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _convs(self):
        """The ten Conv2d in layer order."""
        return [self.conv_1[0]] + [d.conv[0] for d in self.dense_layers] + [self.sub[0][0], self.sub[1][0], self.sub[2][0], self.sub[3]]

    def _pack(self):
        convs = [(c.weight, c.bias) for c in self._convs()]
        params = [t for c in convs for t in c]
        return self._packs.get("u2fusion", params, lambda: ops.u2fusion_pack(convs))

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, x_over, x_under):
        """fusion_model/U2Fusion.py:120-125 -> the fused plane [B,1,H,W] in tanh range."""
        return self._gate(x_over, x_under)

    def _run(self, x_over, x_under, tape):
        (cat, s1, s2, s3), fused = ops.u2fusion_forward(x_over, x_under, self._pack())
        if tape is not None:
            tape.update(cat=cat, s1=s1, s2=s2, s3=s3, out=fused)   # the nine maps and the fused plane: nothing is recomputed
        return fused

    @staticmethod
    def _map_list(cat, s1, s2, s3):
        """The nine LeakyReLU maps in layer order (conv_1, dense_layers.0..4: 44 channels each; sub.0..2: 128, 64, 32) as NHWC views."""
        return [cat[..., 44 * k:44 * (k + 1)] for k in range(6)] + [s1, s2, s3]

    def _reverse(self, d_fused, tape):
        """d/d(fused) -> (d/d(x_over), d/d(x_under)); inside the composite x_over is the infrared plane, x_under the visible Y."""
        return ops.u2fusion_backward(tape["cat"], tape["s1"], tape["s2"], tape["s3"], tape["out"], d_fused, self._pack())
