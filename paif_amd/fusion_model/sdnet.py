"""SDNet baseline -- MI355X-native counterpart of the reference's fusion_model/SDNet.py: same constructor, forward signature and
state_dict keys (a checkpoint of the reference class loads with strict=True); forward and the reverse pass (input gradients) launch the
kernels of csrc/sdnet.hip, one launch per layer, both encoders in every launch, the dense convs on the f32 matrix instruction.

The composite protocol, what is not built and the settings that do not apply: fusion_model/_native.py.  Built: fp32 planes of any size.
The reference's `decom` and `conv51` .. `conv72` are parameter containers: its forward never touches them."""
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache
from ._native import NativeFusion

# (attribute, layer of ops.sdnet_pack, encoder) of the nine convs the forward uses
_USED = (("conv11", 0, 0), ("conv12", 0, 1), ("conv21", 1, 0), ("conv22", 1, 1), ("conv31", 2, 0), ("conv32", 2, 1),
         ("conv41", 3, 0), ("conv42", 3, 1), ("fuse", 4, 0))


class SDNet(NativeFusion):
    """fusion_model/SDNet.py:6-47."""
    NAME = "SDNet"
    TAPED = ("feat",)

    def __init__(self):
        super().__init__()
        act = nn.LeakyReLU
        self.conv11 = nn.Sequential(nn.Conv2d(1, 16, 5, 1, 2), act())
        self.conv12 = nn.Sequential(nn.Conv2d(1, 16, 5, 1, 2), act())
        self.conv21 = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), act())
        self.conv22 = nn.Sequential(nn.Conv2d(16, 16, 3, 1, 1), act())
        self.conv31 = nn.Sequential(nn.Conv2d(32, 16, 3, 1, 1), act())
        self.conv32 = nn.Sequential(nn.Conv2d(32, 16, 3, 1, 1), act())
        self.conv41 = nn.Sequential(nn.Conv2d(48, 16, 3, 1, 1), act())
        self.conv42 = nn.Sequential(nn.Conv2d(48, 16, 3, 1, 1), act())
        self.fuse = nn.Sequential(nn.Conv2d(128, 1, 1, 1, 0), nn.Tanh())
        # SDNet.py:22-31: the decomposition branch of the published training loss -- parameters only, forward never uses them
        self.decom = nn.Sequential(nn.Conv2d(1, 128, 1, 1, 0), act())
        self.conv51 = nn.Sequential(nn.Conv2d(128, 16, 3, 1, 1), act())
        self.conv52 = nn.Sequential(nn.Conv2d(128, 16, 3, 1, 1), act())
        self.conv61 = nn.Sequential(nn.Conv2d(16, 4, 3, 1, 1), act())
        self.conv62 = nn.Sequential(nn.Conv2d(16, 4, 3, 1, 1), act())
        self.conv71 = nn.Sequential(nn.Conv2d(4, 1, 3, 1, 1), nn.Tanh())
        self.conv72 = nn.Sequential(nn.Conv2d(4, 1, 3, 1, 1), nn.Tanh())
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _pack(self):
        convs = [(layer, enc, getattr(self, name)[0].weight, getattr(self, name)[0].bias) for name, layer, enc in _USED]
        params = [t for c in convs for t in c[2:]]
        return self._packs.get("sdnet", params, lambda: ops.sdnet_pack(convs))

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, x1, x2):
        """fusion_model/SDNet.py:33-47 -> the fused plane [B,1,H,W] in tanh range."""
        return self._gate(x1, x2)

    def _run(self, x1, x2, tape):
        feat, out = ops.sdnet_forward(x1, x2, self._pack())
        if tape is not None:
            tape.update(feat=feat, out=out)   # the eight maps and the fused plane: nothing is recomputed
        return out

    @staticmethod
    def _map_list(feat):
        """The eight LeakyReLU maps x11 .. x14, x21 .. x24 (SDNet.py:34-42) as NHWC views."""
        return [feat[e, l] for e in range(2) for l in range(4)]

    def _reverse(self, d_fused, tape):
        """d/d(fused) -> (d/d(x1), d/d(x2)); inside the composite x1 is the infrared plane, x2 the visible Y."""
        return ops.sdnet_backward(tape["feat"], tape["out"], d_fused, self._pack())
