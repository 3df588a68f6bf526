"""The hand-designed fusion network -- MI355X-native counterpart of the reference's core/model_fusion_auto.py:118-188: classes DRDB and
Fusion_Network with the reference's constructor signatures, module tree and state_dict keys (31 entries for Fusion_Network: 15 convs with
weight and bias, and relu.weight; a checkpoint of the reference class loads with strict=True).  The constructor's print is not reproduced.
Forward and the reverse pass (input gradients) launch the kernels of csrc/drdb.hip: the dilation-2 3x3 and the 1x1 convs and their
transposes on the f32 matrix instruction over one NHWC slab per DRDB (csrc/conv_slab.h); the clamp and the batch min / max normalisation
are the plane kernels of csrc/object_glue.hip.

THE TAIL.  fused = (c - min c) / (max c - min c) with c = clamp(f, 0, 1) and min, max over the WHOLE [B,1,H,W] tensor: the output of a
sample depends on the other samples of its batch, forward and reverse.  When max c == min c the reference divides by zero, and so does
this code.  The reverse pass follows torch: the gradient of an extremum is spread evenly over the elements of c that attain it and
reaches f only where the clamp passes (0 <= f <= 1).  That even split comes with the plane kernels; the fixtures hold no exact tie among
unclamped pixels, so it is not covered by the tests of this network.

The composite protocol, what is not built and the settings that do not apply: fusion_model/_native.py.  Built: fp32 planes of any size;
DRDB alone at in_ch = 64, growth_rate = 32.  The PReLU slope is read on the host when the weights are packed (never inside a graph
capture) and must be >= 0: the reverse pass reads the branch off the taped output."""
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache, grad_anchor
from ._native import NativeFusion, need_device

_NO_WGRAD_DRDB = "DRDB: parameter gradients (training the block) are not built"
_FREEZE = (" -- freeze the parameters (requires_grad_(False)), or run under ops.no_param_grads() / torch.no_grad() for input gradients")


class DRDB(nn.Module):
    """core/model_fusion_auto.py:118-158.  Inside Fusion_Network a parameter container; alone, a [B,64,H,W] -> [B,64,H,W] map with input
    gradients (in_ch = 64, growth_rate = 32 only)."""

    def __init__(self, in_ch=64, growth_rate=32):
        super().__init__()
        in_ch_ = in_ch
        for k in range(1, 6):
            setattr(self, "Dcov%d" % k, nn.Conv2d(in_ch_, growth_rate, 3, padding=2, dilation=2))
            in_ch_ += growth_rate
        self.conv = nn.Conv2d(in_ch_, in_ch, 1, padding=0)
        self._shape = (in_ch, growth_rate)
        self._packs = _PackCache()

    def _convs(self):
        return [getattr(self, "Dcov%d" % k) for k in range(1, 6)] + [self.conv]

    def _pack(self):
        convs = [(c.weight, c.bias) for c in self._convs()]
        params = [t for c in convs for t in c]
        return self._packs.get("drdb_block", params, lambda: ops.drdb_pack([None] + convs + [None] * 8))

    def _check(self, x):
        if self._shape != (64, 32):
            raise NotImplementedError("DRDB: only in_ch = 64, growth_rate = 32 (the form Fusion_Network uses) is built, got %s" % (self._shape,))
        need_device(x)
        if x.dtype != torch.float32:
            raise TypeError("DRDB: an fp32 map is expected, got %s" % x.dtype)
        if x.dim() != 4 or x.shape[1] != 64:
            raise ValueError("DRDB: a [B,64,H,W] map is expected, got %s" % (tuple(x.shape),))

    def forward(self, x):
        if ops.want_param_grads(self):
            raise NotImplementedError(_NO_WGRAD_DRDB + _FREEZE)
        self._check(x)
        if torch.is_grad_enabled() and x.requires_grad:
            return _DRDBFn.apply(x, self, grad_anchor(x.device))
        with torch.no_grad():
            return ops.drdb_block_forward(x, self._pack())[1]


class _DRDBFn(torch.autograd.Function):
    """Autograd node of a DRDB alone: hand-written reverse pass, input gradient only."""

    @staticmethod
    def forward(ctx, x, module, anchor):
        maps, out = ops.drdb_block_forward(x.detach(), module._pack())
        ctx.maps, ctx.module = maps, module
        return out

    @staticmethod
    def backward(ctx, d_out):
        d_x = ops.drdb_block_backward(ctx.maps, d_out.contiguous(), ctx.module._pack())
        ctx.maps = None
        return d_x, None, None


class Fusion_Network(NativeFusion):
    """core/model_fusion_auto.py:159-188."""
    NAME = "Fusion_Network"
    TRAINING = "training the network"
    SHAPE_NOTE = " (channel 0 of ir and of vis)"

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(2, 64, 3, padding=1)
        self.DRDB1 = DRDB(in_ch=64)
        self.DRDB2 = DRDB(in_ch=64)
        self.conv2 = nn.Conv2d(64, 32, 3, padding=1)
        self.conv21 = nn.Conv2d(32, 1, 3, padding=1)
        self.relu = nn.PReLU()
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _convs(self):
        """The fifteen Conv2d in paif_amd.synthetic.DRDB_CONVS order."""
        return [self.conv1] + self.DRDB1._convs() + self.DRDB2._convs() + [self.conv2, self.conv21]

    def _pack(self):
        convs = [(c.weight, c.bias) for c in self._convs()]
        params = [t for c in convs for t in c] + [self.relu.weight]       # all 31 tensors: the slope is part of the pack
        return self._packs.get("drdb", params, lambda: ops.drdb_pack(convs, self.relu.weight))

    @staticmethod
    def _first_channel(x):
        """x[:, 0:1] of the reference: any channel count >= 1."""
        if x.dim() == 4 and x.shape[1] > 1:
            return x[:, 0:1, :, :]
        return x

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, ir, vis):
        """core/model_fusion_auto.py:170-188 -> the fused plane [B,1,H,W] in [0, 1], normalised over the batch."""
        return self._gate(self._first_channel(ir), self._first_channel(vis))

    def _run(self, ir, vis, tape):
        maps, fused = ops.drdb_forward(ir, vis, self._pack())
        if tape is not None:
            tape.update(maps=maps, out=fused)   # every map, r6, f before the clamp and (min, max): nothing is recomputed
        return fused

    @staticmethod
    def _map_list(maps):
        """The 17 taped maps in forward order as channel-last views: conv1's PReLU output (64); per DRDB x_1 .. x_5 (32 each), relu(x6)
        (64) and the block's output (64); conv2's PReLU output (32); f, conv21's PReLU output before the clamp (1): 673 channels."""
        s1, s2 = maps["slab"]
        out = [s1[..., 0:64]]
        for slab, r6, nxt in ((s1, maps["r6"][0], s2[..., 0:64]), (s2, maps["r6"][1], maps["f2"])):
            out += [slab[..., 64 + 32 * k:96 + 32 * k] for k in range(5)] + [r6, nxt]
        return out + [maps["c2"], maps["f"].permute(0, 2, 3, 1)]

    def _features(self, ir, vis):
        return super()._features(self._first_channel(ir), self._first_channel(vis))

    def _reverse(self, d_fused, tape):
        """d/d(fused) -> (d/d(ir), d/d(vis))."""
        return ops.drdb_backward(tape["maps"], d_fused, self._pack())
