"""Fusion_Network2 -- MI355X-native counterpart of the reference's core/model_fusion_auto.py:227-260: the hand-designed network whose DRDB
features are mixed with two guidance feature maps through two SKFF gates.  The reference's constructor, module tree and state_dict keys
(41 entries: conv1, the two DRDB, conv2, relu.weight, skff and skff2 with four tensors each, conv3, conv4; a checkpoint of the reference
class loads with strict=True).  SKFF itself is operations_m.SKFF.

    x = PReLU(conv1(cat(ir, vis)));  f1 = DRDB1(x);  v1 = skff([f1, conv3(out1)]);  f2 = DRDB2(v1);  v2 = skff2([f2, conv4(out2)]);
    f = PReLU(conv2(v2));  fused = (f - min f) / (max f - min f)

with min and max over the WHOLE [B,1,H,W] tensor and no clamp: the output of a sample depends on the other samples of its batch, forward
and reverse.  When max f == min f the reference divides by zero, and so does this code.  The gradient of an extremum is spread evenly over
the elements that attain it, as torch's full-reduction min / max does.  One PReLU slope, `relu`, serves conv1 and conv2; it is read on the
host when the weights are packed (never inside a graph capture) and must be >= 0: the reverse pass reads the branch off the taped output.

A plain nn.Module with an autograd node of its own, not a NativeFusion: the composite models' forward_impl(ir, vis, inter, tape) has no
place for out1 / out2, and no composite of the reference constructs this network.  Forward and the reverse pass (gradients of ir, vis,
out1 and out2) launch the kernels of csrc/drdb.hip and csrc/skff.hip (ops.fn2_forward / ops.fn2_backward); the two transposed 1x1
launches are skipped when neither guidance map asks for a gradient.  Parameter gradients are not built."""
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import SKFF, _PackCache, grad_anchor
from ._native import need_device
from .drdb import DRDB, _FREEZE

_NO_WGRAD_FN2 = "Fusion_Network2: parameter gradients (training the network) are not built"


class Fusion_Network2(nn.Module):
    """core/model_fusion_auto.py:227-260."""

    def __init__(self):
        super().__init__()
        self.conv1 = nn.Conv2d(2, 64, 3, padding=1)
        self.DRDB1 = DRDB()
        self.DRDB2 = DRDB()
        self.conv2 = nn.Conv2d(64, 1, 3, padding=1)
        self.relu = nn.PReLU()
        self.skff = SKFF(64, 2)
        self.skff2 = SKFF(64, 2)
        self.conv3 = nn.Conv2d(64, 64, 1, padding=0)
        self.conv4 = nn.Conv2d(128, 64, 1, padding=0)
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _convs(self):
        """The sixteen Conv2d outside the gates in paif_amd.synthetic.FN2_CONVS order."""
        return [self.conv1] + self.DRDB1._convs() + self.DRDB2._convs() + [self.conv2, self.conv3, self.conv4]

    def _pack(self):
        convs = [(c.weight, c.bias) for c in self._convs()]
        params = [t for c in convs for t in c] + [self.relu.weight]
        # the gates' packs have their own cache entries (their own parameters); this one holds the current pair
        g1, g2 = self.skff._pack(), self.skff2._pack()
        pack = self._packs.get("fn2", params, lambda: ops.fn2_pack(convs, self.relu.weight, g1, g2))
        pack.skff, pack.skff2 = g1, g2
        return pack

    # ---- checks: device, then dtype, then shapes ----------------------------------------------------------------------------
    @staticmethod
    def _check(ir, vis, out1, out2):
        for t in (ir, vis, out1, out2):
            need_device(t)
        for t in (ir, vis, out1, out2):
            if t.dtype != torch.float32:
                raise TypeError("Fusion_Network2: fp32 tensors are expected, got %s" % t.dtype)
        if ir.dim() != 4 or ir.shape[1] != 1 or ir.shape != vis.shape:
            raise ValueError("Fusion_Network2: two [B,1,H,W] planes of one shape are expected (channel 0 of ir and of vis), got %s and %s"
                             % (tuple(ir.shape), tuple(vis.shape)))
        B, _, H, W = ir.shape
        if tuple(out1.shape) != (B, 64, H, W) or tuple(out2.shape) != (B, 128, H, W):
            raise ValueError("Fusion_Network2: out1 [B,64,H,W] and out2 [B,128,H,W] of the planes' size %s are expected, got %s and %s"
                             % ((B, H, W), tuple(out1.shape), tuple(out2.shape)))

    @staticmethod
    def _first_channel(x):
        """x[:, 0:1] of the reference: any channel count >= 1."""
        if x.dim() == 4 and x.shape[1] > 1:
            return x[:, 0:1, :, :]
        return x

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, ir, vis, out1, out2):
        """core/model_fusion_auto.py:240-260 -> the fused plane [B,1,H,W] in [0, 1], normalised over the batch."""
        if ops.want_param_grads(self):
            raise NotImplementedError(_NO_WGRAD_FN2 + _FREEZE)
        ir, vis = self._first_channel(ir), self._first_channel(vis)
        self._check(ir, vis, out1, out2)
        if torch.is_grad_enabled() and any(t.requires_grad for t in (ir, vis, out1, out2)):
            return _FN2Fn.apply(ir, vis, out1, out2, self, grad_anchor(ir.device))
        with torch.no_grad():
            return self._run(ir, vis, out1, out2, None)

    def _run(self, ir, vis, out1, out2, tape):
        maps, fused = ops.fn2_forward(ir, vis, out1, out2, self._pack())
        if tape is not None:
            tape.update(maps=maps, out=fused)     # every map, both gates' (a, z), f before the normalisation and (min, max)
        return fused

    def _reverse(self, d_fused, tape, want_guides=True):
        """d/d(fused) -> (d/d(ir), d/d(vis), d/d(out1), d/d(out2)); the last two None without want_guides."""
        return ops.fn2_backward(tape["maps"], d_fused, self._pack(), want_guides)

    @staticmethod
    def _map_list(maps):
        """The 20 taped maps in forward order as channel-last views: conv1's PReLU output (64); DRDB1's x_1 .. x_5 (32 each), relu(x6)
        (64) and output f1 (64); conv3(out1) (64); v1 (64); the same seven of DRDB2 (f2 last); conv4(out2) (64); v2 (64); f, conv2's PReLU
        output before the normalisation (1): 897 channels."""
        s1, s2 = maps["slab"]
        out = [s1[..., 0:64]]
        out += [s1[..., 64 + 32 * k:96 + 32 * k] for k in range(5)] + [maps["r6"][0], maps["f1"], maps["c3"], s2[..., 0:64]]
        out += [s2[..., 64 + 32 * k:96 + 32 * k] for k in range(5)] + [maps["r6"][1], maps["f2"], maps["c4"], maps["v2"]]
        return out + [maps["f"].permute(0, 2, 3, 1)]

    def _features(self, ir, vis, out1, out2):
        """(the taped maps (_map_list) as NCHW tensors, the two gates' attention [B,2,64]) -- for the tests."""
        ir, vis = self._first_channel(ir), self._first_channel(vis)
        self._check(ir, vis, out1, out2)
        tape = {}
        with torch.no_grad():
            self._run(ir, vis, out1, out2, tape)
        m = tape["maps"]
        return [x.permute(0, 3, 1, 2).contiguous() for x in self._map_list(m)], [m["g1"]["a"], m["g2"]["a"]]


class _FN2Fn(torch.autograd.Function):
    """Autograd node of Fusion_Network2: hand-written reverse pass, input gradients only."""

    @staticmethod
    def forward(ctx, ir, vis, out1, out2, module, anchor):
        tape = {}
        out = module._run(ir.detach(), vis.detach(), out1.detach(), out2.detach(), tape)
        ctx.tape, ctx.module = tape, module
        return out

    @staticmethod
    def backward(ctx, d_out):
        want = ctx.needs_input_grad[2] or ctx.needs_input_grad[3]
        d_ir, d_vis, d_1, d_2 = ctx.module._reverse(d_out.contiguous(), ctx.tape, want_guides=want)
        ctx.tape = None
        return d_ir, d_vis, d_1, d_2, None, None
