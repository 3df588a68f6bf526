"""SDNet baseline -- MI355X-native counterpart of the reference's fusion_model/SDNet.py: same constructor, forward signature and
state_dict keys (a checkpoint of the reference class loads with strict=True); forward and the reverse pass (input gradients) launch the
kernels of csrc/sdnet.hip, one launch per layer, both encoders in every launch, the dense convs on the f32 matrix instruction.

It implements the protocol of the fusion network inside the composite models (forward_impl / backward_impl with a tape), so
`Network_MM_CompModel(SDNet(), ...)` runs through `attack_both` and the robustness harness like the searched network.

Built: fp32 planes of any size.  Not built (raises): parameter gradients (training the baseline).  The reference's `decom` and
`conv51` .. `conv72` are parameter containers: its forward never touches them.  The maps stay fp32 under ops.set_storage("bf16" | "f16"),
and the conv_precision / gemm_precision settings and ops.CONFIG["two_stream"] do not apply: there is one arithmetic (exact fp32)."""
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache, grad_anchor

# (attribute, layer of ops.sdnet_pack, encoder) of the nine convs the forward uses
_USED = (("conv11", 0, 0), ("conv12", 0, 1), ("conv21", 1, 0), ("conv22", 1, 1), ("conv31", 2, 0), ("conv32", 2, 1),
         ("conv41", 3, 0), ("conv42", 3, 1), ("fuse", 4, 0))
_NO_WGRAD = "SDNet: parameter gradients (training the baseline) are not built"


class SDNet(nn.Module):
    """fusion_model/SDNet.py:6-47."""

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

    @staticmethod
    def _check_planes(x1, x2):
        for t in (x1, x2):
            if not t.is_cuda:
                raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor -- there is no CPU path" % t.device)
            if t.dtype != torch.float32:
                raise TypeError("SDNet: fp32 planes are expected, got %s" % t.dtype)
        if x1.dim() != 4 or x1.shape[1] != 1 or x1.shape != x2.shape:
            raise ValueError("SDNet: two [B,1,H,W] planes of one shape are expected, got %s and %s" % (tuple(x1.shape), tuple(x2.shape)))

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, x1, x2):
        """fusion_model/SDNet.py:33-47 -> the fused plane [B,1,H,W] in tanh range."""
        if ops.want_param_grads(self):
            raise NotImplementedError(_NO_WGRAD + " -- freeze the parameters (requires_grad_(False)), or run under ops.no_param_grads() / "
                                      "torch.no_grad() for input gradients")
        self._check_planes(x1, x2)
        if torch.is_grad_enabled() and (x1.requires_grad or x2.requires_grad):
            return _SDNetFn.apply(x1, x2, self, grad_anchor(x1.device))
        with torch.no_grad():
            return self._run(x1, x2, None)

    def _run(self, x1, x2, tape):
        feat, out = ops.sdnet_forward(x1, x2, self._pack())
        if tape is not None:
            tape.update(feat=feat, out=out)   # the eight maps and the fused plane: nothing is recomputed
        return out

    def _features(self, x1, x2):
        """The eight LeakyReLU maps x11 .. x14, x21 .. x24 (SDNet.py:34-42) as NCHW tensors -- for the tests."""
        self._check_planes(x1, x2)
        with torch.no_grad():
            feat, _ = ops.sdnet_forward(x1, x2, self._pack())
        return [feat[e, l].permute(0, 3, 1, 2).contiguous() for e in range(2) for l in range(4)]

    # ---- the composite models' protocol (core/model_fusion_auto.py: _CompositeBase) -------------------------
    def forward_impl(self, ir, vis, inter=None, tape=None):
        """ir, vis: [B,>=1,H,W], channel 0 is used (x1 = infrared, x2 = visible Y) -> fused [B,1,H,W]; tape (dict): filled for
        backward_impl."""
        if inter is not None:
            raise NotImplementedError("SDNet: `inter` (the searched network's decomposition intermediates) does not apply")
        if tape is not None and ops.taping_wgrad():
            raise NotImplementedError(_NO_WGRAD)
        x1, x2 = ir[:, 0:1, :, :], vis[:, 0:1, :, :]
        self._check_planes(x1, x2)
        return self._run(x1, x2, tape)

    def backward_impl(self, d_fused, tape, wgrad=False):
        """d/d(fused) [B,1,H,W] -> (d/d(x1), d/d(x2)) as [B,1,H,W] each."""
        if wgrad:
            raise NotImplementedError(_NO_WGRAD + " (wgrad=True)")
        return ops.sdnet_backward(tape["feat"], tape["out"], d_fused, self._pack())


class _SDNetFn(torch.autograd.Function):
    """Autograd node of SDNet: hand-written reverse pass, input gradients only."""

    @staticmethod
    def forward(ctx, x1, x2, module, anchor):
        tape = {}
        out = module._run(x1.detach(), x2.detach(), tape)
        ctx.tape, ctx.module = tape, module
        return out

    @staticmethod
    def backward(ctx, d_out):
        d1, d2 = ctx.module.backward_impl(d_out.contiguous(), ctx.tape)
        ctx.tape = None
        return d1, d2, None, None
