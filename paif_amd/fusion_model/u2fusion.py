"""U2Fusion baseline -- MI355X-native counterpart of the reference's fusion_model/U2Fusion.py: same constructor, forward signature,
module tree and state_dict keys (a checkpoint of the reference class loads with strict=True); forward and the reverse pass (input
gradients) launch the kernels of csrc/u2fusion.hip, one launch per layer, the eight wide convs and their transposes on the f32 matrix
instruction over one 264-channel NHWC slab.

It implements the protocol of the fusion network inside the composite models (forward_impl / backward_impl with a tape), so
`Network_MM_CompModel(U2Fusion(), ...)` runs through `attack_both` and the robustness harness like the searched network.

Built: fp32 planes of any size.  Not built (raises): parameter gradients (training the baseline); the reference's `features_grad` helper.
The maps stay fp32 under ops.set_storage("bf16" | "f16"), and the conv_precision / gemm_precision settings and ops.CONFIG["two_stream"]
do not apply: there is one arithmetic (exact fp32)."""
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache, grad_anchor

_NO_WGRAD = "U2Fusion: parameter gradients (training the baseline) are not built"


def _conv_block(cin, cout):
    """fusion_model/U2Fusion.py:78-90 with act_type='lrelu', norm_type=None: Sequential(Conv2d 3x3 pad 1, LeakyReLU(0.2))."""
    return nn.Sequential(nn.Conv2d(cin, cout, 3, stride=1, padding=1), nn.LeakyReLU(negative_slope=0.2, inplace=True))


class DenseLayer(nn.Module):
    """fusion_model/U2Fusion.py:91-99 -- a parameter container here: U2Fusion's kernels append the layer's map to the concat slab."""

    def __init__(self, num_channels, growth):
        super().__init__()
        self.conv = _conv_block(num_channels, growth)


class U2Fusion(nn.Module):
    """fusion_model/U2Fusion.py:102-125."""

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

    @staticmethod
    def _check_planes(x_over, x_under):
        for t in (x_over, x_under):
            if not t.is_cuda:
                raise RuntimeError("paif_amd ops need CUDA(HIP) tensors; got a %s tensor -- there is no CPU path" % t.device)
            if t.dtype != torch.float32:
                raise TypeError("U2Fusion: fp32 planes are expected, got %s" % t.dtype)
        if x_over.dim() != 4 or x_over.shape[1] != 1 or x_over.shape != x_under.shape:
            raise ValueError("U2Fusion: two [B,1,H,W] planes of one shape are expected, got %s and %s"
                             % (tuple(x_over.shape), tuple(x_under.shape)))

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, x_over, x_under):
        """fusion_model/U2Fusion.py:120-125 -> the fused plane [B,1,H,W] in tanh range."""
        if ops.want_param_grads(self):
            raise NotImplementedError(_NO_WGRAD + " -- freeze the parameters (requires_grad_(False)), or run under ops.no_param_grads() / "
                                      "torch.no_grad() for input gradients")
        self._check_planes(x_over, x_under)
        if torch.is_grad_enabled() and (x_over.requires_grad or x_under.requires_grad):
            return _U2FusionFn.apply(x_over, x_under, self, grad_anchor(x_over.device))
        with torch.no_grad():
            return self._run(x_over, x_under, None)

    def _run(self, x_over, x_under, tape):
        (cat, s1, s2, s3), fused = ops.u2fusion_forward(x_over, x_under, self._pack())
        if tape is not None:
            tape.update(cat=cat, s1=s1, s2=s2, s3=s3, out=fused)   # the nine maps and the fused plane: nothing is recomputed
        return fused

    def _features(self, x_over, x_under):
        """The nine LeakyReLU maps in layer order (conv_1, dense_layers.0..4: 44 channels each; sub.0..2: 128, 64, 32) as NCHW tensors
        -- for the tests."""
        self._check_planes(x_over, x_under)
        with torch.no_grad():
            (cat, s1, s2, s3), _ = ops.u2fusion_forward(x_over, x_under, self._pack())
        maps = [cat[..., 44 * k:44 * (k + 1)] for k in range(6)] + [s1, s2, s3]
        return [m.permute(0, 3, 1, 2).contiguous() for m in maps]

    # ---- the composite models' protocol (core/model_fusion_auto.py: _CompositeBase) -------------------------
    def forward_impl(self, ir, vis, inter=None, tape=None):
        """ir, vis: [B,>=1,H,W], channel 0 is used (x_over = infrared, x_under = visible Y) -> fused [B,1,H,W]; tape (dict): filled for
        backward_impl."""
        if inter is not None:
            raise NotImplementedError("U2Fusion: `inter` (the searched network's decomposition intermediates) does not apply")
        if tape is not None and ops.taping_wgrad():
            raise NotImplementedError(_NO_WGRAD)
        x_over, x_under = ir[:, 0:1, :, :], vis[:, 0:1, :, :]
        self._check_planes(x_over, x_under)
        return self._run(x_over, x_under, tape)

    def backward_impl(self, d_fused, tape, wgrad=False):
        """d/d(fused) [B,1,H,W] -> (d/d(x_over), d/d(x_under)) as [B,1,H,W] each."""
        if wgrad:
            raise NotImplementedError(_NO_WGRAD + " (wgrad=True)")
        return ops.u2fusion_backward(tape["cat"], tape["s1"], tape["s2"], tape["s3"], tape["out"], d_fused, self._pack())


class _U2FusionFn(torch.autograd.Function):
    """Autograd node of U2Fusion: hand-written reverse pass, input gradients only."""

    @staticmethod
    def forward(ctx, x_over, x_under, module, anchor):
        tape = {}
        out = module._run(x_over.detach(), x_under.detach(), tape)
        ctx.tape, ctx.module = tape, module
        return out

    @staticmethod
    def backward(ctx, d_out):
        d1, d2 = ctx.module.backward_impl(d_out.contiguous(), ctx.tape)
        ctx.tape = None
        return d1, d2, None, None
