"""ReCoNet baseline -- MI355X-native counterpart of the reference's fusion_model/Reconet.py: same constructor, forward signature and
state_dict keys (a checkpoint of the reference class loads with strict=True); forward and the reverse pass (input gradients) launch the
kernels of csrc/reconet.hip, one launch per recurrence, the 3*dim-channel map never in memory.

The composite protocol and what is not built: fusion_model/_native.py; `forward_impl` takes `init_f` as well.

Built: depth >= 1, dim 16 / 32 / 64, BatchNorm in eval mode (folded into the packed weights), fp32 planes of any size.  Not built either:
train-mode BatchNorm.  The planes stay fp32 under ops.set_storage("bf16" | "f16") because they have one channel: there is no traffic to
save."""
import torch
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache
from ._native import NativeFusion

DIMS = (16, 32, 64)


class ConvGroup(nn.Module):
    """fusion_model/Reconet.py:10-23: (Conv2d, BatchNorm2d | Identity, GELU) -- a parameter container here."""

    def __init__(self, conv, use_bn):
        super().__init__()
        dim = conv.out_channels
        self.group = nn.Sequential(conv, nn.BatchNorm2d(dim) if use_bn else nn.Identity(), nn.GELU())

    def forward(self, x):
        raise NotImplementedError("ConvGroup holds parameters only: the arithmetic runs inside ReCoNet's fused kernels")


class DGroup(nn.Module):
    """fusion_model/Reconet.py:25-52: three dilated in_c -> dim convs, concat, 3*dim -> out_c conv, tanh -- a parameter container here."""

    def __init__(self, in_c, out_c, dim, k_size, use_bn):
        super().__init__()
        self.conv_d = nn.ModuleList([
            ConvGroup(nn.Conv2d(in_c, dim, kernel_size=k_size, padding='same', dilation=(i + 1)), use_bn=use_bn) for i in range(3)])
        self.conv_s = nn.Sequential(nn.Conv2d(3 * dim, out_c, kernel_size=3, padding='same'), nn.Tanh())

    def forward(self, x):
        raise NotImplementedError("DGroup holds parameters only: the arithmetic runs inside ReCoNet's fused kernels")


class ReCoNet(NativeFusion):
    """fusion_model/Reconet.py:55-105."""
    NAME = "ReCoNet"

    def __init__(self, depth: int, dim: int, use_bn: bool):
        super().__init__()
        if int(depth) < 1:
            raise ValueError("ReCoNet: depth must be >= 1, got %r" % (depth,))
        if dim not in DIMS:
            raise NotImplementedError("ReCoNet: dim=%r is not built -- the fused kernels exist for dim in %s (the published network "
                                      "uses 64); there is no eager fallback" % (dim, list(DIMS)))
        self.depth = int(depth)
        self.dim = int(dim)
        self.use_bn = bool(use_bn)
        self.att_a_conv = nn.Conv2d(2, 1, kernel_size=3, padding='same', bias=False)
        self.att_b_conv = nn.Conv2d(2, 1, kernel_size=3, padding='same', bias=False)
        self.decoder = DGroup(in_c=3, out_c=1, dim=dim, k_size=3, use_bn=use_bn)
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _pack(self):
        if self.use_bn and self.training:
            raise NotImplementedError("ReCoNet: train-mode BatchNorm (batch statistics) is not built -- call .eval(); the running "
                                      "statistics are folded into the packed conv weights")
        groups, params = [], [self.att_a_conv.weight, self.att_b_conv.weight, self.decoder.conv_s[0].weight, self.decoder.conv_s[0].bias]
        for cg in self.decoder.conv_d:
            conv, bn = cg.group[0], cg.group[1]
            params += [conv.weight, conv.bias]
            if self.use_bn:
                params += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
                groups.append((conv.weight, conv.bias, (bn.weight, bn.bias, bn.running_mean, bn.running_var, float(bn.eps))))
            else:
                groups.append((conv.weight, conv.bias, None))
        cs = self.decoder.conv_s[0]
        return self._packs.get("reconet", params, lambda: ops.reconet_pack(self.att_a_conv.weight, self.att_b_conv.weight, groups,
                                                                           cs.weight, cs.bias, self.dim))

    @classmethod
    def _no_wgrad_true(cls):
        return "ReCoNet: parameter gradients (wgrad=True, training the baseline) are not built"

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, i_1, i_2, init_f: str = 'max', show_detail: bool = False):
        """fusion_model/Reconet.py:67-80: -> the last i_f, or (list of depth+1 i_f, list of att_a, list of att_b) under show_detail."""
        if not show_detail:
            return self._gate(i_1, i_2, init_f)
        if self._wants_node(i_1, i_2):
            raise NotImplementedError("ReCoNet: show_detail returns the intermediate planes without an autograd node -- call it "
                                      "under torch.no_grad()")
        with torch.no_grad():
            tape = {}
            self._run(i_1, i_2, init_f, tape)
            return tape["i_f"], tape["att_a"], tape["att_b"]

    def _run(self, i_1, i_2, init_f, tape):
        pack = self._pack()
        use_max = init_f == 'max'
        f = ops.reconet_init(i_1, i_2, use_max)
        if tape is None:
            for _ in range(self.depth):
                f = ops.reconet_step(i_1, i_2, f, pack, self.dim)
            return f
        fs, aa, ab = [f], [], []
        for _ in range(self.depth):
            f, a, b = ops.reconet_step(i_1, i_2, f, pack, self.dim, want_att=True)
            fs.append(f), aa.append(a), ab.append(b)
        tape.update(i_1=i_1, i_2=i_2, i_f=fs, att_a=aa, att_b=ab, use_max=use_max)
        return f

    # ---- the composite models' protocol (core/model_fusion_auto.py: _CompositeBase) -------------------------
    def forward_impl(self, ir, vis, inter=None, tape=None, init_f='max'):
        """ir, vis: [B,>=1,H,W], channel 0 is used (i_1 = infrared, i_2 = visible Y) -> fused [B,1,H,W]; tape (dict): filled for
        backward_impl (the depth+1 i_f planes and the attention maps: 3*depth+1 planes, nothing wide)."""
        i_1, i_2 = self._impl_planes(ir, vis, inter, tape)
        return self._run(i_1, i_2, init_f, tape)

    def _reverse(self, d_fused, tape):
        """d/d(fused) [B,1,H,W] -> (d/d(i_1), d/d(i_2)) as [B,1,H,W] each.  Ties: see csrc/reconet.hip (the channel max of the attention
        input routes a tie to the image plane, the initialisation's elementwise max splits it)."""
        pack = self._pack()
        i_1, i_2, fs = tape["i_1"], tape["i_2"], tape["i_f"]
        d_f = d_fused.contiguous()
        d_i1, d_i2 = torch.empty_like(fs[0]), torch.empty_like(fs[0])
        ws = torch.empty((2,) + tuple(fs[0].shape), device=d_f.device, dtype=torch.float32)
        for k in range(self.depth - 1, -1, -1):
            d_f = ops.reconet_step_bwd(i_1, i_2, fs[k], tape["att_a"][k], tape["att_b"][k], fs[k + 1], d_f, pack, self.dim, d_i1, d_i2, ws,
                                       accumulate=k != self.depth - 1)
        ops.reconet_init_bwd_(d_i1, d_i2, i_1, i_2, tape["use_max"], d_f)
        return d_i1, d_i2
