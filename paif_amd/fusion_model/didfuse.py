"""DIDFuse baseline -- MI355X-native counterpart of the reference's fusion_model/AUIF.py (class DID, the DIDFuse auto-encoder): same
constructors, forward signature, module tree and state_dict keys (83 entries: 11 convs, 11 BatchNorms, 6 PReLU slopes; a checkpoint of the
reference class loads with strict=True); forward and the reverse pass (input gradients) launch the kernels of csrc/didfuse.hip, ten and
nine launches, the 64- and 128-channel convs and their transposes on the f32 matrix instruction over NHWC slabs (csrc/conv_slab.h).

BatchNorm is the EVAL-MODE one (running statistics), folded into the weight pack on the device; every reference flow calls model.eval().
A forward in .train() mode raises: batch-statistics BatchNorm is not built, and running statistics are never used silently in its place.
The running statistics and the PReLU slopes are part of the pack's key: an in-place change of any of them rebuilds the pack.  The six
slopes are read to the host when the pack is built (never inside a hipGraph capture) and must be >= 0: the reverse pass reads the PReLU
branch off the taped output.

The composite calls forward(ir[:, 0:1], Y[:, 0:1]): the infrared plane enters x_over / AE_Encoder1, Y enters x_under / AE_Encoder2.

The composite protocol, what is not built and the settings that do not apply: fusion_model/_native.py.  Built: fp32 planes with
H, W >= 2 (reflection padding).  Not built either: .train() mode."""
import torch.nn as nn

from .. import ops
from ..operations_m import _PackCache
from ._native import NativeFusion

_NO_TRAIN = ("DIDFuse: training-mode BatchNorm (batch statistics) is not built -- call .eval(), as every reference flow does; the running "
             "statistics are not used in its place")

channel = 64


# ---- the reference's member classes, as parameter containers: DID's kernels do the arithmetic --------------------------------------
class Cov1(nn.Module):
    """fusion_model/AUIF.py:7-18."""

    def __init__(self):
        super().__init__()
        self.cov1 = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(1, channel, 3, padding=0), nn.BatchNorm2d(channel), nn.PReLU())


class Cov2(nn.Module):
    """fusion_model/AUIF.py:21-31."""

    def __init__(self):
        super().__init__()
        self.cov2 = nn.Sequential(nn.Conv2d(channel, channel, 3, padding=1), nn.BatchNorm2d(channel), nn.PReLU())


class Cov3(nn.Module):
    """fusion_model/AUIF.py:34-45."""

    def __init__(self):
        super().__init__()
        self.cov3 = nn.Sequential(nn.Conv2d(channel, channel, 3, padding=1), nn.BatchNorm2d(channel), nn.Tanh())


class Cov4(nn.Module):
    """fusion_model/AUIF.py:48-59."""

    def __init__(self):
        super().__init__()
        self.cov4 = nn.Sequential(nn.Conv2d(channel, channel, 3, padding=1), nn.BatchNorm2d(channel), nn.Tanh())


class Cov5(nn.Module):
    """fusion_model/AUIF.py:62-72."""

    def __init__(self):
        super().__init__()
        self.cov5 = nn.Sequential(nn.Conv2d(channel * 2, channel, 3, padding=1), nn.BatchNorm2d(channel), nn.PReLU())


class Cov6(nn.Module):
    """fusion_model/AUIF.py:75-85."""

    def __init__(self):
        super().__init__()
        self.cov6 = nn.Sequential(nn.Conv2d(channel * 2, channel, 3, padding=1), nn.BatchNorm2d(channel), nn.PReLU())


class Cov7(nn.Module):
    """fusion_model/AUIF.py:88-99."""

    def __init__(self):
        super().__init__()
        self.cov7 = nn.Sequential(nn.ReflectionPad2d(1), nn.Conv2d(channel * 2, 1, 3, padding=0), nn.BatchNorm2d(1), nn.Sigmoid())


class AE_Encoder(nn.Module):
    """fusion_model/AUIF.py:102-115."""

    def __init__(self):
        super().__init__()
        self.cov1 = Cov1()
        self.cov2 = Cov2()
        self.cov3 = Cov3()
        self.cov4 = Cov4()


class AE_Decoder(nn.Module):
    """fusion_model/AUIF.py:118-129."""

    def __init__(self):
        super().__init__()
        self.cov5 = Cov5()
        self.cov6 = Cov6()
        self.cov7 = Cov7()


class DID(NativeFusion):
    """fusion_model/AUIF.py:131-150."""
    NAME = "DIDFuse"

    def __init__(self):
        super().__init__()
        self.num_channels = 2
        self.num_features = 44
        self.growth = 44
        self.AE_Encoder1 = AE_Encoder()
        self.AE_Encoder2 = AE_Encoder()
        self.AE_Decoder1 = AE_Decoder()
        self._packs = _PackCache()

    # ---- packed weights ---------------------------------------------------------------------------------------------------
    def _blocks(self):
        """The eleven nn.Sequential in paif_amd.synthetic.DIDFUSE_CONVS order."""
        out = []
        for e in (self.AE_Encoder1, self.AE_Encoder2):
            out += [e.cov1.cov1, e.cov2.cov2, e.cov3.cov3, e.cov4.cov4]
        d = self.AE_Decoder1
        return out + [d.cov5.cov5, d.cov6.cov6, d.cov7.cov7]

    @staticmethod
    def _conv_bn(seq):
        mods = list(seq)
        conv = next(m for m in mods if isinstance(m, nn.Conv2d))
        bn = next(m for m in mods if isinstance(m, nn.BatchNorm2d))
        return conv, bn

    def _pack(self):
        convs, slopes = [], []
        for seq in self._blocks():
            conv, bn = self._conv_bn(seq)
            convs.append((conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps))
            slopes += [m.weight for m in seq if isinstance(m, nn.PReLU)]
        # the key: every tensor the pack is computed from -- the BatchNorm buffers and the PReLU slopes included
        params = [t for c in convs for t in c[:6]] + slopes
        eps = tuple(float(c[6]) for c in convs)     # a Python float on the module, folded into the pack: a changed eps starts a new cache
        if self.__dict__.setdefault("_pack_eps", eps) != eps:
            self._packs, self._pack_eps = _PackCache(), eps
        return self._packs.get("didfuse", params, lambda: ops.didfuse_pack(convs, slopes))

    @classmethod
    def _check_planes(cls, x_over, x_under):
        super()._check_planes(x_over, x_under)
        if x_over.shape[2] < 2 or x_over.shape[3] < 2:
            raise ValueError("DIDFuse: reflection padding by 1 needs H, W >= 2 (as torch's ReflectionPad2d), got [B,1,H,W] = %s"
                             % (tuple(x_over.shape),))

    def _check_mode(self):
        if self.training:
            raise NotImplementedError(_NO_TRAIN)

    # ---- the reference's interface --------------------------------------------------------------------------------------
    def forward(self, x_over, x_under):
        """fusion_model/AUIF.py:141-150 -> the fused plane [B,1,H,W] in (0, 1)."""
        return self._gate(x_over, x_under)

    def _run(self, x_over, x_under, tape):
        maps, fused = ops.didfuse_forward(x_over, x_under, self._pack())
        if tape is not None:
            tape.update(maps=maps, out=fused)   # every map and the fused plane: nothing is recomputed
        return fused

    @staticmethod
    def _map_list(maps):
        """The 14 taped maps in forward order as NHWC views: per stream (x_over, x_under) f1, f2, fB, fD (64 each); the means F_1, F_2,
        F_b, F_d (64 each); Out1, Out2 (64 each): 896 channels."""
        out = []
        for s in range(2):
            out += [maps["enc"][s][..., 64 * k:64 * (k + 1)] for k in range(4)]
        out += [maps["d2"][..., 64:128], maps["d1"][..., 64:128], maps["bd"][..., 0:64], maps["bd"][..., 64:128]]
        return out + [maps["d1"][..., 0:64], maps["d2"][..., 0:64]]

    def _reverse(self, d_fused, tape):
        """d/d(fused) -> (d/d(x_over), d/d(x_under)): inside the composite, (d/d(ir), d/d(Y))."""
        return ops.didfuse_backward(tape["maps"], tape["out"], d_fused, self._pack())
