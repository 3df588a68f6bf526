"""SKFF and Fusion_Network2 restated with torch's own ops on a module's parameters (any device; `dtype` converts parameters and inputs):
the arithmetic of DESIGN.md's SKFF section, written from it.  Used by tests/test_skff_gpu.py and tools/skff_time.py; `taps` collects the
taped maps in Fusion_Network2._map_list order, `gates` the attention [B,n,64] of each gate."""
import torch
import torch.nn.functional as F

from tests.drdb_eager import drdb


def _p(t, dtype):
    return t if dtype is None else t.to(dtype)


def skff(mod, xs, dtype=None, gates=None):
    """xs: n maps [B,64,H,W] -> V = sum_h a_h X_h, a = softmax over h of fcs.h(PReLU(conv_du.0(mean over pixels of sum_h X_h)))."""
    xs = [_p(x, dtype) for x in xs]
    du, act = mod.conv_du[0], mod.conv_du[1]
    s = sum(xs).mean(dim=(2, 3))                                                         # [B,64]
    z = F.linear(s, _p(du.weight, dtype).flatten(1), None if du.bias is None else _p(du.bias, dtype))
    zz = torch.where(z > 0, z, _p(act.weight, dtype) * z)
    a = torch.stack([F.linear(zz, _p(fc.weight, dtype).flatten(1), None if fc.bias is None else _p(fc.bias, dtype)) for fc in mod.fcs], 1)
    a = torch.softmax(a, dim=1)                                                          # [B,n,64]
    if gates is not None:
        gates.append(a)
    return sum(a[:, h, :, None, None] * x for h, x in enumerate(xs))


def pre_norm(net, ir, vis, out1, out2, dtype=None, taps=None, gates=None):
    """-> f [B,1,H,W]: conv2's PReLU output, before the normalisation."""
    a = _p(net.relu.weight, dtype)

    def prelu(v):
        return torch.where(v > 0, v, a * v)

    def conv(c, x, pad=0):
        return F.conv2d(x, _p(c.weight, dtype), _p(c.bias, dtype), padding=pad)

    class _Blk:   # a DRDB's convs in `dtype`, for tests.drdb_eager.drdb
        def __init__(self, blk):
            for name in ("Dcov1", "Dcov2", "Dcov3", "Dcov4", "Dcov5", "conv"):
                c = getattr(blk, name)
                setattr(self, name, type("C", (), dict(weight=_p(c.weight, dtype), bias=_p(c.bias, dtype))))

    ir, vis, out1, out2 = (_p(t, dtype) for t in (ir, vis, out1, out2))
    x = prelu(conv(net.conv1, torch.cat((ir[:, 0:1], vis[:, 0:1]), 1), 1))
    t = None if taps is None else []
    if t is not None:
        t.append(x)
    f1 = drdb(_Blk(net.DRDB1), x, t)
    c3 = conv(net.conv3, out1)
    v1 = skff(net.skff, [f1, c3], dtype, gates)
    if t is not None:
        t += [c3, v1]
    f2 = drdb(_Blk(net.DRDB2), v1, t)
    c4 = conv(net.conv4, out2)
    v2 = skff(net.skff2, [f2, c4], dtype, gates)
    f = prelu(conv(net.conv2, v2, 1))
    if t is not None:
        taps += t + [c4, v2, f]
    return f


def normalise(f):
    """(f - min f) / (max f - min f) over the whole batch, no clamp."""
    return (f - f.min()) / (f.max() - f.min())


def fusion_network2(net, ir, vis, out1, out2, dtype=None):
    return normalise(pre_norm(net, ir, vis, out1, out2, dtype))
