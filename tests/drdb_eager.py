"""The hand-designed fusion network restated with torch's own convs on a module's parameters (any device, any dtype): the arithmetic of
DESIGN.md's DRDB section, written from it.  Used by tests/test_drdb_gpu.py and tools/drdb_time.py; `taps` collects the taped maps in
Fusion_Network._map_list order."""
import torch
import torch.nn.functional as F


def drdb(blk, x, taps=None):
    """x [B,64,H,W] -> x + relu(conv(cat(x, x_1 .. x_5))), x_k = relu(Dcov_k(cat(x, x_1 .. x_{k-1}))) at dilation 2, zero pad 2."""
    cat = x
    for k in range(1, 6):
        c = getattr(blk, "Dcov%d" % k)
        xk = F.relu(F.conv2d(cat, c.weight, c.bias, padding=2, dilation=2))
        if taps is not None:
            taps.append(xk)
        cat = torch.cat((cat, xk), 1)
    r = F.relu(F.conv2d(cat, blk.conv.weight, blk.conv.bias))
    out = x + r
    if taps is not None:
        taps += [r, out]
    return out


def pre_clamp(net, ir, vis, taps=None):
    """-> f [B,1,H,W]: conv21's PReLU output, before the clamp."""
    a = net.relu.weight

    def prelu(v):
        return torch.where(v > 0, v, a * v)

    x = prelu(F.conv2d(torch.cat((ir[:, 0:1], vis[:, 0:1]), 1), net.conv1.weight, net.conv1.bias, padding=1))
    if taps is not None:
        taps.append(x)
    x = drdb(net.DRDB2, drdb(net.DRDB1, x, taps), taps)
    c2 = prelu(F.conv2d(x, net.conv2.weight, net.conv2.bias, padding=1))
    f = prelu(F.conv2d(c2, net.conv21.weight, net.conv21.bias, padding=1))
    if taps is not None:
        taps += [c2, f]
    return f


def normalise(f):
    """clamp to [0, 1], then (c - min c) / (max c - min c) over the whole batch."""
    c = torch.where(f > 1, torch.ones_like(f), f)
    c = torch.where(c < 0, torch.zeros_like(c), c)
    return (c - c.min()) / (c.max() - c.min())


def fusion_network(net, ir, vis):
    return normalise(pre_clamp(net, ir, vis))
