"""TEST INFRASTRUCTURE: the Sobel fusion criteria restated from torch.nn.functional calls, in any float dtype and on any device.

The GPU tests compare the HIP criteria (paif_amd/core/loss.py) with the recorded float64 results of tests/golden/gl_fusion_losses*.npz;
this restatement produces the same quantities for inputs no fixture holds (the non-dyadic run, the timing tool's eager column) and is
itself pinned to the fixtures by tests/test_fusion_losses_cpu.py.  Every function takes the planes as the criteria do: channel 0 of
`ir`, `vis` (YCrCb) and `mask` is read, `gen` is [B,1,H,W]."""
import torch
import torch.nn.functional as F

GX = [[-1.0, 0.0, 1.0], [-2.0, 0.0, 2.0], [-1.0, 0.0, 1.0]]
GY = [[1.0, 2.0, 1.0], [0.0, 0.0, 0.0], [-1.0, -2.0, -1.0]]


def sobel(x):
    """|Gx * x| + |Gy * x|: two 3x3 cross-correlations with zero padding 1 on a [B,1,H,W] map."""
    wx = torch.tensor(GX, dtype=x.dtype, device=x.device).view(1, 1, 3, 3)
    wy = torch.tensor(GY, dtype=x.dtype, device=x.device).view(1, 1, 3, 3)
    return F.conv2d(x, wx, padding=1).abs() + F.conv2d(x, wy, padding=1).abs()


def _c0(t):
    return t[:, :1, :, :]


def fusionloss(ir, vis, gen):
    y, ir = _c0(vis), _c0(ir)
    return F.l1_loss(torch.max(y, ir), gen) + 8 * F.l1_loss(torch.max(sobel(y), sobel(ir)), sobel(gen))


def fusionloss2(ir, vis, gen, mask):
    return F.l1_loss(_c0(mask), gen)


def fusionloss3(ir, vis, gen, mask):
    return F.l1_loss(_c0(mask), gen) + F.l1_loss(sobel(_c0(mask)), sobel(gen))


def fusionloss4(ir, vis, gen, mask):
    syn = (_c0(vis) + _c0(ir)) / 2
    return F.l1_loss(syn, gen) + 4 * F.l1_loss(sobel(syn), sobel(gen))


def fusionloss6(ir, vis, gen, mask):
    y, ir = _c0(vis), _c0(ir)
    return (F.l1_loss(_c0(mask), gen) * 0.5 + F.l1_loss(y + ir, gen) * 0.5
            + 6 * F.l1_loss(torch.max(sobel(y), sobel(ir)), sobel(gen)))


def fusionloss_add(ir, vis, gen):
    y, ir = _c0(vis), _c0(ir)
    return F.l1_loss(y * 0.4 + ir * 0.6, gen) * 1.5 + 5 * F.l1_loss(torch.max(sobel(y), sobel(ir)), sobel(gen))


def total_fusion_loss3(ir, vis, mask, gen):
    return fusionloss(ir, vis, gen) * 3


def _ssim(x, y):
    """Mean SSIM with the 11x11 Gaussian window (sigma 1.5), zero padding 5, one channel."""
    import math
    g = torch.tensor([math.exp(-(i - 5) ** 2 / (2 * 1.5 ** 2)) for i in range(11)], dtype=torch.float32)
    g = g / g.sum()                      # the window is built and normalised in float32 whatever the images' dtype is
    w = (g[:, None] * g[None, :]).view(1, 1, 11, 11).to(device=x.device, dtype=x.dtype)
    mu1, mu2 = F.conv2d(x, w, padding=5), F.conv2d(y, w, padding=5)
    s1 = F.conv2d(x * x, w, padding=5) - mu1 * mu1
    s2 = F.conv2d(y * y, w, padding=5) - mu2 * mu2
    s12 = F.conv2d(x * y, w, padding=5) - mu1 * mu2
    c1, c2 = 0.01 ** 2, 0.03 ** 2
    return (((2 * mu1 * mu2 + c1) * (2 * s12 + c2)) / ((mu1 * mu1 + mu2 * mu2 + c1) * (s1 + s2 + c2))).mean()


def fusionloss_grad3(ir, vis, gen, mask):
    m = _c0(mask)
    return F.mse_loss(m, gen) + 1.1 * (1 - _ssim(gen, m))


# name -> (restatement, argument order, intensity weights w_i, gradient weights v_j); the weights enter the tests' error bounds
CRITERIA = {
    "Fusionloss": (fusionloss, ("ir", "vis", "gen"), (1.0,), (8.0,)),
    "Fusionloss2": (fusionloss2, ("ir", "vis", "gen", "mask"), (1.0,), ()),
    "Fusionloss3": (fusionloss3, ("ir", "vis", "gen", "mask"), (1.0,), (1.0,)),
    "Fusionloss4": (fusionloss4, ("ir", "vis", "gen", "mask"), (1.0,), (4.0,)),
    "Fusionloss6": (fusionloss6, ("ir", "vis", "gen", "mask"), (0.5, 0.5), (6.0,)),
    "Fusionloss_add": (fusionloss_add, ("ir", "vis", "gen"), (1.5,), (5.0,)),
    "Fusionloss_grad3": (fusionloss_grad3, ("ir", "vis", "gen", "mask"), None, None),
    "Total_fusion_loss3": (total_fusion_loss3, ("ir", "vis", "mask", "gen"), (3.0,), (24.0,)),
}


def value_bound(name):
    """|value - float64 value| <= 2^-20 * (sum_i w_i * 2 + 8 * sum_j v_j): planes in [0, 2], S <= 8, 16 ulp per pixel term."""
    _, _, w, v = CRITERIA[name]
    return 2.0 ** -20 * (2 * sum(w) + 8 * sum(v))


def grad_bound(name, n):
    """elementwise |d gen - float64 d gen| <= 2^-20 * (sum_i w_i + 8 * sum_j v_j) / N."""
    _, _, w, v = CRITERIA[name]
    return 2.0 ** -20 * (sum(w) + 8 * sum(v)) / n


def call(name, planes, dtype=None, device=None, grad=False):
    """planes: dict ir / vis / gen / mask of tensors or arrays -> value (and d value / d gen when `grad`)."""
    fn, order = CRITERIA[name][:2]
    t = {k: torch.as_tensor(v).to(device=device, dtype=dtype) for k, v in planes.items()}
    if grad:
        t["gen"] = t["gen"].clone().requires_grad_(True)
    val = fn(*[t[k] for k in order])
    if not grad:
        return val
    val.backward()
    return val.detach(), t["gen"].grad
