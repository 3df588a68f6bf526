"""TEST INFRASTRUCTURE -- fixtures of the Sobel fusion criteria and of Sobelxy.  Build container only (CPU):

    python tools/make_golden_fusion_losses.py <reference tree>

Imports the reference's own classes (core/loss.py) through the shims of oracle/ref_import.py and stores one file per case under
tests/golden/, gl_fusion_losses_<B>x1x<H>x<W>.npz:

ir [B,3,H,W], vis [B,3,H,W] (the YCrCb tensor: channel 0 = Y), mask [B,1,H,W], gen [B,1,H,W], cot [B,1,H,W]      float32 inputs
<Class>/value32, <Class>/value64          the criterion in float32 and float64
<Class>/dgen32, <Class>/dgen64            d value / d gen from float32 and float64 autograd
<Class>/floor                             (|value32 - value64|, max|dgen32 - dgen64|): the reference's own float32 floor
Sobelxy/out32, out64, dx32, dx64          S(gen) and its input gradient for the cotangent `cot`

INPUTS.  Every plane is an integer multiple of 1/256 in [0, 1] (the cotangent: of 1/128 in [-1, 1]) from the counter hash of
paif_amd/synthetic.py, so every Sobel sum, max, difference and comparison is exact in float32 in any summation order.  Ties and flat
zones are deliberate: the left half of `gen` (the upper half of a single column) equals the mask, the lower right quadrant of `gen` is
the constant 1/2, and in the last image the upper right quadrant equals max(Y, ir).  No tie stands against 0.4 Y + 0.6 ir, which is not
exact: a pixel of `gen` within 1e-3 of it (Y = ir = gen, by chance or by the ties above) is moved by 1/256.

Only data is stored.  For float64 the two Sobel weight tensors of each reference module are re-wrapped in float64."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import ref_import  # noqa: E402
from paif_amd import synthetic as S  # noqa: E402
from tests import fusion_loss_eager as E  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
TILE = (32, 64)    # the kernels' tile (csrc/sobel_loss.hip): the last case is one pixel more in both dimensions
CASES = ((1, 1, 1), (1, 1, 7), (1, 7, 1), (1, 3, 5), (2, 19, 29), (2, TILE[0] + 1, TILE[1] + 1))


def tag(B, H, W):
    return "%dx1x%dx%d" % (B, H, W)


def dyadic(seed, shape):
    n = int(np.prod(shape))
    return (np.minimum(np.floor(S.hash_uniform(seed, n) * 257.0), 256.0) / 256.0).astype(np.float32).reshape(shape)


def make_inputs(B, H, W):
    seed = 7000 + 131 * H + W
    ir, vis = dyadic(seed, (B, 3, H, W)), dyadic(seed + 1, (B, 3, H, W))
    mask, gen = dyadic(seed + 2, (B, 1, H, W)), dyadic(seed + 3, (B, 1, H, W))
    cot = (dyadic(seed + 4, (B, 1, H, W)) * 2.0 - 1.0).astype(np.float32)
    if W > 1:
        gen[:, :, :, :W // 2] = mask[:, :, :, :W // 2]
    else:
        gen[:, :, :H // 2] = mask[:, :, :H // 2]
    if H > 1 and W > 1:
        gen[-1, 0, :H // 2, W // 2:] = np.maximum(vis[-1, 0], ir[-1, 0])[:H // 2, W // 2:]
        gen[:, :, H // 2:, W // 2:] = 0.5
    # 0.4 Y + 0.6 ir is not exact: where it meets `gen` (Y = ir = gen by chance or by the ties above) float32 and float64 disagree on
    # the sign of the difference, so such a pixel of `gen` moves by 1/256
    near = np.abs(0.4 * vis[:, :1].astype(np.float64) + 0.6 * ir[:, :1].astype(np.float64) - gen) < 1e-3
    gen[near] = np.where(gen[near] < 1.0, gen[near] + 1.0 / 256.0, gen[near] - 1.0 / 256.0).astype(np.float32)
    assert np.abs(0.4 * vis[:, :1].astype(np.float64) + 0.6 * ir[:, :1].astype(np.float64) - gen).min() > 1e-3
    return dict(ir=ir, vis=vis, mask=mask, gen=gen, cot=cot)


def retype(module, dtype):
    """The reference builds its Sobel weights as float32 tensors: re-wrap them in the dtype of the run."""
    for m in module.modules():
        if type(m).__name__ == "Sobelxy":
            m.weightx = torch.nn.Parameter(m.weightx.data.to(dtype), requires_grad=False)
            m.weighty = torch.nn.Parameter(m.weighty.data.to(dtype), requires_grad=False)
    return module


def run(cls, order, planes, dtype):
    t = {k: torch.from_numpy(v).to(dtype) for k, v in planes.items()}
    t["gen"].requires_grad_(True)
    with ref_import.quiet():
        crit = retype(cls(), dtype)
    val = crit(*[t[k] for k in order])
    assert val.dtype == dtype, (cls.__name__, val.dtype)
    val.backward()
    return val.detach().numpy(), t["gen"].grad.numpy()


def main():
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "core")):
        sys.exit(__doc__)
    ref_import.REF_ROOT = os.path.abspath(sys.argv[1])
    L = ref_import.load()["loss"]
    for B, H, W in CASES:
        planes = make_inputs(B, H, W)
        out = dict(planes)
        for name, (_, order, _, _) in E.CRITERIA.items():
            v32, g32 = run(getattr(L, name), order, planes, torch.float32)
            v64, g64 = run(getattr(L, name), order, planes, torch.float64)
            out.update({name + "/value32": v32, name + "/value64": v64, name + "/dgen32": g32, name + "/dgen64": g64,
                        name + "/floor": np.array([abs(float(v32) - float(v64)), np.abs(g32.astype(np.float64) - g64).max()])})
        for dtype, sfx in ((torch.float32, "32"), (torch.float64, "64")):
            x = torch.from_numpy(planes["gen"]).to(dtype).requires_grad_(True)
            s = retype(L.Sobelxy(), dtype)(x)
            s.backward(torch.from_numpy(planes["cot"]).to(dtype))
            out.update({"Sobelxy/out" + sfx: s.detach().numpy(), "Sobelxy/dx" + sfx: x.grad.numpy()})
        path = os.path.join(OUT, "gl_fusion_losses_%s.npz" % tag(B, H, W))
        np.savez_compressed(path, **out)
        floors = {n: out[n + "/floor"] for n in E.CRITERIA}
        n_px = B * H * W
        print("%-12s %7d bytes   worst value floor %.2e   worst |d dgen| * N %.2e   (max|dgen| * N %.1f)" % (
            tag(B, H, W), os.path.getsize(path), max(f[0] for f in floors.values()), max(f[1] for f in floors.values()) * n_px,
            max(np.abs(out[n + "/dgen64"]).max() for n in E.CRITERIA) * n_px))


if __name__ == "__main__":
    main()
