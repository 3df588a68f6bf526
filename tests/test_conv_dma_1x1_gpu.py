"""GPU tests of conv_h16_dma_1x1 (csrc/conv_dma_1x1.hip): the folded decomposition 1x1 -- three 16-bit NHWC-32 maps, plain 16-bit
weights, no residual maps -- as a streaming LDS-DMA kernel.

1. Bit-equality with the kernel it replaces (conv_bf16x3_ws<1, 1, 4 | 12>): the same MFMAs in the same order and the same epilogue
   expression must give the same 16-bit patterns.  The switch PAIF_CONV_DMA1X1 is read once per process, so the old kernel's results come
   from a fresh child process (this file run as a script with PAIF_CONV_DMA1X1=0) that writes one .npy per case.
2. The dispatch rule, through ops.conv2d_kernel_name.
3. Against float64 on the CPU for a ragged shape (tolerance of tests/test_f16_storage_gpu.py's _close(..., frac=1e-4)), so the file also
   stands once the old kernel is removed."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from paif_amd import _lib, ops  # noqa: E402

pytestmark = pytest.mark.gpu

FMTS = ["f16", "bf16"]
# (8, 480, 640): the benchmarked shape; (2, 333, 517): ragged, above the dispatch threshold (1428 tiles of 8 x 32, 344322 pixels = 5380 runs
# of 64 + 2); (1, 97, 131) and (4, 96, 100): below it (both processes run the tile-per-workgroup kernel)
SHAPES = [(8, 480, 640), (2, 333, 517), (1, 97, 131), (4, 96, 100)]
# epilogue forms: the decomposition cell's own (bias only), and the rest of paif_conv_desc's affine / activation fields
VARIANTS = ["bias", "scale_alpha", "prelu", "relu_alpha"]
NEW, OLD = "conv_h16_dma_1x1<%d>", "conv_bf16x3_ws<1, 1, %d>"


def _cases():
    for fmt in FMTS:
        for shape in SHAPES:
            for var in VARIANTS:
                if shape == SHAPES[0] and var != "bias":
                    continue          # the full-size maps once per format
                yield fmt, shape, var


def _key(fmt, shape, var):
    return "%s_%dx%dx%d_%s" % ((fmt,) + tuple(shape) + (var,))


def _dt(fmt):
    return torch.float16 if fmt == "f16" else torch.bfloat16


def _big(shape):
    B, H, W = shape
    return B * ((H + 7) // 8) * ((W + 31) // 32) >= 1024


def _inputs(fmt, shape, var):
    """Deterministic maps / weights (values representable in the format), on the GPU."""
    B, H, W = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(4000 + 7 * W + VARIANTS.index(var) + (100 if fmt == "bf16" else 0))
    dt = _dt(fmt)
    xs = [ops.cast_storage(torch.randn(B, H, W, 32, generator=g).to(dev), dt) for _ in range(3)]
    w = (torch.randn(32, 96, 1, 1, generator=g) * 0.05).to(dev).to(dt).float()
    scale = (torch.rand(32, generator=g) + 0.5).to(dev)
    shift = (torch.randn(32, generator=g) * 0.1).to(dev)
    slope = torch.tensor([0.2], device=dev)
    kw = dict(shift=shift)
    if var == "scale_alpha":
        kw.update(scale=scale, alpha=0.3)
    elif var == "prelu":
        kw.update(scale=scale, act=ops.ACT_PRELU, prelu=slope, alpha=0.7)
    elif var == "relu_alpha":
        kw.update(act=ops.ACT_RELU, alpha=1.5)
    return xs, w, kw


def _desc(fmt, nsrc=3, nres=0, storage=None, precision=None):
    d = _lib.ConvDesc()
    one = ctypes.c_void_p(16)         # (only null / non-null matters to the name query)
    for i in range(3):
        d.src[i] = one if i < nsrc else None
        d.res[i] = one if i < nres else None
    d.wpk, d.out = one, one
    d.nsrc, d.cin, d.cout, d.kh, d.dil, d.alpha = nsrc, 32, 32, 1, 1, 1.0
    d.storage = (3 if fmt == "f16" else 1) if storage is None else storage
    d.precision = (4 if fmt == "f16" else ops.PREC_BF16) if precision is None else precision
    return d


def _run(fmt, shape, var):
    xs, w, kw = _inputs(fmt, shape, var)
    old = dict(ops.CONFIG)
    try:
        ops.set_storage(fmt)          # (bf16: conv2d then takes the pack's hi halves as plain bf16 weights)
        wpk = ops.pack_conv_weight(w, 3, 32, 1, precision="f16" if fmt == "f16" else "bf16x3")
        out = ops.conv2d(xs, wpk, 1, 1, **kw)
        torch.cuda.synchronize()
    finally:
        ops.CONFIG.update(old)
        ops._ACT_BF16[0] = False
    assert out.dtype == _dt(fmt) and tuple(out.shape) == tuple(shape) + (32,)
    return out


def _child(outdir):
    """PAIF_CONV_DMA1X1=0: every case on the kernel the parent commit runs; raw 16-bit patterns to <outdir>/<key>.npy."""
    assert os.environ.get("PAIF_CONV_DMA1X1") == "0"
    for fmt in FMTS:
        code = 12 if fmt == "f16" else 4
        assert ops.conv2d_kernel_name(_desc(fmt), 8, 480, 640) == OLD % code          # the switch off: the parent's name
    for fmt, shape, var in _cases():
        out = _run(fmt, shape, var)
        np.save(os.path.join(outdir, _key(fmt, shape, var) + ".npy"), out.view(torch.int16).cpu().numpy())
    print("child ok")


@pytest.fixture(scope="module")
def old_kernel_outputs(tmp_path_factory):
    outdir = str(tmp_path_factory.mktemp("conv1x1_old"))
    env = dict(os.environ, PAIF_CONV_DMA1X1="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), outdir], env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       timeout=600)
    assert r.returncode == 0 and b"child ok" in r.stdout, r.stdout.decode(errors="replace")[-3000:]
    return outdir


@pytest.mark.parametrize("fmt,shape,var", list(_cases()), ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_bit_equal_to_the_register_staged_kernel(old_kernel_outputs, fmt, shape, var):
    assert os.environ.get("PAIF_CONV_DMA1X1", "1") != "0", "run this test with the switch on"
    name = ops.conv2d_kernel_name(_desc(fmt), *shape)
    assert name.startswith("conv_h16_dma_1x1<") == _big(shape), name
    out = _run(fmt, shape, var).view(torch.int16).cpu()
    ref = torch.from_numpy(np.load(os.path.join(old_kernel_outputs, _key(fmt, shape, var) + ".npy")))
    ndiff = int((out != ref).sum())
    print("%s: %d of %d 16-bit patterns differ" % (_key(fmt, shape, var), ndiff, out.numel()))
    assert torch.equal(out, ref), ndiff


def test_dispatch_rule():
    assert os.environ.get("PAIF_CONV_DMA1X1", "1") != "0", "run this test with the switch on"
    B, H, W = 8, 480, 640
    name = ops.conv2d_kernel_name
    assert name(_desc("f16"), B, H, W) == NEW % 2
    assert name(_desc("bf16"), B, H, W) == NEW % 1
    assert name(_desc("f16"), 2, 333, 517) == NEW % 2
    # everything else keeps its kernel
    assert name(_desc("f16", nsrc=1), B, H, W) == "conv_bf16x3_ws<1, 1, 12>"
    assert name(_desc("f16", nsrc=2), B, H, W) == "conv_bf16x3_ws<1, 1, 12>"
    assert name(_desc("f16", nres=1), B, H, W) == "conv_mfma_bf16x3<1, 1, false, 12>"
    assert name(_desc("bf16", nres=1), B, H, W) == "conv_mfma_bf16x3<1, 1, false, 4>"
    assert name(_desc("f16", precision=5), B, H, W) == "conv_bf16x3_ws<1, 1, 9>"             # fp16 maps, hi + lo weight pieces
    assert name(_desc("bf16", precision=1), B, H, W) == "conv_bf16x3_ws<1, 1, 1>"            # bf16 maps, split-bf16 weights
    assert name(_desc("bf16", storage=2, precision=1), B, H, W) == "conv_bf16x3_ws<1, 1, 2>"  # fp32 in / bf16 out
    assert name(_desc("f16", storage=0, precision=1), B, H, W) == "conv_bf16x3_ws<1, 1, 0>"   # fp32 storage
    assert name(_desc("f16"), 2, 64, 96) == "conv_mfma_bf16x3<1, 1, false, 12>"               # a small image
    assert name(_desc("f16"), 1, 97, 131) == "conv_mfma_bf16x3<1, 1, false, 12>"
    d = _desc("f16")
    d.in_act = 2
    assert not name(d, B, H, W).startswith("conv_h16_dma_1x1")
    d = _desc("f16")
    d.kh = 3
    assert name(d, B, H, W) == "conv3x3_h16_dma<3, 0, 2, false, 1, 0>"


@pytest.mark.parametrize("fmt", FMTS)
def test_against_float64_on_a_ragged_shape(fmt):
    """out = rn16(act(scale * (sum_k w x) + shift) * alpha) against float64 on the CPU; inputs and weights are values of the format, so
    the products are exact and the error is the fp32 accumulation plus the rounding of the output: half an ulp of the format, a
    fraction 1e-4 of the elements on the other neighbour (test_f16_storage_gpu._close(..., frac=1e-4))."""
    shape, var = (2, 333, 517), "prelu"
    xs, w, kw = _inputs(fmt, shape, var)
    out = _run(fmt, shape, var).float().cpu().double()
    x = torch.cat([x_.float().cpu().double() for x_ in xs], dim=-1)                     # [B,H,W,96]
    z = x @ w.view(32, 96).cpu().double().t()
    z = z * kw["scale"].cpu().double() + kw["shift"].cpu().double()
    z = torch.where(z >= 0, z, z * float(kw["prelu"].float().cpu()[0])) * kw["alpha"]
    eps = 2.0 ** -11 if fmt == "f16" else 2.0 ** -8
    err = (out - z).abs()
    tol = eps * z.abs() * 1.01 + 1e-5
    bad = err > tol
    print("%s: max |err| %.3e, %d of %d beyond half an ulp" % (fmt, float(err.max()), int(bad.sum()), bad.numel()))
    assert float(bad.double().mean()) < 1e-4 and bool((err <= 2 * tol).all()), (int(bad.sum()), float(err.max()))


if __name__ == "__main__":
    _child(sys.argv[1])
