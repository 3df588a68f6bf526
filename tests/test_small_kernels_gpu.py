"""Direct float64 tests of the segmentation, evaluation and layout kernels and of the host-side weight folds that no other
test calls by name (csrc/seg_kernels.hip, csrc/seg_backward.hip, csrc/train_kernels.hip, csrc/loss_kernels.hip and the
fold kernels of csrc/conv_mfma.hip / csrc/fusion_backward.hip).

Bounds (fp32 kernels against float64 on the CPU), the ones the suite already holds these classes of kernel to:
  REV  max|err| <= 2e-5 * max|ref|          reverse kernels (tests/test_train_kernels_gpu.py)
  PW   max|err| <= 2e-6 * max(1, max|ref|)  pointwise and interpolation kernels (tests/test_seg_gpu.py)
  bit equality for the data movers.
The grid-stride kernels here cap their grid at 2048 blocks of 256 threads: one sweep is 524,288 work items, and each
family has one case beyond that.  Every test prints the error it measured."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import paif_oracle as O
from paif_amd import ops
from tests.kernel_check import PW, dev as _dev, err as _err, exact as _exact, gen, pw as _pw, rev as _rev, to_dev as _d

pytestmark = pytest.mark.gpu


def _gen(*key):
    return gen(*key, base=29)


# ---------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------
# the (M, C) of test_layernorm_affine_gradient, and C = 160, 256 (MiT-b0 stages 3, 4).  A block takes 256 / G rows
# (G = 16, 32 or 64 lanes per row): (19200, 128) is 2400 blocks of 8 rows, beyond one 2048-block sweep
LN_SHAPES = [(300, 512), (1201, 320), (4803, 64), (19200, 128), (5, 32), (777, 160), (1201, 256)]


@pytest.mark.parametrize("M,C", LN_SHAPES)
@pytest.mark.parametrize("eps", [1e-6, 1e-5])
def test_layernorm_and_layernorm_bwd(M, C, eps):
    """oracle._ln = F.layer_norm over the last axis (core/mix_transformer.py: eps 1e-6 in the blocks, 1e-5 in the patch
    embeddings) and its input gradient, with and without the `add` operand."""
    g = _gen(M, C)
    x = torch.randn(M, C, generator=g) * 1.5 + 0.3
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.1
    dy, add = torch.randn(M, C, generator=g), torch.randn(M, C, generator=g)
    xl = x.double().requires_grad_(True)
    ref = O._ln(xl, {"weight": gam.double(), "bias": bet.double()}, "", eps)
    (ref * dy.double()).sum().backward()
    tag = "%dx%d eps%g" % (M, C, eps)
    _pw("layernorm " + tag, ops.layernorm(_d(x), _d(gam), _d(bet), eps), ref)
    _rev("layernorm_bwd " + tag, ops.layernorm_bwd(_d(x), _d(gam), _d(dy), eps), xl.grad)
    _rev("layernorm_bwd add " + tag, ops.layernorm_bwd(_d(x), _d(gam), _d(dy), eps, add=_d(add)), xl.grad + add.double())


# ---------------------------------------------------------------------------------------------
# bilinear resize into a channel slice, the head's sum of four resolutions
# ---------------------------------------------------------------------------------------------
def _up(x_nhwc64, size):
    """NHWC float64 -> F.interpolate(bilinear, align_corners=False) -> NHWC."""
    return F.interpolate(x_nhwc64.permute(0, 3, 1, 2), size=size, mode="bilinear", align_corners=False).permute(0, 2, 3, 1)


# integer and non-integer ratios, up and down, the identity; the last: 2 * 150 * 203 * 64 / 4 = 974,400 float4 items,
# beyond one 524,288-item sweep
@pytest.mark.parametrize("B,IH,IW,OH,OW,C,ldo,coff", [
    (2, 5, 7, 20, 28, 8, 20, 8), (2, 5, 7, 13, 18, 8, 20, 8), (1, 23, 31, 10, 14, 4, 12, 4), (2, 24, 32, 12, 16, 8, 16, 8),
    (1, 9, 11, 9, 11, 12, 28, 16), (1, 1, 3, 8, 18, 8, 12, 4), (2, 38, 51, 150, 203, 64, 72, 4)])
def test_resize_bilinear_into(B, IH, IW, OH, OW, C, ldo, coff):
    """F.interpolate(align_corners=False) into out[..., coff:coff+C] of a wider tensor (core/segformer_head.py:66-77); the
    channels outside the slice keep the sentinel they were filled with.

    Bound.  The pointwise bound, except where fp32 interpolation itself cannot meet it: the source coordinate
    scale * (dst + 0.5) - 0.5 is formed in fp32 (as ATen forms it), so at a non-integer ratio it carries a rounding error of
    up to about one ulp of the coordinate (3.8e-6 at 32 <= coordinate < 64), and that error multiplies the difference of
    neighbouring inputs (up to ~5 for unit normal data).  torch's own fp32 F.interpolate on the CPU, against the same float64
    reference, is off by 5.4e-6 at 23x31 -> 10x14 (pointwise bound 4.7e-6) and by 1.74e-5 at 38x51 -> 150x203 (bound
    8.0e-6); at the other sizes it stays under a quarter of the bound.  So the bound is the larger of the pointwise one and
    4 x the error of that fp32 evaluation of the reference (4 x for the different order of the four products)."""
    g = _gen(B, IH, IW, OH, OW)
    x = torch.randn(B, IH, IW, C, generator=g)
    sentinel = -777.25
    out = torch.full((B, OH, OW, ldo), sentinel, device=_dev(), dtype=torch.float32)
    ret = ops.resize_bilinear_into(_d(x), out, coff)
    assert ret is out
    got = out.cpu()
    ref = _up(x.double(), (OH, OW))
    err32 = float((_up(x, (OH, OW)).double() - ref).abs().max())
    _err("resize_bilinear_into %dx%d->%dx%d" % (IH, IW, OH, OW), got[..., coff:coff + C], ref,
         max(PW * max(1.0, float(ref.abs().max())), 4.0 * err32))
    outside = torch.cat((got[..., :coff], got[..., coff + C:]), dim=-1)
    assert outside.numel() > 0 and bool((outside == sentinel).all()), "resize_bilinear_into wrote outside its channel slice"


# 1:2:4:8, and what the head meets at image sizes that are no multiple of 32: 40 x 56 and 32 x 72
# (tests/golden/gs_model_forward_ragged) give strides-4/8/16/32 maps of 10x14, 5x7, 3x4, 2x2 and 8x18, 4x9, 2x5, 1x3.
# The last: 2 * 120 * 160 * 64 / 4 = 614,400 float4 items
@pytest.mark.parametrize("B,C,sizes", [
    (2, 256, [(16, 24), (8, 12), (4, 6), (2, 3)]), (1, 12, [(10, 14), (5, 7), (3, 4), (2, 2)]), (3, 32, [(8, 18), (4, 9), (2, 5), (1, 3)]),
    (2, 64, [(120, 160), (60, 80), (30, 40), (15, 20)])])
def test_head_sum(B, C, sizes):
    """relu((z1 + up z2 + up z3 + up z4) * scale + shift): core/segformer_head.py:63-80 with linear_fuse folded in front."""
    g = _gen(B, C, *sizes[0])
    zs = [torch.randn(B, h, w, C, generator=g) for h, w in sizes]
    scale, shift = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    ref = zs[0].double()
    for z in zs[1:]:
        ref = ref + _up(z.double(), sizes[0])
    ref = F.relu(ref * scale.double() + shift.double())
    assert 0.2 < float((ref == 0).double().mean()) < 0.8
    _pw("head_sum %dx%d C%d" % (sizes[0] + (C,)), ops.head_sum([_d(z) for z in zs], _d(scale), _d(shift)), ref)


# ---------------------------------------------------------------------------------------------
# evaluation: upsample + argmax, confusion matrix
# ---------------------------------------------------------------------------------------------
# the last: 2 * 480 * 640 = 614,400 output pixels, beyond one 524,288-pixel sweep
@pytest.mark.parametrize("B,IH,IW,OH,OW", [(2, 16, 24, 64, 96), (1, 10, 14, 40, 56), (3, 8, 18, 32, 72), (2, 7, 5, 9, 11), (2, 120, 160, 480, 640)])
def test_upsample_argmax(B, IH, IW, OH, OW):
    """argmax_c of the bilinear upsample (test_original.py:180).  A pixel is judged when the float64 reference's two largest
    values are more than 1e-5 of the logit range apart; at most 0.1 % of the pixels may be left unjudged."""
    g = _gen(B, IH, IW, OH, OW)
    logits = torch.randn(B, IH, IW, 9, generator=g)
    ref = _up(logits.double(), (OH, OW))
    top = ref.topk(2, dim=-1)[0]
    judged = (top[..., 0] - top[..., 1]) > 1e-5 * float(ref.max() - ref.min())
    share = 1.0 - float(judged.double().mean())
    pred = ops.upsample_argmax(_d(logits), OH, OW).cpu()
    wrong = int(((pred != ref.argmax(-1)) & judged).sum())
    print("ERR | upsample_argmax %dx%d->%dx%d unjudged %.2e | %d | 0 wrong" % (IH, IW, OH, OW, share, wrong))
    assert share <= 1e-3
    assert pred.dtype == torch.int64 and wrong == 0


def test_upsample_argmax_equal_channels_give_the_lower_index():
    """Channels 2 and 5 are equal everywhere and above the rest: torch.argmax returns 2, and so must the kernel."""
    g = _gen(5)
    logits = torch.randn(2, 10, 14, 9, generator=g)
    top = logits.max(dim=-1)[0] + 1.0
    logits[..., 2] = top
    logits[..., 5] = top
    ref = _up(logits.double(), (40, 56)).argmax(-1)
    assert bool((ref == 2).all())
    pred = ops.upsample_argmax(_d(logits), 40, 56).cpu()
    assert bool((pred == 2).all())


# n = 3922 and 614,401 are no multiples of the 256-thread block; the second is beyond one 524,288-element sweep
@pytest.mark.parametrize("n", [3922, 100, 614401])
def test_confusion_matrix_accum(n):
    """Two accumulating calls against oracle.confusion_matrix: labels 255 (ignore), 9 and 12 (>= ncls) and -1, predictions
    outside 0..8 are dropped."""
    rng = np.random.RandomState(n)
    conf = torch.zeros(9, 9, device=_dev(), dtype=torch.int64)
    ref = np.zeros((9, 9), dtype=np.int64)
    for call in range(2):
        label = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 255, 9, 12, -1], size=n, p=[0.09] * 9 + [0.1, 0.03, 0.03, 0.03]).astype(np.int64)
        pred = rng.choice([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -1], size=n, p=[0.1] * 9 + [0.05, 0.05]).astype(np.int64)
        assert (label == 255).any() and (label >= 9).any()
        ret = ops.confusion_matrix_accum_(conf, torch.from_numpy(label).to(_dev()), torch.from_numpy(pred).to(_dev()), 9)
        assert ret is conf
        ref += O.confusion_matrix(label, pred, 9)
        got = conf.cpu().numpy()
        print("ERR | confusion_matrix_accum_ n%d call%d | %d | 0" % (n, call, int(np.abs(got - ref).max())))
        assert np.array_equal(got, ref)
    assert 0 < ref.sum() < 2 * n


# ---------------------------------------------------------------------------------------------
# data movers: bit equality with the torch expression
# ---------------------------------------------------------------------------------------------
# 37 * 53 = 1961 pixels (no multiple of 64); C = 3, 9, 5 (no multiples of 4); (2, 150, 203, 9) = 548,100 elements, beyond
# one 524,288-element sweep
@pytest.mark.parametrize("B,H,W,C", [(2, 37, 53, 3), (3, 5, 3, 9), (1, 19, 150, 32), (2, 150, 203, 9)])
def test_layout_movers_are_bit_exact(B, H, W, C):
    g = _gen(B, H, W, C)
    x = torch.randn(B, H, W, C, generator=g)
    tag = " %dx%dx%dx%d" % (B, H, W, C)
    _exact("nhwc_to_nchw" + tag, ops.nhwc_to_nchw(_d(x)), x.permute(0, 3, 1, 2).contiguous())
    y = torch.randn(B, C, H, W, generator=g)
    _exact("nchw_to_nhwc" + tag, ops.nchw_to_nhwc(_d(y)), y.permute(0, 2, 3, 1).contiguous())
    for cp in (C, 32):
        padded = torch.zeros(B, H, W, cp)
        padded[..., :C] = y.permute(0, 2, 3, 1)
        _exact("nchw_to_nhwc_pad cp%d" % cp + tag, ops.nchw_to_nhwc_pad(_d(y), cp), padded)
    for cs in (C, max(1, C - 2)):
        _exact("nhwc_slice_to_nchw C%d" % cs + tag, ops.nhwc_slice_to_nchw(_d(x), cs), x[..., :cs].permute(0, 3, 1, 2).contiguous())


# (700, 777): 777 * 704 = 547,008 elements, beyond one sweep
@pytest.mark.parametrize("N,K,npad", [(9, 256, None), (150, 37, None), (32, 5, 64), (1, 1, None), (700, 777, None)])
def test_transpose_pad_is_bit_exact(N, K, npad):
    w = torch.randn(N, K, generator=_gen(N, K))
    want = torch.zeros(K, npad or (N + 31) // 32 * 32)
    want[:, :N] = w.t()
    _exact("transpose_pad %dx%d" % (N, K), ops.transpose_pad(_d(w), npad), want)


# 2 * 150 * 203 * 16 = 974,400 float4 items, beyond one sweep
@pytest.mark.parametrize("B,H,W", [(2, 37, 53), (1, 5, 3), (2, 150, 203)])
def test_decomp_cat_is_bit_exact(B, H, W):
    """(cat(LF0, LF1), cat(x - LF0, x - LF1)) on the channel axis (core/model_fusion_auto.py:522-535): one fp32 subtraction."""
    g = _gen(B, H, W)
    x, lf = torch.randn(B, H, W, 32, generator=g), torch.randn(2, B, H, W, 32, generator=g)
    lfc, hfc = ops.decomp_cat(_d(x), _d(lf))
    _exact("decomp_cat lf %dx%dx%d" % (B, H, W), lfc, torch.cat((lf[0], lf[1]), dim=-1))
    _exact("decomp_cat hf %dx%dx%d" % (B, H, W), hfc, torch.cat((x - lf[0], x - lf[1]), dim=-1))


# (8200, 256): 524,800 float4 items, beyond one sweep
@pytest.mark.parametrize("M,C", [(1961, 12), (5, 4), (777, 256), (8200, 256)])
def test_relu_mask_scale_is_bit_exact(M, C):
    """d_pre = d_x * scale[c] where x > 0, else 0 (backward of the head's folded BatchNorm + ReLU): one fp32 product.
    x is a ReLU output, about half of it exactly 0."""
    g = _gen(M, C)
    x = F.relu(torch.randn(M, C, generator=g))
    dx, scale = torch.randn(M, C, generator=g), torch.randn(C, generator=g)
    assert 0.3 < float((x == 0).float().mean()) < 0.7
    _exact("relu_mask_scale %dx%d" % (M, C), ops.relu_mask_scale(_d(dx), _d(x), _d(scale)), torch.where(x > 0, dx * scale, torch.zeros(())))


# (3, 3, 260, 301) = 704,340 elements, beyond one 1024-block sweep of this kernel (262,144) and one of 2048 blocks
@pytest.mark.parametrize("B,C,H,W", [(2, 3, 37, 53), (1, 5, 5, 3), (3, 3, 260, 301)])
def test_channel_affine_nchw_is_bit_exact(B, C, H, W):
    """out = x * scale[c] + shift[c] as ONE fused multiply-add per element: the product of two fp32 numbers is exact in
    float64, so the float64 expression rounded to fp32 is that fma up to a double rounding: the float64 sum is rounded once
    more on the way to fp32, which differs from the fma only when that sum lands exactly on an fp32 rounding midpoint (about
    one element in 2^29).  The fixed seeds here do not hit it; if a change of seed does, it is this and not the kernel.
    Without a shift the reference is the fp32 product."""
    g = _gen(B, C, H, W)
    x, scale, shift = torch.randn(B, C, H, W, generator=g), torch.randn(C, generator=g), torch.randn(C, generator=g)
    sc, sh = scale.view(1, C, 1, 1), shift.view(1, C, 1, 1)
    tag = " %dx%dx%dx%d" % (B, C, H, W)
    _exact("channel_affine_nchw" + tag, ops.channel_affine_nchw(_d(x), _d(scale), _d(shift)), (x.double() * sc.double() + sh.double()).float())
    _exact("channel_affine_nchw no shift" + tag, ops.channel_affine_nchw(_d(x), _d(scale)), x * sc)


# ---------------------------------------------------------------------------------------------
# host-side weight folds
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [32, 256, 37])
def test_bn_fold_and_bn_eval_stats(C):
    """Eval-mode BatchNorm as scale = gamma / sqrt(var + eps), shift = beta - mean * scale; bn_eval_stats also returns
    (mean, invstd = 1 / sqrt(var + eps))."""
    g = _gen(C)
    gam, bet = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g)
    mean, var = torch.randn(C, generator=g), torch.rand(C, generator=g) * 2 + 0.01
    eps = 1e-5
    invstd = 1.0 / torch.sqrt(var.double() + eps)
    scale = gam.double() * invstd
    shift = bet.double() - mean.double() * scale
    s, h = ops.bn_fold(_d(gam), _d(bet), _d(mean), _d(var), eps)
    _pw("bn_fold scale C%d" % C, s, scale)
    _pw("bn_fold shift C%d" % C, h, shift)
    m2, i2, s2, h2 = ops.bn_eval_stats(_d(gam), _d(bet), _d(mean), _d(var), eps)
    assert torch.equal(m2.cpu(), mean)
    _pw("bn_eval_stats invstd C%d" % C, i2, invstd)
    _pw("bn_eval_stats scale C%d" % C, s2, scale)
    _pw("bn_eval_stats shift C%d" % C, h2, shift)
    # the folded pair IS the BatchNorm: F.batch_norm in eval mode on a small map
    x = torch.randn(2, C, 5, 7, generator=g).double()
    bn = F.batch_norm(x, mean.double(), var.double(), gam.double(), bet.double(), False, 0.0, eps)
    _pw("bn_fold applied C%d" % C, x * s.cpu().double().view(1, C, 1, 1) + h.cpu().double().view(1, C, 1, 1), bn)


@pytest.mark.parametrize("k,dil", [(3, 2), (5, 1), (3, 1)])
def test_compose_dw_pw_weight(k, dil):
    """W[co][ci][tap] = pw[co][ci] * dw[ci][tap]: the dense kernel of conv1x1(dwconv(.)) (DilConv, operations_m.py:494-506)."""
    g = _gen(k, dil)
    dw, pw = torch.randn(32, 1, k, k, generator=g) * 0.3, torch.randn(32, 32, 1, 1, generator=g) * 0.2
    ref = pw.double()[:, :, 0, 0, None, None] * dw.double()[None, :, 0]
    got = ops.compose_dw_pw_weight(_d(dw), _d(pw))
    _pw("compose_dw_pw_weight k%d" % k, got, ref)
    x = torch.randn(2, 32, 9, 11, generator=g).double()
    pad = dil * (k - 1) // 2
    two = F.conv2d(F.conv2d(x, dw.double(), None, 1, pad, dil, 32), pw.double())
    _pw("compose_dw_pw_weight conv k%d d%d" % (k, dil), F.conv2d(x, got.cpu().double(), None, 1, pad, dil), two)


@pytest.mark.parametrize("Co,Cm,Ci,k", [(32, 32, 32, 3), (16, 24, 8, 5), (32, 32, 32, 1)])
def test_compose_pw_conv_weight(Co, Cm, Ci, k):
    """W[co][ci][tap] = sum_m pw[co][m] * w[m][ci][tap]: the dense kernel of conv1x1(conv_kxk(.)) (ResidualModule,
    operations_m.py:451-464: the 3x3 dilation 2 conv and the 1x1 behind it)."""
    g = _gen(Co, Cm, Ci, k)
    w, pw = torch.randn(Cm, Ci, k, k, generator=g) * 0.1, torch.randn(Co, Cm, 1, 1, generator=g) * 0.2
    ref = torch.einsum("om,mikl->oikl", pw.double()[:, :, 0, 0], w.double())
    got = ops.compose_pw_conv_weight(_d(pw), _d(w))
    _pw("compose_pw_conv_weight %dx%dx%d k%d" % (Co, Cm, Ci, k), got, ref)
    x = torch.randn(2, Ci, 10, 9, generator=g).double()
    pad = 2 * (k - 1) // 2
    two = F.conv2d(F.conv2d(x, w.double(), None, 1, pad, 2), pw.double())
    _pw("compose_pw_conv_weight conv k%d" % k, F.conv2d(x, got.cpu().double(), None, 1, pad, 2), two)


def test_fold_decomp1x1_weight():
    """The decomposition's 1x1 over cat(LF1, LF2, x - LF1, x - LF2) (core/model_fusion_auto.py:492-535) folded to a
    [32, 96, 1, 1] weight over cat(x, LF1, LF2): (w[64:96] + w[96:128], w[0:32] - w[64:96], w[32:64] - w[96:128])."""
    g = _gen(128)
    w = torch.randn(32, 128, 1, 1, generator=g) * 0.2
    w64 = w.double()
    ref = torch.cat((w64[:, 64:96] + w64[:, 96:128], w64[:, 0:32] - w64[:, 64:96], w64[:, 32:64] - w64[:, 96:128]), dim=1)
    got = ops.fold_decomp1x1_weight(_d(w))
    _pw("fold_decomp1x1_weight", got, ref)
    x, lf1, lf2 = (torch.randn(2, 32, 6, 7, generator=g).double() for _ in range(3))
    direct = F.conv2d(torch.cat((lf1, lf2, x - lf1, x - lf2), 1), w64)
    _pw("fold_decomp1x1_weight conv", F.conv2d(torch.cat((x, lf1, lf2), 1), got.cpu().double()), direct)
