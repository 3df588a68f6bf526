"""Direct float64 tests of the hand-written reverse pass and of the fusion -> segmentation glue (csrc/fusion_backward.hip,
csrc/glue_backward.hip, csrc/object_glue.hip, csrc/loss_kernels.hip and the dgrad use of the dense conv).

Every test calls one `ops.*` wrapper and compares it with torch autograd over a float64 restatement of the same operator
on the CPU (oracle/paif_oracle.py where it has one), so a failure names one kernel.  The inputs are float32 values, so both
sides see the same numbers.

Bounds (fp32 kernels against float64), the ones the suite already holds these classes of kernel to:
  REV  max|err| <= 2e-5 * max|ref|          reverse kernels (tests/test_train_kernels_gpu.py)
  PW   max|err| <= 2e-6 * max(1, max|ref|)  pointwise kernels (tests/test_seg_gpu.py)
  dense dgrad conv: 2e-5 * max|ref| ("f32") and 1e-4 * max|ref| ("bf16x3"), as tests/test_fusion_gpu.py holds the forward conv.

Shapes.  The grid-stride kernels cap their grid at MAXGRID = 2048 blocks; a block takes 32 pixels (64 in tail_bwd, 256 in
the glue kernels).  Each kernel gets a map smaller than its stencil, two ragged multi-block maps whose pixel groups straddle
the image boundary (37 * 53 = 1961 pixels per image is no multiple of 32, 64, 1024 or 2048) and one map on which the second
sweep of the grid-stride loop runs and ends in a partial block.  Every test prints the error it measured."""
import pytest
import torch
import torch.nn.functional as F

from oracle import paif_oracle as O
from paif_amd import ops
from tests.kernel_check import dev as _dev, gen as _gen, pw as _pw, rev as _rev, to_dev as _d

pytestmark = pytest.mark.gpu

# 32 pixels per block: one sweep = 2048 * 32 = 65,536 pixels.  3 * 150 * 203 = 91,350: the second sweep takes the other
# 25,814 = 806 * 32 + 22 pixels, so it runs and its last block is partial
SHAPES32 = [(1, 5, 3), (2, 37, 53), (3, 19, 150), (3, 150, 203)]
# 64 pixels per block (tail_bwd): one sweep = 2048 * 64 = 131,072 pixels.  2 * 260 * 301 = 156,520: the second sweep takes
# 25,448 = 397 * 64 + 40 pixels
SHAPES64 = [(1, 5, 3), (2, 37, 53), (3, 19, 150), (2, 260, 301)]
# 256 pixels per block (glue_bwd apply, plane_clamp_minmax normalise / apply, rgb2ycrcb_bwd): one sweep = 2048 * 256 =
# 524,288 pixels.  2 * 520 * 601 = 625,040: the second sweep takes 100,752 = 393 * 256 + 144 pixels.  Their reduction
# passes take 2048 pixels per block without a cap: 1961-pixel images straddle those blocks
SHAPES256 = [(1, 5, 3), (2, 37, 53), (3, 19, 150), (2, 520, 601)]
# ECA: B = 3 (three gates); 1961 = 1024 + 937 and 19 * 150 = 2850 = 2 * 1024 + 802 leave a ragged last block of the
# ECA_PIX_PER_BLOCK = 1024 reduction; (3, 150, 203): see SHAPES32
SHAPES_ECA = [(3, 5, 3), (2, 37, 53), (3, 37, 53), (3, 19, 150), (3, 150, 203)]


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _rand(g, *shape):
    return torch.rand(*shape, generator=g)


def _nhwc(x):
    """CPU NCHW (any float dtype) -> dense fp32 NHWC on the device."""
    return x.detach().float().permute(0, 2, 3, 1).contiguous().to(_dev())


def _nchw(y):
    """device NHWC -> CPU NCHW float64."""
    return y.permute(0, 3, 1, 2).cpu().double()


def _leaf(x):
    return x.detach().double().requires_grad_(True)


def _tag(*a):
    return "x".join(str(v) for v in a)


# ---------------------------------------------------------------------------------------------
# depthwise dgrad
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES32)
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 2), (5, 1), (5, 2)])
def test_dwconv_bwd(k, dil, B, H, W):
    """out = dwconv^T(dt) * (aux > 0) + add against autograd of the depthwise F.conv2d (behind a ReLU when `aux` is given:
    DilConv / SepConv, operations_m.py:494-525).  aux is itself a ReLU output: about half of it is exactly 0, where
    torch's ReLU passes no gradient either.  The padding P = dil * (k - 1) / 2 reaches 4: (1, 5, 3) is narrower than it."""
    g = _gen(k, dil, B, H, W)
    w = _randn(g, 32, 1, k, k) * 0.3
    dt = _randn(g, B, 32, H, W)
    x = F.relu(_randn(g, B, 32, H, W))
    add = _randn(g, B, 32, H, W)
    assert float((x == 0).float().mean()) > 0.3
    refs = {}
    for relu in (False, True):
        xl = _leaf(x)
        t = F.conv2d(F.relu(xl) if relu else xl, w.double(), None, 1, dil * (k - 1) // 2, dil, 32)
        (t * dt.double()).sum().backward()
        refs[relu] = xl.grad
    dtn, auxn, addn, wd = _nhwc(dt), _nhwc(x), _nhwc(add), _d(w)
    for has_aux in (False, True):
        for has_add in (False, True):
            got = ops.dwconv_bwd(dtn, wd, k, dil, aux=auxn if has_aux else None, add=addn if has_add else None)
            ref = refs[has_aux] + (add.double() if has_add else 0.0)
            _rev("dwconv_bwd k%d d%d aux%d add%d %s" % (k, dil, has_aux, has_add, _tag(B, H, W)), _nchw(got), ref)


def test_dwconv_bwd_unbuilt_kernel_size_raises():
    dt = torch.zeros(1, 4, 4, 32, device=_dev())
    with pytest.raises(RuntimeError, match="not built"):
        ops.dwconv_bwd(dt, torch.zeros(32, 1, 7, 7, device=_dev()), 7, 1)
    with pytest.raises(RuntimeError, match="not built"):
        ops.dwconv_bwd(dt, torch.zeros(32, 1, 3, 3, device=_dev()), 3, 3)


# ---------------------------------------------------------------------------------------------
# dense dgrad conv: pack_conv_dgrad_weight + conv2d
# ---------------------------------------------------------------------------------------------
# (Co, Ctot, k, dil) of every forward conv whose input gradient operations_m.py / core/model_fusion_auto.py ask for:
#   ResidualDenseBlock conv1/2/3 (Denseblocks_3_1, _5_2, _7_1): Ctot = 32, 64, 96, one dgrad per 32-channel source slice
#   ResidualModule (Residualblocks_7_1, _3_2, _5_2): its k x k conv, the 3x3 dilation 2 behind it, the 1x1
#   DilConv / SepConv: the 1x1;  ECA / SPA blocks: conv1 3x3 and conv2 k = 3
#   the folded decomposition 1x1 [32, 96, 1, 1] (three slices);  stem_out.0 [16, 32, 3, 3] (cin = 16: always "f32")
DGRAD_CONVS = [(32, 32, 3, 1), (32, 64, 3, 1), (32, 96, 3, 1), (32, 32, 5, 2), (32, 64, 5, 2), (32, 96, 5, 2),
               (32, 32, 7, 1), (32, 64, 7, 1), (32, 96, 7, 1), (32, 32, 3, 2), (32, 32, 1, 1), (32, 96, 1, 1), (16, 32, 3, 1)]
DGRAD_BOUND = {"f32": 2e-5, None: 1e-4}      # None = the default pack, "bf16x3"
DGRAD_BIG = {(32, 32, 1, 1), (32, 32, 3, 1), (32, 32, 5, 2), (32, 32, 7, 1)}     # SHAPES32[3] once per kernel size


def _dgrad_case(Co, Ctot, k, dil, B, H, W):
    g = _gen(Co, Ctot, k, dil, B, H, W)
    w = _randn(g, Co, Ctot, k, k) * 0.05
    dy = _randn(g, B, Co, H, W)
    xl = _leaf(torch.zeros(B, Ctot, H, W))
    (F.conv2d(xl, w.double(), None, 1, dil * (k - 1) // 2, dil) * dy.double()).sum().backward()
    dyn, wd = _nhwc(dy), _d(w)
    assert ops.CONFIG["conv_precision"] == "bf16x3"
    for coff in range(0, Ctot, 32):
        ref = xl.grad[:, coff:coff + 32]
        for prec, rel in DGRAD_BOUND.items():
            wpk = ops.pack_conv_dgrad_weight(wd, coff, 32, precision=prec)
            got = ops.conv2d([dyn], wpk, k, dil, cin=Co, cout=32)
            _rev("dgrad conv %s coff%d %s %s" % (_tag(Co, Ctot, k, dil), coff, prec or "bf16x3", _tag(B, H, W)), _nchw(got), ref,
                 rel=rel)


@pytest.mark.parametrize("Co,Ctot,k,dil", DGRAD_CONVS)
def test_dense_conv_input_gradient(Co, Ctot, k, dil):
    """d/dx of F.conv2d(x, w) for every coff slice, as the k x k conv with cin = Co of pack_conv_dgrad_weight's rotated,
    transposed weights."""
    for B, H, W in SHAPES32[:3]:
        _dgrad_case(Co, Ctot, k, dil, B, H, W)
    if (Co, Ctot, k, dil) in DGRAD_BIG:
        _dgrad_case(Co, Ctot, k, dil, *SHAPES32[3])


# ---------------------------------------------------------------------------------------------
# ECA block
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES_ECA)
@pytest.mark.parametrize("k", [3, 5])
def test_eca_bwd(k, B, H, W):
    """out = PReLU(o * gate + r), gate = sigmoid(conv1d_k(mean_hw o)): the tail of oracle.eca_basic_block.  d_o, d_r and the
    per-image sums dgate = d loss / d gate against autograd (the gate as a leaf gives dgate); coef, the gradient that reaches
    every pixel of o through the pooled mean, against conv1d^T(dgate * g * (1 - g)) / (H * W) written out: d_o IS coef at the
    pixels where dout is 0, and two pixels per image are made so.  A slip in the 1 / (H * W) factor shows in the coef check at
    the small shapes (H * W against H * W + 1 is 6 % at 5 x 3, 5e-4 at 37 x 53, 3.5e-4 at 19 x 150); at 150 x 203 it is 3.3e-5,
    next to the bound."""
    g = _gen(k, B, H, W)
    o = _randn(g, B, 32, H, W) + torch.tensor([-1.2, 0.1, 1.4])[:B].view(B, 1, 1, 1)
    r = _randn(g, B, 32, H, W)
    dout = _randn(g, B, 32, H, W) + 0.3
    dout[:, :, 0, 0] = 0.0
    dout[:, :, H - 1, W - 1] = 0.0
    w1d = _randn(g, 1, 1, k) * 0.8
    a = torch.tensor([0.2])
    ol, rl = _leaf(o), _leaf(r)
    y = F.conv1d(ol.mean(dim=(2, 3), keepdim=True).squeeze(-1).transpose(-1, -2), w1d.double(), None, 1, (k - 1) // 2)
    gate = torch.sigmoid(y.transpose(-1, -2).unsqueeze(-1))          # oracle.eca_basic_block, operations_m.py:353-367
    u = ol * gate + rl
    (F.prelu(u, a.double()) * dout.double()).sum().backward()
    # the gate as a leaf: d loss / d gate[b, c] = sum_px du * o
    gl = _leaf(gate)
    (F.prelu(o.double() * gl + r.double(), a.double()) * dout.double()).sum().backward()
    dgate = gl.grad.reshape(B, 32)
    g2 = gate.detach().reshape(B, 32)
    if B == 3:      # three visibly different gates
        assert min(float((g2[i] - g2[j]).abs().max()) for i, j in ((0, 1), (0, 2), (1, 2))) > 0.05
    un, on_ = _nhwc(u), _nhwc(o)
    gated = g2.float().contiguous().to(_dev())
    args = (_nhwc(dout), un, on_, gated, _d(w1d), k, _d(a))
    d_o, d_r = ops.eca_bwd(*args)
    d_o2, d_r2, partial = ops.eca_bwd(*args, want_partial=True)
    assert torch.equal(d_o, d_o2) and torch.equal(d_r, d_r2)
    tag = "k%d %s" % (k, _tag(B, H, W))
    _rev("eca_bwd d_o " + tag, _nchw(d_o), ol.grad)
    _rev("eca_bwd d_r " + tag, _nchw(d_r), rl.grad)
    assert tuple(partial.shape) == (B, (H * W + 1023) // 1024, 32)
    _rev("eca_bwd partial " + tag, partial.sum(1), dgate)
    dy = dgate * g2 * (1 - g2)
    coef = torch.zeros(B, 32, dtype=torch.float64)
    pad = (k - 1) // 2
    for c in range(32):
        for j in range(k):            # y[cc] = sum_j w[j] * mean[cc + j - pad]  ->  d mean[c] = sum_j w[j] * dy[c - j + pad]
            cc = c - j + pad
            if 0 <= cc < 32:
                coef[:, c] += dy[:, cc] * float(w1d[0, 0, j])
    coef /= H * W
    for yy, xx in ((0, 0), (H - 1, W - 1)):
        _rev("eca_bwd coef " + tag, d_o[:, yy, xx, :], coef)


# ---------------------------------------------------------------------------------------------
# spatial attention: the two-stream blend and the SPAattention block
# ---------------------------------------------------------------------------------------------
def _plant_ties(x, g, stride, pairs=((3, 4), (0, 31))):
    """At every `stride`-th pixel (a different phase per pair) make two channels share the channel maximum exactly."""
    B, C, H, W = x.shape
    flat = x.permute(0, 2, 3, 1).reshape(-1, C).clone()
    idx = []
    for n, (c0, c1) in enumerate(pairs):
        rows = torch.arange(n * (stride // 2), flat.shape[0], stride)
        top = flat[rows].max(dim=1)[0] + 0.75
        flat[rows, c0] = top
        flat[rows, c1] = top
        idx.append((rows, c0, c1))
    return flat.reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous(), idx


def _assert_lowest_index_wins(x, idx):
    """The premise of the tie tests: torch.max(dim) on the CPU returns (and routes its gradient to) the lowest tied index."""
    arg = x.permute(0, 2, 3, 1).reshape(-1, x.shape[1]).max(dim=1)[1]
    for rows, c0, _ in idx:
        assert rows.numel() > 0 and bool((arg[rows] == c0).all())


def _spa_blend_case(B, H, W, ties):
    g = _gen(B, H, W, ties)
    ir, vis = _randn(g, B, 32, H, W), _randn(g, B, 32, H, W) * 1.3 + 0.2
    idx_i = idx_v = ()
    if ties:
        ir, idx_i = _plant_ties(ir, g, 7)
        vis, idx_v = _plant_ties(vis, g, 5)
    w = _randn(g, 1, 4, 5, 5) * 0.2
    dagg = _randn(g, B, 32, H, W)
    add_i, add_v = _randn(g, B, 32, H, W), _randn(g, B, 32, H, W)
    il, vl = _leaf(ir), _leaf(vis)
    _assert_lowest_index_wins(il.detach(), idx_i)
    _assert_lowest_index_wins(vl.detach(), idx_v)
    comp = torch.cat((il.max(1, keepdim=True)[0], il.mean(1, keepdim=True), vl.max(1, keepdim=True)[0], vl.mean(1, keepdim=True)), 1)
    pre = O.basic_conv(comp, w.double(), 5, 1)
    pre.retain_grad()
    s = torch.sigmoid(pre)
    s_oracle = O.spatial_attn_m(il.detach(), vl.detach(), {"spatial.conv.weight": w.double()}, "")
    assert float((s.detach() - s_oracle).abs().max()) <= 1e-14
    ((s * il + (1 - s) * vl) * dagg.double()).sum().backward()       # core/model_fusion_auto.py:631
    irn, visn, sn = _nhwc(ir), _nhwc(vis), s.detach().float()[:, 0].contiguous().to(_dev())
    tag = "%s%s" % (_tag(B, H, W), " ties" if ties else "")
    for has_add in (False, True):
        d_ir, d_vis, dpre = ops.spa_blend_bwd(_nhwc(dagg), _d(w), irn, visn, sn, add_ir=_nhwc(add_i) if has_add else None,
                                              add_vis=_nhwc(add_v) if has_add else None, want_dpre=True)
        _rev("spa_blend_bwd d_ir add%d %s" % (has_add, tag), _nchw(d_ir), il.grad + (add_i.double() if has_add else 0.0))
        _rev("spa_blend_bwd d_vis add%d %s" % (has_add, tag), _nchw(d_vis), vl.grad + (add_v.double() if has_add else 0.0))
        _rev("spa_blend_bwd dpre add%d %s" % (has_add, tag), dpre, pre.grad[:, 0])
    two = ops.spa_blend_bwd(_nhwc(dagg), _d(w), irn, visn, sn)
    assert len(two) == 2 and torch.equal(two[0], ops.spa_blend_bwd(_nhwc(dagg), _d(w), irn, visn, sn, want_dpre=True)[0])


@pytest.mark.parametrize("B,H,W", SHAPES32)
def test_spa_blend_bwd(B, H, W):
    """agg = s * ir + (1 - s) * vis, s = oracle.spatial_attn_m(ir, vis): d_ir, d_vis (with and without add_ir / add_vis) and
    dpre = d loss / d(conv output in front of the sigmoid).  The 5 x 5 stencil is wider than the (1, 5, 3) map."""
    _spa_blend_case(B, H, W, False)


@pytest.mark.parametrize("B,H,W", [(2, 37, 53)])
def test_spa_blend_bwd_routes_a_tied_maximum_to_the_lowest_channel(B, H, W):
    """At every 7th (ir) / 5th (vis) pixel channels (3, 4), resp. (0, 31), share the maximum exactly: pairs that sit in
    different 4-channel lane groups.  The max-pool gradient must land on the lower index only, as torch.max(dim) does."""
    _spa_blend_case(B, H, W, True)


def _spa1_case(k, B, H, W, ties):
    g = _gen(k, B, H, W, ties)
    o, r = _randn(g, B, 32, H, W), _randn(g, B, 32, H, W)
    idx = ()
    if ties:
        o, idx = _plant_ties(o, g, 7)
    w = _randn(g, 1, 2, k, k) * (0.6 / k)
    a = torch.tensor([0.25])
    dout = _randn(g, B, 32, H, W)
    ol, rl = _leaf(o), _leaf(r)
    _assert_lowest_index_wins(ol.detach(), idx)
    comp = torch.cat((ol.max(1, keepdim=True)[0], ol.mean(1, keepdim=True)), 1)       # oracle.spatial_basic_block
    pre = O.basic_conv(comp, w.double(), k, 1)
    pre.retain_grad()
    s = torch.sigmoid(pre)
    u = ol * s + rl
    out = F.prelu(u, a.double())
    (out * dout.double()).sum().backward()
    tag = "k%d %s%s" % (k, _tag(B, H, W), " ties" if ties else "")
    on_, rn, wd, ad = _nhwc(o), _nhwc(r), _d(w), _d(a)
    # forward: a 2 * k * k-term fp32 dot product into a sigmoid, then one multiply-add per element -- a short fixed-length
    # sum per output, the pointwise class (estimated error: 2e-7 on s, 6e-7 on u at |o| <= 5)
    got_out, got_u, got_s, got_comp = ops.spa1(on_, rn, wd, k, ad, save=True, want_comp=True)
    _pw("spa1 out " + tag, _nchw(got_out), out)
    _pw("spa1 u " + tag, _nchw(got_u), u)
    _pw("spa1 s " + tag, got_s, s[:, 0])
    _pw("spa1 comp " + tag, _nchw(got_comp), comp)
    assert torch.equal(ops.spa1(on_, rn, wd, k, ad), got_out)
    three = ops.spa1(on_, rn, wd, k, ad, save=True)
    assert len(three) == 3 and torch.equal(three[1], got_u) and torch.equal(three[2], got_s)
    # backward on the float64 forward's own u and s (rounded to fp32), so that it alone is under test
    un, sn = _nhwc(u), s.detach().float()[:, 0].contiguous().to(_dev())
    d_o, d_r, dpre = ops.spa1_bwd(_nhwc(dout), un, on_, sn, wd, k, ad, want_dpre=True)
    _rev("spa1_bwd d_o " + tag, _nchw(d_o), ol.grad)
    _rev("spa1_bwd d_r " + tag, _nchw(d_r), rl.grad)
    _rev("spa1_bwd dpre " + tag, dpre, pre.grad[:, 0])
    two = ops.spa1_bwd(_nhwc(dout), un, on_, sn, wd, k, ad)
    assert len(two) == 2 and torch.equal(two[0], d_o) and torch.equal(two[1], d_r)


@pytest.mark.parametrize("k,B,H,W", [(3,) + s for s in SHAPES32] + [(5, 2, 37, 53), (7, 2, 37, 53), (7, 1, 5, 3)])
def test_spa1_and_spa1_bwd(k, B, H, W):
    """SPAattention's tail, out = PReLU(o * s + r), s = sigmoid(conv_k(max_c o, mean_c o)) (oracle.spatial_basic_block)."""
    _spa1_case(k, B, H, W, False)


def test_spa1_bwd_routes_a_tied_maximum_to_the_lowest_channel():
    _spa1_case(3, 2, 37, 53, True)


# ---------------------------------------------------------------------------------------------
# tail and stem
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", SHAPES64)
def test_tail_bwd(B, H, W):
    """fused = tanh(PReLU(z)), z = conv3x3 16 -> 1 (core/model_fusion_auto.py:616-620).  The kernel reads the forward's saved
    fused and z, so the reference is built from those same tensors: autograd of tanh(PReLU(.)) at the saved z, then autograd
    of the conv.  (A float64 z would differ in sign from the saved fp32 one at a few |z| ~ 1e-7 pixels.)"""
    g = _gen(B, H, W)
    t16 = _randn(g, B, 16, H, W)
    w = _randn(g, 1, 16, 3, 3) * 0.15
    a = torch.tensor([0.3])
    dfused = _randn(g, B, 1, H, W)
    fused, z = ops.tail(_nhwc(t16), _d(w), _d(a), save=True)
    tl = _leaf(t16)
    z64 = F.conv2d(tl, w.double(), None, 1, 1)
    tag = _tag(B, H, W)
    _rev("tail z " + tag, z.cpu(), z64)
    zl = _leaf(z.cpu())
    f64 = torch.tanh(F.prelu(zl, a.double()))
    _pw("tail fused " + tag, fused.cpu(), f64)
    (f64 * dfused.double()).sum().backward()
    (z64 * zl.grad).sum().backward()
    got = ops.tail_bwd(_d(dfused), fused, z, _d(w), _d(a))
    _rev("tail_bwd " + tag, _nchw(got), tl.grad)


@pytest.mark.parametrize("B,H,W", SHAPES32)
def test_stem_bwd(B, H, W):
    """feat = PReLU(conv3x3 1 -> 32 (img)) (core/model_fusion_auto.py:604-609).  The kernel takes PReLU' from the sign of the
    forward's saved feat (a positive slope keeps the sign), so does the reference: autograd of PReLU at the saved map,
    then autograd of the conv."""
    g = _gen(B, H, W)
    img = _rand(g, B, 1, H, W)
    w = _randn(g, 32, 1, 3, 3) * 0.4
    a = torch.tensor([0.2])
    dfeat = _randn(g, B, 32, H, W)
    feat, guide = ops.stem(_d(img), _d(w), _d(a))
    il = _leaf(img)
    pre = F.conv2d(il, w.double(), None, 1, 1)
    tag = _tag(B, H, W)
    _rev("stem feat " + tag, _nchw(feat), F.prelu(pre, a.double()))
    fl = _leaf(_nchw(feat))
    (F.prelu(fl, a.double()) * dfeat.double()).sum().backward()       # = dfeat * PReLU'(pre): sign(feat) = sign(pre)
    (pre * fl.grad).sum().backward()
    got = ops.stem_bwd(_nhwc(dfeat), feat, _d(w), _d(a))
    _rev("stem_bwd " + tag, got.cpu(), il.grad)


# ---------------------------------------------------------------------------------------------
# fusion -> segmentation glue
# ---------------------------------------------------------------------------------------------
NEAR = 1e-5        # the clamp is decided in fp32 on the device and in float64 here: elements this close to 0 or 1 are not compared


def _glue_inputs(regime, B, H, W):
    """(fused, ycc) whose recomposed RGB (a) stays inside (0, 1) with ONE smallest and ONE largest element, or (b) is clamped
    at both ends for a large share of the elements, so that mn = 0, mx = 1 and thousands of elements tie, or (t) is as (a) but
    with THREE unclamped elements sharing the minimum and TWO the maximum: the only case in which the even split of the
    min / max gradient over the tied elements reaches an output (in (b) every tied element is clamped and passes nothing)."""
    g = _gen(ord(regime), B, H, W)
    if regime in "at":
        fused = 0.3 + 0.4 * _rand(g, B, 1, H, W)
        ycc = torch.cat((_rand(g, B, 1, H, W), 0.45 + 0.1 * _rand(g, B, 2, H, W)), 1)
        # the extrema: G = 0.1 - 0.714 * 0.02 = 0.0857 at pixel (0, 0), R = 0.9 + 1.403 * 0.02 = 0.928 at the last pixel;
        # everything else lies in [0.2, 0.8]
        fused[0, 0, 0, 0], fused[-1, 0, -1, -1] = 0.1, 0.9
        ycc[0, 1, 0, 0], ycc[-1, 1, -1, -1] = 0.52, 0.52
        ycc[0, 2, 0, 0], ycc[-1, 2, -1, -1] = 0.5, 0.5
        if regime == "t":      # the same (fused, Cr, Cb) triple at more pixels: the same fp32 and the same float64 G resp. R
            fused[0, 0, 0, 1:3], fused[-1, 0, -1, -2] = 0.1, 0.9
            ycc[0, 1, 0, 1:3], ycc[-1, 1, -1, -2] = 0.52, 0.52
            ycc[0, 2, 0, 1:3], ycc[-1, 2, -1, -2] = 0.5, 0.5
    else:
        fused = -0.4 + 1.8 * _rand(g, B, 1, H, W)
        ycc = torch.cat((_rand(g, B, 1, H, W), 0.2 + 0.6 * _rand(g, B, 2, H, W)), 1)
    return fused, ycc


def _recomposed(fused, ycc):
    return O.ycrcb2rgb(torch.cat((fused, ycc[:, 1:2], ycc[:, 2:]), dim=1))


def _check_regime(regime, v, n_min_ties):
    """v: the reference's values in front of the clamp.  Returns the mask of the values that are compared."""
    near = (v.abs() <= NEAR) | ((v - 1).abs() <= NEAR)
    assert float(near.double().mean()) <= 1e-3, float(near.double().mean())
    c = v.clamp(0, 1).flatten().sort()[0]
    if regime in "at":
        nmin, nmax = (1, 1) if regime == "a" else (3, 2)
        assert bool(((v > 0) & (v < 1)).all())
        assert int((c == c[0]).sum()) == nmin and int((c == c[-1]).sum()) == nmax
        assert float(c[nmin] - c[0]) > NEAR and float(c[-1] - c[-1 - nmax]) > NEAR
    else:
        assert float(c[0]) == 0.0 and float(c[-1]) == 1.0
        if n_min_ties:
            assert int((c == 0).sum()) >= n_min_ties and int((c == 1).sum()) >= n_min_ties
        assert float(((v < 0) | (v > 1)).double().mean()) > 0.15
    return ~near


@pytest.mark.parametrize("B,H,W", SHAPES256)
@pytest.mark.parametrize("regime", ["a", "b", "t"])
def test_glue_bwd(regime, B, H, W):
    """d seg_in -> (d fused, d Cr/Cb) against autograd of oracle.seg_input_from_fused, with and without dfused_direct.
    torch's semantics: the clamp passes gradient only inside [0, 1]; min / max spread theirs evenly over the tied extrema.
    In regimes (a) and (t) the few extremal pixels carry a whole-batch sum (about 1e3 against 5 for an ordinary pixel at the
    largest shape) and so set max|ref|: the ordinary pixels are compared a second time on their own scale."""
    fused, ycc = _glue_inputs(regime, B, H, W)
    g = _gen(7, B, H, W)
    dseg, direct = _randn(g, B, 3, H, W), _randn(g, B, 1, H, W)
    fl, yl = _leaf(fused), _leaf(ycc)
    keep3 = _check_regime(regime, _recomposed(fl.detach(), yl.detach()), 1000 if B * H * W > 3000 else 0)
    keep = keep3.all(dim=1, keepdim=True)          # a pixel is compared when all three of its channels are
    assert float((~keep).double().mean()) <= 1e-3
    ref = O.seg_input_from_fused(fl, yl)
    (ref * dseg.double()).sum().backward()
    v = _recomposed(fl.detach(), yl.detach())
    ordinary = keep & ~((v == v.min()) | (v == v.max())).any(dim=1, keepdim=True)
    fd, yd = _d(fused), _d(ycc)
    seg_in, mm = ops.seg_input_from_fused(fd, yd, return_minmax=True)
    tag = "%s %s" % (regime, _tag(B, H, W))
    _pw("seg_input_from_fused " + tag, seg_in.cpu(), ref)
    for has_direct in (False, True):
        dfused, dcrcb = ops.glue_bwd(_d(dseg), fd, yd, mm, _d(direct) if has_direct else None)
        _rev("glue_bwd dfused direct%d %s" % (has_direct, tag), dfused.cpu(), fl.grad + (direct.double() if has_direct else 0.0), keep)
        _rev("glue_bwd dcrcb direct%d %s" % (has_direct, tag), dcrcb.cpu(), yl.grad[:, 1:3], keep.expand(-1, 2, -1, -1))
        if regime in "at":
            _rev("glue_bwd dfused ordinary %s" % tag, dfused.cpu(), fl.grad + (direct.double() if has_direct else 0.0), ordinary,
                 scale_over_keep=True)
            _rev("glue_bwd dcrcb ordinary %s" % tag, dcrcb.cpu(), yl.grad[:, 1:3], ordinary.expand(-1, 2, -1, -1), scale_over_keep=True)
    assert float(yl.grad[:, 0].abs().max()) == 0.0      # the Y plane of the visible image does not reach seg_in


@pytest.mark.parametrize("B,H,W", SHAPES256)
@pytest.mark.parametrize("regime", ["a", "b", "t"])
def test_plane_clamp_minmax_and_bwd(regime, B, H, W):
    """forward_object's extra step (core/model_fusion_auto.py:743-751): clamp to [0, 1] by two torch.where, batch-global min-max.
    Regimes as in _glue_inputs; in (t) three elements are 0.1 and two are 0.9."""
    g = _gen(ord(regime), 3, B, H, W)
    if regime in "at":
        x = 0.2 + 0.6 * _rand(g, B, 1, H, W)
        x[0, 0, 0, 0], x[-1, 0, -1, -1] = 0.1, 0.9
        if regime == "t":
            x[0, 0, 0, 1:3], x[-1, 0, -1, -2] = 0.1, 0.9
    else:
        x = -0.5 + 2.0 * _rand(g, B, 1, H, W)
    dout = _randn(g, B, 1, H, W)
    xl = _leaf(x)
    keep = _check_regime(regime, xl.detach(), 1000 if B * H * W > 5000 else 0)
    c = torch.where(xl > 1, torch.ones_like(xl), xl)
    c = torch.where(c < 0, torch.zeros_like(c), c)
    ref = (c - torch.min(c)) / (torch.max(c) - torch.min(c))
    (ref * dout.double()).sum().backward()
    out, mm = ops.plane_clamp_minmax(_d(x))
    tag = "%s %s" % (regime, _tag(B, H, W))
    assert mm.cpu().double().tolist() == [float(c.detach().min()), float(c.detach().max())]
    _pw("plane_clamp_minmax " + tag, out.cpu(), ref)
    dx = ops.plane_clamp_minmax_bwd(_d(dout), _d(x), mm)
    _rev("plane_clamp_minmax_bwd " + tag, dx.cpu(), xl.grad, keep)
    if regime in "at":
        ordinary = keep & (xl.detach() != xl.detach().min()) & (xl.detach() != xl.detach().max())
        _rev("plane_clamp_minmax_bwd ordinary " + tag, dx.cpu(), xl.grad, ordinary, scale_over_keep=True)


@pytest.mark.parametrize("B,H,W", SHAPES256)
def test_rgb2ycrcb_bwd_and_recompose_clamp(B, H, W):
    g = _gen(B, H, W)
    vis = _rand(g, B, 3, H, W)
    dY, dcrcb = _randn(g, B, 1, H, W), _randn(g, B, 2, H, W)
    vl = _leaf(vis)
    ycc = O.rgb2ycrcb(vl)
    ((ycc[:, 0:1] * dY.double()).sum() + (ycc[:, 1:3] * dcrcb.double()).sum()).backward()
    tag = _tag(B, H, W)
    _pw("rgb2ycrcb_bwd " + tag, ops.rgb2ycrcb_bwd(_d(dY), _d(dcrcb)).cpu(), vl.grad)
    fused, ycc_b = _glue_inputs("b", B, H, W)
    ref = _recomposed(fused.double(), ycc_b.double()).clamp(0, 1)
    rgb, partial = ops.recompose_clamp(_d(fused), _d(ycc_b))
    _pw("recompose_clamp " + tag, rgb.cpu(), ref)
    nblk = (B * H * W + 2047) // 2048
    assert partial.numel() == 2 * nblk
    assert float(partial[:nblk].min()) == float(rgb.min()) and float(partial[nblk:].max()) == float(rgb.max())
    fa, ya = _glue_inputs("a", B, H, W)
    rgb, partial = ops.recompose_clamp(_d(fa), _d(ya))
    ref = _recomposed(fa.double(), ya.double())
    _pw("recompose_clamp (no clamp) " + tag, rgb.cpu(), ref)
    _pw("recompose_clamp min " + tag, partial[:nblk].min().cpu(), ref.min())
    _pw("recompose_clamp max " + tag, partial[nblk:].max().cpu(), ref.max())


# ---------------------------------------------------------------------------------------------
# fusion loss: L1 + SSIM
# ---------------------------------------------------------------------------------------------
# one workgroup per 16 x 16 tile (no grid-stride loop): smaller than the 11-tap window, exactly one tile, ragged in both
# directions (37 = 2 * 16 + 5, 53 = 3 * 16 + 5; 19 = 16 + 3, 150 = 9 * 16 + 6), and the sizes of the other tests
SHAPES_SSIM = [(1, 5, 3), (2, 8, 9), (2, 16, 16), (1, 11, 11), (2, 37, 53), (3, 19, 150), (2, 150, 203)]


def _ssim_inputs(B, H, W):
    """x in [0.1, 0.9]; |y - x| in [0.02, 0.22]: the sign term of the L1 part has no gradient at y = x."""
    g = _gen(B, H, W)
    x = 0.1 + 0.8 * _rand(g, B, 1, H, W)
    d = (0.02 + 0.2 * _rand(g, B, 1, H, W)) * torch.where(_rand(g, B, 1, H, W) < 0.5, -1.0, 1.0)
    y = x + d
    assert float((y - x).abs().min()) >= 0.019
    return x, y


@pytest.mark.parametrize("B,H,W", SHAPES_SSIM)
def test_ssim_l1(B, H, W):
    """(mean SSIM, mean |y - x|) against oracle.ssim in float64.  Held to the pointwise bound: a pixel's SSIM is a ratio of
    121-term fp32 sums whose largest cancellation, E[x^2] - mu^2 ~ 0.05 of 0.3 on these inputs, costs under 1e-6 relative,
    and the mean over the pixels (formed in double by the finishing kernel) only averages that down."""
    x, y = _ssim_inputs(B, H, W)
    s, l1 = ops.ssim_l1(_d(x), _d(y))
    _pw("ssim_l1 ssim " + _tag(B, H, W), s.cpu(), O.ssim(x.double(), y.double()))
    _pw("ssim_l1 l1 " + _tag(B, H, W), l1.cpu(), (y.double() - x.double()).abs().mean())


@pytest.mark.parametrize("B,H,W", SHAPES_SSIM)
def test_ssim_l1_bwd(B, H, W):
    """dx per pixel against autograd of k_l1 * sum|y - x| + k_ss * sum(1 - S), S = the SSIM map of oracle.ssim (its mean
    times the pixel count is the sum) -- core/loss.py:490-502."""
    x, y = _ssim_inputs(B, H, W)
    k_l1, k_ss = 0.37, 1.1
    xl = _leaf(x)
    n = x.numel()
    (k_l1 * (y.double() - xl).abs().sum() + k_ss * n * (1 - O.ssim(xl, y.double()))).backward()
    dev = _dev()
    dx = ops.ssim_l1_bwd(_d(x), _d(y), torch.tensor(k_l1, device=dev), torch.tensor(k_ss, device=dev))
    _rev("ssim_l1_bwd " + _tag(B, H, W), dx.cpu(), xl.grad)
