"""Direct float64 tests of the forward fusion kernels (csrc/fusion_kernels.hip, and channel_sum_chunks of
csrc/object_glue.hip behind eca_layer_fwd) in all three storages: fp32, bf16 and IEEE fp16 maps.

Every case calls one `ops.*` wrapper and compares it with a float64 restatement of the operator on the CPU in plain torch
(F.conv2d, amax, mean, sigmoid, tanh), so a failure names one kernel.  No other kernel of the project serves as the
reference.  The inputs are seeded, signed (randn) float32 values; a 16-bit input is first made representable (cast_storage
down and up) and the float64 reference takes those same values.  Weights are scaled so that the outputs are O(1).

Bounds, the ones the suite already holds these classes of kernel to (tests/kernel_check.py):
  stencil kernels in fp32 (stem, dwconv, spa_blend, tail, eca_layer_fwd)   max|err| <= REV * max|ref| = 2e-5 * max|ref|
  pointwise kernels (channel_pool mean, eca_finish, colour)                max|err| <= PW * max(1, max|ref|), PW = 2e-6
  single-rounding outputs (max, max - min, fp32 add) and data movement     bit equality
  16-bit outputs, per element      |got - ref| <= 1.01 * eps16 * |ref| + the fp32 bound of the same kernel at that case,
                                   eps16 = 2^-8 (bf16), 2^-11 (fp16): tests/test_bf16_storage_gpu.py, test_f16_storage_gpu.py
  fp32 outputs from 16-bit inputs (channel_pool, tail)                     the fp32 bound, unchanged.

Shapes.  The per-pixel kernels cap their grid at MAXGRID = 2048 blocks and grid-stride:
  32 pixels per block (dwconv, channel_pool, channel_residue, spa_blend, eca_apply): one sweep = 65,536 pixels;
     3 * 150 * 203 = 91,350 runs a second sweep of 25,814 = 806 * 32 + 22 pixels, which ends in a partial block;
  64 pixels per block (tail): one sweep = 131,072 pixels; 2 * 260 * 301 = 156,520 leaves 25,448 = 397 * 64 + 40;
  256 pixels per block (rgb2ycrcb, ycrcb2rgb: grid_for(B * H * W, 256), 256 threads): one sweep = 524,288 pixels; the case
     beyond it is (2, 520, 601) = 625,040 pixels, whose second sweep takes 100,752 = 393 * 256 + 144 pixels;
  256 float4 per block (add): one sweep = 2,097,152 floats; 2,098,355 leaves 300 float4 and a 3-element tail.
stem walks (row, 128-pixel chunk) items on a grid capped at 4096 with two LDS patch buffers: (1, 8300, 3) has 8300 items,
so blocks take a third item and reuse a buffer.  The 16-bit spa_blend walks 4 x 64 tiles on a grid capped at 4096:
(1, 16400, 1) has 4100 tiles and (1, 33000, 3) 8250, so the tile loop runs a second and a third time.  The 16-bit 3 x 3
dwconv takes 24-row strips of 64-column tiles: (2, 24, 64) fits exactly, (1, 25, 65) hangs over by one pixel each way,
(1, 23, 63) falls short by one, (2, 49, 130) has three strips and three column tiles, (1, 1, 1) and (1, 2, 3) have H <= DIL.
eca_scale sums `tiles_per_img` partials in 32 strided parts: 1, 32, 33 and 133 tiles.  Every check prints its ERR line."""
import functools

import pytest
import torch
import torch.nn.functional as F

from paif_amd import ops
from tests.kernel_check import PW, REV, dev as _dev, err as _err, exact as _exact, gen, h16 as _h16, pw as _pw, rev as _rev, to_dev as _d

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
STORAGES = [F32, BF16, F16]
EPS16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
NAME = {F32: "f32", BF16: "bf16", F16: "f16"}
_ids = NAME.get

SHAPES32 = [(1, 1, 1), (1, 2, 3), (2, 37, 53), (3, 19, 150)]
SWEEP32 = (3, 150, 203)
POOL_SHAPES = [(1, 1, 1), (2, 37, 53), SWEEP32]


def _gen(*key):
    return gen(*key, base=43)


@pytest.fixture(autouse=True)
def _default_arithmetic():
    old = dict(ops.CONFIG)
    ops.set_conv_precision("bf16x3")
    ops.set_storage("f32")
    yield
    ops.CONFIG.update(old)
    ops._ACT_BF16[0] = False
    ops._TWINS.clear()


def _tag(B, H, W, dt=F32, *more):
    return " ".join(["%dx%dx%d" % (B, H, W), NAME[dt]] + [str(m) for m in more])


def _store(x, dt):
    """CPU fp32 map -> (the map on the device in storage dt, the values it holds there as a CPU fp32 tensor)."""
    xd = _d(x)
    if dt is F32:
        return xd, x
    x16 = ops.cast_storage(xd, dt)
    assert x16.dtype == dt
    return x16, ops.cast_storage(x16, F32).cpu()


def _nchw64(x):
    """CPU NHWC -> NCHW float64."""
    return x.double().permute(0, 3, 1, 2)


def _nhwc(y):
    return y.permute(0, 2, 3, 1)


def _scale(ref, rel=REV):
    return rel * float(ref.abs().max())


def _pw_bound(ref):
    return PW * max(1.0, float(ref.abs().max()))


def _check(name, got, ref, dt, bound32):
    """fp32 output: the fp32 bound; 16-bit output: its rounding on top."""
    if got.dtype == F32:
        _err(name, got, ref, bound32)
    else:
        assert got.dtype == dt
        _h16(name, got, ref, EPS16[dt], bound32)


# ---------------------------------------------------------------------------------------------
# stem: conv3x3 1 -> 32 + PReLU
# ---------------------------------------------------------------------------------------------
STEM_CASES = [(1, 1, 1, 0), (1, 5, 3, 0), (2, 37, 53, 0), (1, 3, 128, 0), (1, 3, 129, 0), (2, 9, 257, 0), (1, 8300, 3, 0),
              (2, 37, 53, 1)]      # the last: the image is channel 0 of a [B,3,H,W] tensor (batch stride 3 * H * W)


@functools.lru_cache(maxsize=None)
def _stem_case(B, H, W, strided):
    g = _gen(B, H, W, strided)
    src = torch.randn(B, 3 if strided else 1, H, W, generator=g)
    w = torch.randn(32, 1, 3, 3, generator=g) * 0.3
    a = torch.tensor([0.2])
    pre = F.conv2d(src[:, 0:1].double(), w.double(), None, 1, 1)
    # PReLU is the only non-linearity: both of its branches are taken, and the values are O(1) (share of |pre| < 1)
    assert float((pre.abs() < 1).double().mean()) > 0.5 and bool((pre < 0).any()) and bool((pre > 0).any())
    return src, w, a, _nhwc(F.prelu(pre, a.double())).contiguous()


@pytest.mark.parametrize("mode", ["f32", "bf16", "f16", "f16_only"])
@pytest.mark.parametrize("B,H,W,strided", STEM_CASES)
def test_stem(B, H, W, strided, mode, monkeypatch):
    """feat = PReLU(conv3x3 1 -> 32 (img)) (core/model_fusion_auto.py:604-609), want_guide=False.  fp32 storage: the fp32
    map.  bf16 / fp16 storage: the fp32 map and the 16-bit twin the same kernel writes, which must also be the RNE cast of
    the fp32 map (a single rounding); fp16 with CONFIG["gf_in_f16"]: the fp16 map alone."""
    src, w, a, ref = _stem_case(B, H, W, strided)
    srcd = src.to(_dev())
    img = srcd[:, 0:1]
    assert img.is_contiguous() == (not strided)
    tag = _tag(B, H, W, F32, mode, "strided" if strided else "dense")
    b32 = _scale(ref)
    if mode == "f32":
        feat, guide = ops.stem(img, _d(w), _d(a), want_guide=False)
        assert guide is None and feat.dtype == F32
        _err("stem feat " + tag, feat, ref, b32)
        return
    dt = BF16 if mode == "bf16" else F16
    monkeypatch.setitem(ops.CONFIG, "gf_in_f16", mode == "f16_only")
    ops.set_storage("bf16" if dt is BF16 else "f16")
    with ops.bf16_activations():
        feat, guide = ops.stem(img, _d(w), _d(a), want_guide=False)
        twin = ops.cast_storage(feat, dt)
        if mode == "f16_only":
            assert twin is feat
        else:
            assert ops._TWINS[feat.data_ptr()][1] is twin       # written by the stem kernel, not by a cast pass
    assert guide is None and twin.dtype == dt
    if mode != "f16_only":
        _err("stem feat " + tag, feat, ref, b32)
        _exact("stem twin = cast(feat) " + tag, twin, feat.cpu().to(dt))
    _h16("stem twin " + tag, twin, ref, EPS16[dt], b32)


# ---------------------------------------------------------------------------------------------
# depthwise k x k
# ---------------------------------------------------------------------------------------------
def _dwconv_case(B, H, W, k, dil, in_relu, dt):
    g = _gen(B, H, W, k, dil)
    x = torch.randn(B, H, W, 32, generator=g)
    w = torch.randn(32, 1, k, k, generator=g) / k
    xd, xv = _store(x, dt)
    x64 = _nchw64(xv)
    ref = _nhwc(F.conv2d(F.relu(x64) if in_relu else x64, w.double(), None, 1, dil * (k - 1) // 2, dil, 32))
    got = ops.dwconv(xd, _d(w), k, dil, in_relu)
    assert got.dtype == dt
    _check("dwconv k%d d%d relu%d %s" % (k, dil, in_relu, _tag(B, H, W, dt)), got, ref, dt, _scale(ref))


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 2), (5, 1), (5, 2), (7, 1), (7, 2)])
@pytest.mark.parametrize("B,H,W", SHAPES32)
def test_dwconv_f32(B, H, W, k, dil, in_relu):
    """Depthwise conv (groups = 32), zero padding dil * (k - 1) / 2, optional ReLU on the input (operations_m.py DilConv /
    SepConv); signed input, so in_relu changes the result; (1,1,1) and (1,2,3) are smaller than every stencil."""
    _dwconv_case(B, H, W, k, dil, in_relu, F32)


@pytest.mark.parametrize("k,dil,in_relu", [(3, 2, True), (5, 1, False), (7, 2, True)])
def test_dwconv_f32_second_sweep(k, dil, in_relu):
    _dwconv_case(*SWEEP32, k, dil, in_relu, F32)


# 24-row strips, 64-column tiles (dwconv3_bf16_kernel); (2,37,53): the shape the 16-bit kernels had before
DW16_SHAPES = [(1, 1, 1), (1, 2, 3), (2, 24, 64), (1, 25, 65), (2, 49, 130), (1, 23, 63), (2, 37, 53)]


@pytest.mark.parametrize("in_relu", [False, True])
@pytest.mark.parametrize("k,dil", [(3, 1), (3, 2), (5, 1)])
@pytest.mark.parametrize("B,H,W", DW16_SHAPES)
@pytest.mark.parametrize("dt", [BF16, F16], ids=_ids)
def test_dwconv_16bit(dt, B, H, W, k, dil, in_relu):
    """The 3x3 forms run the strip kernel (a register window of 2 * dil + 1 rows, loaded two rows ahead), 5x5 the per-pixel
    kernel on 16-bit loads."""
    _dwconv_case(B, H, W, k, dil, in_relu, dt)


def test_dwconv_refuses_sizes_that_are_not_built():
    """16-bit (5,2) and (7,1), fp32 (9,1): the library's error, and the outputs of earlier calls stay as they were."""
    g = _gen(9)
    x = torch.randn(2, 9, 11, 32, generator=g)
    w = {k: _d(torch.randn(32, 1, k, k, generator=g) / k) for k in (3, 5, 7, 9)}
    maps = {dt: _store(x, dt)[0] for dt in STORAGES}
    good = {dt: ops.dwconv(maps[dt], w[3], 3, 1, False) for dt in STORAGES}
    torch.cuda.synchronize()
    keep = {dt: good[dt].cpu().clone() for dt in STORAGES}
    for dt, k, dil in [(BF16, 5, 2), (F16, 5, 2), (BF16, 7, 1), (F16, 7, 1), (F32, 9, 1)]:
        with pytest.raises(RuntimeError, match="kernel %d dil %d not built" % (k, dil)):
            ops.dwconv(maps[dt], w[k], k, dil, False)
    torch.cuda.synchronize()
    for dt in STORAGES:
        _exact("dwconv output after the refusals " + NAME[dt], good[dt], keep[dt])
    _dwconv_case(2, 9, 11, 3, 1, False, F32)      # and the library goes on working


# ---------------------------------------------------------------------------------------------
# ChannelPool, residue
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", POOL_SHAPES)
@pytest.mark.parametrize("dt", STORAGES, ids=_ids)
def test_channel_pool2(dt, B, H, W):
    """(max_c ir, mean_c ir, max_c vis, mean_c vis) per pixel (operations_m.py ChannelPool): fp32 output in every storage."""
    g = _gen(B, H, W)
    (ad, av), (bd, bv) = [_store(torch.randn(B, H, W, 32, generator=g), dt) for _ in range(2)]
    comp = ops.channel_pool2(ad, bd)
    assert comp.dtype == F32 and tuple(comp.shape) == (B, H, W, 4)
    tag = _tag(B, H, W, dt)
    for name, v, c in (("ir", av, 0), ("vis", bv, 2)):
        _exact("channel_pool2 max %s %s" % (name, tag), comp[..., c], v.amax(-1))
        _pw("channel_pool2 mean %s %s" % (name, tag), comp[..., c + 1], v.double().mean(-1))


@pytest.mark.parametrize("coff", [0, 2])
@pytest.mark.parametrize("B,H,W", POOL_SHAPES)
@pytest.mark.parametrize("dt", STORAGES, ids=_ids)
def test_channel_pool1(dt, B, H, W, coff):
    """ChannelPool of one map into its half of the interleaved plane; the other half keeps every bit."""
    g = _gen(B, H, W, coff)
    xd, xv = _store(torch.randn(B, H, W, 32, generator=g), dt)
    before = torch.randn(B, H, W, 4, generator=g)
    comp = _d(before)
    assert ops.channel_pool1(xd, comp, coff) is comp
    tag = _tag(B, H, W, dt, "coff%d" % coff)
    _exact("channel_pool1 max " + tag, comp[..., coff], xv.amax(-1))
    _pw("channel_pool1 mean " + tag, comp[..., coff + 1], xv.double().mean(-1))
    _exact("channel_pool1 other half " + tag, comp[..., 2 - coff:4 - coff], before[..., 2 - coff:4 - coff])


@pytest.mark.parametrize("B,H,W", POOL_SHAPES)
def test_channel_residue(B, H, W):
    """max_c - min_c (Cell_Decom.get_residue): max and min are exact, their fp32 difference is one rounding."""
    x = torch.randn(B, H, W, 32, generator=_gen(B, H, W))
    _exact("channel_residue " + _tag(B, H, W), ops.channel_residue(_d(x)), x.amax(-1) - x.amin(-1))


# ---------------------------------------------------------------------------------------------
# spatial attention blend
# ---------------------------------------------------------------------------------------------
def _spa_case(B, H, W, dt):
    """comp is the test's own random plane, not a ChannelPool of ir and vis: the 100 weights of the 5x5 4 -> 1 conv all count."""
    g = _gen(B, H, W)
    comp = torch.randn(B, H, W, 4, generator=g)
    w = torch.randn(1, 4, 5, 5, generator=g) * 0.1
    (ird, irv), (visd, visv) = [_store(torch.randn(B, H, W, 32, generator=g), dt) for _ in range(2)]
    pre = _nhwc(F.conv2d(_nchw64(comp), w.double(), None, 1, 2))
    assert float((pre.abs() < 2).double().mean()) > 0.5      # the sigmoid is not saturated
    s = torch.sigmoid(pre)
    return _d(comp), _d(w), ird, visd, s[..., 0], s * irv.double() + (1 - s) * visv.double()


@pytest.mark.parametrize("B,H,W", SHAPES32 + [SWEEP32])
def test_spa_blend_f32(B, H, W):
    """scale = sigmoid(conv5x5 4 -> 1 (comp)), agg = scale * ir + (1 - scale) * vis (operations_m.py spatial attention)."""
    comp, w, ir, vis, s, ref = _spa_case(B, H, W, F32)
    tag = _tag(B, H, W)
    _err("spa_blend agg " + tag, ops.spa_blend(comp, w, ir, vis), ref, _scale(ref))
    agg, scale = ops.spa_blend(comp, w, ir, vis, want_scale=True)
    _err("spa_blend agg (want_scale) " + tag, agg, ref, _scale(ref))
    _err("spa_blend scale " + tag, scale, s, _scale(s))


@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 4, 64), (1, 5, 65), (3, 4, 64), (2, 37, 130), (1, 16400, 1), (1, 33000, 3)])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_ids)
def test_spa_blend_16bit_tiled(dt, B, H, W, monkeypatch):
    """4 x 64 tiles through LDS, grid capped at 4096: the last two shapes make a block take a second and a third tile."""
    monkeypatch.setenv("PAIF_SPA_TILED", "1")
    comp, w, ir, vis, _, ref = _spa_case(B, H, W, dt)
    _check("spa_blend tiled " + _tag(B, H, W, dt), ops.spa_blend(comp, w, ir, vis), ref, dt, _scale(ref))


@pytest.mark.parametrize("B,H,W", [(1, 2, 3), (2, 37, 130)])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_ids)
def test_spa_blend_16bit_untiled(dt, B, H, W, monkeypatch):
    """PAIF_SPA_TILED=0: the pixel-per-8-lanes kernel on 16-bit maps."""
    monkeypatch.setenv("PAIF_SPA_TILED", "0")
    comp, w, ir, vis, _, ref = _spa_case(B, H, W, dt)
    _check("spa_blend untiled " + _tag(B, H, W, dt), ops.spa_blend(comp, w, ir, vis), ref, dt, _scale(ref))


# ---------------------------------------------------------------------------------------------
# ECA: gate from the per-tile partial sums, then out = PReLU(o * gate + r)
# ---------------------------------------------------------------------------------------------
def _gate(mean, w1d, k):
    """sigmoid(conv1d_k over the channels, zero padded) of per-image channel means [B,32] (float64)."""
    return torch.sigmoid(F.conv1d(mean.unsqueeze(1), w1d.double().view(1, 1, k), None, 1, (k - 1) // 2).squeeze(1))


@pytest.mark.parametrize("k", [1, 3, 5, 7, 9])
@pytest.mark.parametrize("B,H,W,tiles", [(3, 5, 3, 1), (2, 64, 128, 32), (2, 88, 96, 33), (2, 150, 203, 133)])
@pytest.mark.parametrize("dt", STORAGES, ids=_ids)
def test_eca_finish(dt, B, H, W, tiles, k):
    """The partial sums are random and unrelated to o (the kernel only reduces them), scaled so that the channel means are
    O(1) and the gate is not saturated; o and r are signed and the slope is 0.25, so both PReLU branches are taken."""
    assert ops.lib().paif_conv2d_blocks(1, H, W) == tiles
    g = _gen(B, H, W, k)
    partial = torch.randn(B, tiles, 32, generator=g) * (H * W / tiles ** 0.5)
    w1d = torch.randn(k, generator=g) / k ** 0.5
    a = torch.tensor([0.25])
    (od, ov), (rd, rv) = [_store(torch.randn(B, H, W, 32, generator=g), dt) for _ in range(2)]
    gate = _gate(partial.double().sum(1) / (H * W), w1d, k)
    assert float(((gate > 0.1) & (gate < 0.9)).double().mean()) > 0.5
    u = ov.double() * gate[:, None, None, :] + rv.double()
    ref = torch.where(u >= 0, u, 0.25 * u)
    tag = _tag(B, H, W, dt, "k%d" % k)
    if dt is F32:
        out, ud, gd = ops.eca_finish(od, rd, _d(partial), _d(w1d), k, _d(a), save=True)
        _pw("eca_finish gate " + tag, gd, gate)
        _pw("eca_finish u " + tag, ud, u)
        _pw("eca_finish out " + tag, out, ref)
    _check("eca_finish out (no save) " + tag, ops.eca_finish(od, rd, _d(partial), _d(w1d), k, _d(a)), ref, dt, _pw_bound(ref))


@pytest.mark.parametrize("k", [3, 5])
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (2, 37, 53), (2, 150, 203)])
def test_eca_layer_fwd(B, H, W, k):
    """x * sigmoid(conv1d_k(mean_hw x)) (operations_m.py:353-367): channel_sum_chunks, eca_scale, eca_apply.  Each channel
    carries an offset of its own, so the means are O(1) and differ between the channels the conv1d mixes."""
    g = _gen(B, H, W, k)
    x = torch.randn(B, H, W, 32, generator=g) + torch.randn(B, 1, 1, 32, generator=g) * 1.5
    w1d = torch.randn(k, generator=g) / k ** 0.5
    gate = _gate(x.double().mean((1, 2)), w1d, k)
    ref = x.double() * gate[:, None, None, :]
    _rev("eca_layer_fwd %s k%d" % (_tag(B, H, W), k), ops.eca_layer_fwd(_d(x), _d(w1d), k), ref)


# ---------------------------------------------------------------------------------------------
# tail: conv3x3 16 -> 1, PReLU, tanh
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W", [(1, 1, 1), (1, 5, 3), (2, 37, 53), (3, 19, 150), (2, 260, 301)])
@pytest.mark.parametrize("dt", STORAGES, ids=_ids)
def test_tail(dt, B, H, W):
    """fused = tanh(PReLU(z)), z = conv3x3 16 -> 1 (core/model_fusion_auto.py:616-620); fp32 output in every storage."""
    g = _gen(B, H, W)
    xd, xv = _store(torch.randn(B, H, W, 16, generator=g), dt)
    w = torch.randn(1, 16, 3, 3, generator=g) * 0.08
    a = torch.tensor([0.3])
    z = F.conv2d(_nchw64(xv), w.double(), None, 1, 1)
    assert float((z.abs() < 1).double().mean()) > 0.5          # tanh is not saturated: it would hide an error in z
    ref = torch.tanh(F.prelu(z, a.double()))
    tag = _tag(B, H, W, dt)
    if dt is F32:
        fused, zd = ops.tail(xd, _d(w), _d(a), save=True)
        _err("tail z " + tag, zd, z, _scale(z))
        _err("tail fused (save) " + tag, fused, ref, _scale(ref))
    fused = ops.tail(xd, _d(w), _d(a))
    assert fused.dtype == F32
    _err("tail fused " + tag, fused, ref, _scale(ref))


# ---------------------------------------------------------------------------------------------
# add
# ---------------------------------------------------------------------------------------------
ADD_SWEEP = 2048 * 256 * 4 + 300 * 4


@pytest.mark.parametrize("n", [3, 1036, 1037, 1038, 1039, ADD_SWEEP + 3])
def test_add_f32(n):
    """One rounding per element: bit-equal to torch's fp32 add.  n % 4 = 0, 1, 2, 3 (the tail the first block adds), n < 4,
    and a second sweep with a partial block and a tail."""
    g = _gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    _exact("add f32 n=%d" % n, ops.add(_d(a), _d(b)), a + b)


@pytest.mark.parametrize("mixed", [0, 1, 2])
@pytest.mark.parametrize("shape", [(2, 37, 53, 32), (ADD_SWEEP,)])
@pytest.mark.parametrize("dt", [BF16, F16], ids=_ids)
def test_add_16bit(dt, shape, mixed):
    """16-bit add (fp32 sum of the two stored values, rounded once more on the store); mixed 1 / 2: the first / second operand
    is an fp32 tensor (of representable values), which ops.add casts down first.  The fp32 bound of add is bit equality."""
    g = _gen(len(shape), mixed)
    (ad, av), (bd, bv) = [_store(torch.randn(*shape, generator=g), dt) for _ in range(2)]
    if mixed == 1:
        ad = _d(av)
    if mixed == 2:
        bd = _d(bv)
    got = ops.add(ad, bd)
    assert got.dtype == dt
    _h16("add %s n=%d mixed%d" % (NAME[dt], av.numel(), mixed), got, av.double() + bv.double(), EPS16[dt], 0.0)


# ---------------------------------------------------------------------------------------------
# colour
# ---------------------------------------------------------------------------------------------
COLOUR_SHAPES = [(1, 1, 1), (2, 37, 53), (2, 520, 601)]


@pytest.mark.parametrize("B,H,W", COLOUR_SHAPES)
def test_rgb2ycrcb(B, H, W):
    """Y = 0.299 R + 0.587 G + 0.114 B, Cr = (R - Y) 0.713 + 0.5, Cb = (B - Y) 0.564 + 0.5 (core/model_fusion_auto.py:69-92)."""
    rgb = torch.randn(B, 3, H, W, generator=_gen(B, H, W))
    R, G, Bl = rgb.double().unbind(1)
    Y = 0.299 * R + 0.587 * G + 0.114 * Bl
    ref = torch.stack((Y, (R - Y) * 0.713 + 0.5, (Bl - Y) * 0.564 + 0.5), 1)
    _pw("rgb2ycrcb " + _tag(B, H, W), ops.rgb2ycrcb(_d(rgb)), ref)


@pytest.mark.parametrize("B,H,W", COLOUR_SHAPES)
def test_ycrcb2rgb(B, H, W):
    """(ycc + (0, -0.5, -0.5)) times the matrix of core/model_fusion_auto.py:94-111, no clamp."""
    ycc = torch.randn(B, 3, H, W, generator=_gen(B, H, W))
    Y, cr, cb = ycc.double().unbind(1)
    cr, cb = cr - 0.5, cb - 0.5
    ref = torch.stack((Y + 1.403 * cr, Y - 0.714 * cr - 0.344 * cb, Y + 1.773 * cb), 1)
    _pw("ycrcb2rgb " + _tag(B, H, W), ops.ycrcb2rgb(_d(ycc)), ref)
