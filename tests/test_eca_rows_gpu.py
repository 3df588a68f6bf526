"""GPU tests of the ECA block's tail without the map o (csrc/conv_eca_rows.hip, paif_eca_conv2_gated_fwd_f16): conv2 over PReLU(r) run
twice as a row-streaming LDS-DMA kernel -- once for the per-tile pool partials, once with out = PReLU(fp16(o) * gate + r) in its epilogue.

The reference is the path it replaces, in the same process: ops.conv2d([r], wpk, 3, 1, in_act=PRELU, in_prelu=a, pool=True) +
ops.eca_finish (conv_mfma_bf16x3<3, 1, false, 14>, eca_scale_kernel, eca_apply_kernel<2>).  The same MFMAs in the same order, the same
summation tree of the pool and the same epilogue expression must give the same BITS: partial, gate and out are compared as integers, no
element exempt, no tolerance.

1. Bit-equality at 1x8x32 (one full tile), 1x9x33 (a 1-row and a 1-column tile), 1x1x1, 2x17x70 (runs cross strips and images), 1x97x131,
   2x64x96, 3x40x64, with slopes 0.25, 0.1 (not an fp16 number), 1.0 and 0.0; r about half negative, at 1x9x33 with +-0 and fp16 subnormals
   in it.  `out`, `partial` and `gate` sit between sentinels that must come back untouched.  Two runs are bit-identical.
2. The size rule with the switch unset, on either side of it: 7x151x992 (32,767 strip-rows: the three old launches) and 8x64x2048
   (32,768: the new path), which path ran read from the timer tag.
3. The PReLU staging (the in-place rewrite of a landed row piece) over all 65,536 fp16 bit patterns x those slopes, through the test hook
   paif_eca_conv2_staged_f16 (out = the operand rows as staged), against f32 -> f16 (RNE) of (v >= 0 ? v : fp32(a * v)) computed on the
   CPU.  NaN inputs (2,046 patterns) must come out NaN; their payload bits are not compared.
4. A torch.cuda.graph capture + replay of the block's tail equals the eager result.
5. The whole Network_Fusion_Searched forward under fp16 storage at 1x97x131 and 2x64x96: PAIF_ECA_ROWS=0 against =1, bit-identical."""
import functools
import os

import pytest
import torch

from paif_amd import _lib, ops, synthetic as S
from tests.helpers import t
from tests.kernel_check import dev as _dev, exact as _exact, gen

pytestmark = pytest.mark.gpu

F32, F16 = torch.float32, torch.float16
SWITCH = "PAIF_ECA_ROWS"
SENTINEL = 0x5A5B
PAD = 64                       # sentinel floats on either side of partial / gate
SLOPES = [0.25, 0.1, 1.0, 0.0]
SHAPES = [(1, 8, 32), (1, 9, 33), (1, 1, 1), (2, 17, 70), (1, 97, 131), (2, 64, 96), (3, 40, 64)]
SPECIAL = (1, 9, 33)           # the case with +-0 and subnormals in r
BELOW, ABOVE = (7, 151, 992), (8, 64, 2048)
OLD_CONV = "conv_mfma_bf16x3<3, 1, false, 14>"


def _switch(value):
    """paif_eca_conv2_gated_fits reads the variable on every call: None = unset, the size rule."""
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value


@pytest.fixture(autouse=True)
def _f16_storage():
    old, serp, env = dict(ops.CONFIG), ops._SERP[0], os.environ.get(SWITCH)
    ops.set_conv_precision("bf16x3")
    ops.set_storage("f16")
    yield
    ops.TIMER = None
    ops.set_storage("f32")
    ops.CONFIG.update(old)
    ops._SERP[0] = serp
    ops._ACT_BF16[0] = False
    _switch(env)


@functools.lru_cache(maxsize=4)
def _r(shape):
    """The block's r: seeded fp16 values, about half of them negative."""
    B, H, W = shape
    if B * H * W > 200000:
        x = torch.randn(B, H, W, 32, generator=torch.Generator(device=_dev()).manual_seed(9100 + B), device=_dev())
    else:
        x = torch.randn(B, H, W, 32, generator=gen(B, H, W, base=97)).to(_dev())
    x16 = ops.cast_storage(x, F16)
    if shape == SPECIAL:
        v = x16.view(torch.int16)
        sp = torch.tensor([0x0000, -0x8000, 0x0001, -0x7FFF, 0x03FF, -0x7C01, 0x0200, -0x7E00], dtype=torch.int16, device=_dev())   # +-0, subnormals
        v[0, :, 0::3, 0:8] = sp
        v[0, 4, :, 8:16] = sp
    return x16


@functools.lru_cache(maxsize=None)
def _params():
    g = gen(3, base=97)
    w = (torch.randn(32, 32, 3, 3, generator=g) * 0.05).to(F16).float()
    w1d = torch.randn(1, 1, 3, generator=g)
    return ops.pack_conv_weight(w.to(_dev()), 1, 32, 3, precision="f16"), w1d.to(_dev())


def _slope(a):
    return torch.tensor([a], dtype=F32, device=_dev())


def _guarded(n):
    """n floats between two runs of PAD sentinel floats."""
    buf = torch.empty(n + 2 * PAD, dtype=F32, device=_dev())
    buf.view(torch.int16).fill_(SENTINEL)
    return buf


def _guards_intact(tag, buf, n):
    edge = torch.full((2 * PAD,), SENTINEL, dtype=torch.int16)
    _exact(tag + " sentinels in front", buf[:PAD].view(torch.int16), edge)
    _exact(tag + " sentinels behind", buf[PAD + n:].view(torch.int16), edge)


@functools.lru_cache(maxsize=None)
def _old(shape, a):
    """Today's three launches: (partial, gate, out) as integer tensors on the CPU.  Computed once per case and left unchanged."""
    B, H, W = shape
    r, (wpk, w1d), sl = _r(shape), _params(), _slope(a)
    _switch("0")
    ops.TIMER = timer = ops.KernelTimer(lambda tag: True)
    o, partial = ops.conv2d([r], wpk, 3, 1, in_act=ops.ACT_PRELU, in_prelu=sl, pool=True)
    ops.TIMER = None
    assert [rec[0] for rec in timer.records] == [OLD_CONV]
    out = ops.eca_finish(o, r, partial, w1d, 3, sl)
    # eca_finish keeps its gate to itself: the same entry once more with a gate buffer of the test's
    gate = torch.empty((B, 32), dtype=F32, device=_dev())
    out2 = torch.empty_like(o)
    _lib.check(ops.lib().paif_eca_finish_fwd_f16(ops._pa(o), ops._pa(r), ops._p(partial), ops._p(w1d.contiguous()), 3, ops._p(sl), ops._p(gate),
                                                 ops._pa(out2), B, H, W, ops._stream()), "eca_finish")
    torch.cuda.synchronize()
    assert torch.equal(out2, out)
    return partial.view(torch.int32).cpu(), gate.view(torch.int32).cpu(), out.view(torch.int16).cpu()


def _new(shape, a, tag):
    """paif_eca_conv2_gated_fwd_f16 into guarded buffers: (partial, gate, out) as integer tensors on the CPU."""
    B, H, W = shape
    r, (wpk, w1d), sl = _r(shape), _params(), _slope(a)
    L = ops.lib()
    assert L.paif_eca_conv2_gated_fits(B, H, W) == 1
    nt = L.paif_conv2d_blocks(B, H, W) * 32
    pbuf, gbuf = _guarded(nt), _guarded(B * 32)
    big = torch.empty((B + 2, H, W, 32), dtype=F16, device=_dev())
    big.view(torch.int16).fill_(SENTINEL)
    partial, gate, out = pbuf[PAD:PAD + nt], gbuf[PAD:PAD + B * 32], big[1:B + 1]
    _lib.check(L.paif_eca_conv2_gated_fwd_f16(ops._pa(r), ops._p(wpk.data), ops._p(sl), ops._p(partial), ops._p(w1d.contiguous()), 3, ops._p(sl),
                                              ops._p(gate), ops._pa(out), B, H, W, ops._stream()), "eca_conv2_gated")
    torch.cuda.synchronize()
    _guards_intact(tag + " partial", pbuf, nt)
    _guards_intact(tag + " gate", gbuf, B * 32)
    edge = torch.full(tuple(big[0].view(torch.int16).shape), SENTINEL, dtype=torch.int16)
    _exact(tag + " guard image 0", big[0].view(torch.int16), edge)
    _exact(tag + " guard image B+1", big[B + 1].view(torch.int16), edge)
    return partial.view(torch.int32).cpu().view(-1, 32), gate.view(torch.int32).cpu().view(B, 32), out.view(torch.int16).cpu()


@pytest.mark.parametrize("a", SLOPES, ids=lambda a: "slope%g" % a)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bit_equal_to_the_three_launches_it_replaces(shape, a):
    tag = "%dx%dx%d slope %g" % (shape + (a,))
    ref = _old(shape, a)
    _switch("1")
    got = _new(shape, a, tag)
    for name, g, rf in zip(("partial", "gate", "out"), got, ref):
        print("%s %s: %d of %d words differ" % (tag, name, int((g != rf).sum()), g.numel()))
    for name, g, rf in zip(("partial", "gate", "out"), got, ref):
        _exact("%s %s" % (tag, name), g, rf)
    again = _new(shape, a, tag + " second run")
    for name, g, rf in zip(("partial", "gate", "out"), again, got):
        _exact("%s %s, second run" % (tag, name), g, rf)
    # the same through the helper ECABasicBlock calls, which names what it ran
    r, (wpk, w1d), sl = _r(shape), _params(), _slope(a)
    ops.TIMER = timer = ops.KernelTimer(lambda tg: True)
    out = ops.eca_block_tail(r, wpk, 3, w1d, sl)
    ops.TIMER = None
    torch.cuda.synchronize()
    assert [rec[0] for rec in timer.records] == [ops.ECA_ROWS_TAG]
    _exact(tag + " ops.eca_block_tail", out.view(torch.int16), ref[2])


@pytest.mark.parametrize("shape,new", [(BELOW, False), (ABOVE, True)], ids=["7x151x992-below", "8x64x2048-above"])
def test_size_rule_with_the_switch_unset(shape, new):
    B, H, W = shape
    a = 0.25
    ref = _old(shape, a)[2]
    r, (wpk, w1d), sl = _r(shape), _params(), _slope(a)
    _switch(None)
    assert ops.lib().paif_eca_conv2_gated_fits(B, H, W) == (1 if new else 0)
    ops.TIMER = timer = ops.KernelTimer(lambda tg: True)
    out = ops.eca_block_tail(r, wpk, 3, w1d, sl)
    ops.TIMER = None
    torch.cuda.synchronize()
    assert [rec[0] for rec in timer.records] == ([ops.ECA_ROWS_TAG] if new else [OLD_CONV])
    _exact("%dx%dx%d switch unset" % shape, out.view(torch.int16), ref)
    _switch("0")
    assert ops.lib().paif_eca_conv2_gated_fits(B, H, W) == 0
    _switch("1")
    assert ops.lib().paif_eca_conv2_gated_fits(B, H, W) == 1
    assert ops.lib().paif_eca_conv2_gated_fits(32, 1024, 1024) == 0          # 2 GiB of source: 32-bit offsets


@pytest.mark.parametrize("a", SLOPES, ids=lambda a: "slope%g" % a)
def test_prelu_staging_over_every_fp16_value(a):
    B, H, W = 1, 32, 64                                  # 2,048 pixels x 32 channels = every 16-bit pattern once
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    perm = torch.randperm(65536, generator=gen(5, base=97))
    x = bits[perm].view(B, H, W, 32).view(F16)
    v = x.float()
    want = torch.where(v >= 0, v, torch.tensor(a, dtype=F32) * v).to(F16)     # fp32 product rounded to fp32, then RNE to fp16
    nan = torch.isnan(v)
    assert int(nan.sum()) == 2046
    wpk, _ = _params()
    big = torch.empty((B + 2, H, W, 32), dtype=F16, device=_dev())
    big.view(torch.int16).fill_(SENTINEL)
    xd = x.to(_dev())
    _lib.check(ops.lib().paif_eca_conv2_staged_f16(ops._pa(xd), ops._p(wpk.data), ops._p(_slope(a)), ops._pa(big[1:2]), B, H, W, ops._stream()),
               "eca_conv2_staged")
    torch.cuda.synchronize()
    got = big[1].cpu().view(B, H, W, 32)
    edge = torch.full(tuple(big[0].view(torch.int16).shape), SENTINEL, dtype=torch.int16)
    _exact("staging guard image 0", big[0].view(torch.int16), edge)
    _exact("staging guard image 2", big[2].view(torch.int16), edge)
    assert bool(torch.isnan(got.float())[nan].all())
    gi, wi = got.view(torch.int16).clone(), want.view(torch.int16).clone()
    gi[nan], wi[nan] = 0, 0
    print("slope %g: %d of %d staged values differ" % (a, int((gi != wi).sum()), 65536 - 2046))
    _exact("staged operand, slope %g" % a, gi, wi)


def test_graph_replay_equals_eager():
    shape, a = (2, 17, 70), 0.1
    r, (wpk, w1d), sl = _r(shape), _params(), _slope(a)
    _switch("1")
    eager = ops.eca_block_tail(r, wpk, 3, w1d, sl)
    torch.cuda.synchronize()
    gs = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(gs):
        ops.eca_block_tail(r, wpk, 3, w1d, sl)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=gs):
            gout = ops.eca_block_tail(r, wpk, 3, w1d, sl)
    gout.zero_()
    graph.replay()
    torch.cuda.synchronize()
    _exact("graph replay", gout.view(torch.int16), eager.view(torch.int16).cpu())
    _exact("graph replay against the old path", gout.view(torch.int16), _old(shape, a)[2])


@pytest.mark.parametrize("shape", [(1, 97, 131), (2, 64, 96)], ids=lambda s: "x".join(map(str, s)))
def test_whole_forward_old_path_against_new(shape):
    from paif_amd.core.model_fusion_auto import Network_Fusion_Searched
    from paif_amd.genotypes import FUSION_AT

    net = Network_Fusion_Searched(32, None, FUSION_AT).eval()
    net.load_state_dict({k: t(S.formula_tensor("enhance_net." + k, tuple(v.shape))).to(v.dtype) for k, v in net.state_dict().items()}, strict=True)
    net = net.to(_dev())
    ir, vis, _ = S.make_batch(*shape)
    irt, ycc = t(ir).to(_dev()), ops.rgb2ycrcb(t(vis).to(_dev()))
    with torch.no_grad():
        _switch("0")
        ops.TIMER = t_old = ops.KernelTimer(lambda tg: True)
        ref = net(irt, ycc)
        _switch("1")
        ops.TIMER = t_new = ops.KernelTimer(lambda tg: True)
        out = net(irt, ycc)
        ops.TIMER = None
    torch.cuda.synchronize()
    old_tags, new_tags = [rec[0] for rec in t_old.records], [rec[0] for rec in t_new.records]
    n_blocks = new_tags.count(ops.ECA_ROWS_TAG)
    assert n_blocks >= 1 and ops.ECA_ROWS_TAG not in old_tags and old_tags.count(OLD_CONV) - new_tags.count(OLD_CONV) == n_blocks
    assert out.dtype == F32
    _exact("fused image %dx%dx%d" % shape, out.view(torch.int32), ref.view(torch.int32).cpu())
