"""GPU tests of conv3x3_h16_dma_rows (csrc/conv_dma_rows.hip): the 3x3 dilation-2 conv over one 16-bit NHWC-32 source with plain 16-bit
weights and no input activation, 0-3 residual maps, 16-bit output or fp32 output from fp16 maps, as a row-streaming LDS-DMA kernel.

1. Bit-equality with the kernel it replaces, in one process: the switch PAIF_CONV_DMA_ROWS is read per call, so the same `ops.conv2d`
   call runs with it at 0 (the persistent conv_bf16x3_ws<3, 2, S>, or the tile-per-workgroup conv_mfma_bf16x3<3, 2, false, S> on small
   maps) and at 1 (the new kernel wherever its 32-bit addressing holds), in both walk directions.  The same 18 MFMAs per pixel in the same
   order and the same epilogue expression must give the same bits.  Maps of at most 80,000 pixels are written into the middle of a
   (B + 2)-image buffer of sentinels, whose guard images must come back untouched.
   Shapes: 1x1x1; 1x2x33 (one row per parity, the second strip one column wide); 1x5x31 (H below the ring depth, W below a strip);
   2x7x70 (a ragged 6-column strip, B > 1); 3x37x53; 1x400x33 (runs longer than three ring depths: 13 waves of 64 / 32 strip-rows, each
   split at a chain boundary, so first and last runs are ragged); 2x64x96; 3x130x4100 (50,310 strip-rows: above the size rule, run with
   the switch UNSET against 0); 8x480x640 (the benchmarked shape, fp16, the forward's own form).
2. Against float64 on the CPU on 2x7x70, 3x37x53 and 1x400x33 with the switch at 1: F.conv2d over the source, then
   act(scale * z + shift) * alpha + sum(res) (the restatement of tests/test_dense_conv16_gpu.py), within the bounds of
   tests/kernel_check.py: `h16` per element for 16-bit outputs, `rev` for fp32 outputs.  No element is exempt.
3. The dispatch rule, by host-only name queries.

The ReLU-input forms (the composed DilConv, with or without the fused ChannelPool) are not built on this kernel: they keep
conv3x3_h16_dma<1, NRES, F, CP, 2, 2>, which the dispatch test asserts."""
import ctypes
import functools
import os

import pytest
import torch
import torch.nn.functional as F

from paif_amd import _lib, ops
from tests.kernel_check import REV, dev as _dev, exact as _exact, gen, h16 as _h16, rev as _rev

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FMTS = [F16, BF16]
EPS16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
NAME = {BF16: "bf16", F16: "f16"}
FCODE = {BF16: 1, F16: 2}
SCODE = {BF16: 4, F16: 12}
SENTINEL = 0x5A5B
GUARD_PIXELS = 80000
SWITCH = "PAIF_CONV_DMA_ROWS"

SMALL = [(1, 1, 1), (1, 2, 33), (1, 5, 31), (2, 7, 70), (3, 37, 53), (1, 400, 33), (2, 64, 96)]
F64_SHAPES = [(2, 7, 70), (3, 37, 53), (1, 400, 33)]
ABOVE, BENCH = (3, 130, 4100), (8, 480, 640)
# the dilation-2 shapes whose kernel names the other test modules pin
PINNED = [(1023, 9, 1), (1023, 1, 33), (704, 9, 1), (600, 3, 40), (512, 8, 64), (1, 250, 1030), (31, 70, 100), (1023, 2, 545), (512, 2, 2017),
          (1023, 8, 32), (2, 37, 53), (1, 1, 1), (1, 3, 3), (3, 8, 32), (1, 9, 33), (128, 8, 64), (2, 333, 517), (1, 480, 640), (4, 96, 100),
          (1, 64, 96), (2, 64, 96)]


class Form:
    """nres residual maps, output activation act (0 none, 1 PReLU, 2 ReLU), with / without scale and shift, alpha, fp32 output."""

    def __init__(self, nres, act, affine, alpha, out_f32=False):
        self.nres, self.act, self.affine, self.alpha, self.out_f32 = nres, act, affine, alpha, out_f32

    @property
    def id(self):
        return "r%d-a%d-%s-alpha%g%s" % (self.nres, self.act, "affine" if self.affine else "noaffine", self.alpha, "-f32" if self.out_f32 else "")


# NRES 0 / 1 / 2 / 3, the three activations, with and without scale / shift, alpha = 1 and != 1, 16-bit and fp32 output
FORMS = [Form(0, 0, False, 1.0), Form(0, 1, True, 0.5), Form(1, 0, True, 1.0), Form(2, 2, True, 0.5), Form(3, 0, True, 0.7), Form(3, 1, False, 1.5),
         Form(2, 1, True, 0.5, out_f32=True), Form(0, 2, False, 1.5, out_f32=True), Form(3, 2, True, 0.7, out_f32=True)]
BENCH_FORM = FORMS[6]


def _forms(dt):
    return [f for f in FORMS if dt is F16 or not f.out_f32]       # fp32 output: fp16 maps only


def _cases():
    out = []
    for dt in FMTS:
        for shape in SMALL:
            out += [(shape, dt, f) for f in _forms(dt)]
        out += [(ABOVE, dt, FORMS[3]), (ABOVE, dt, FORMS[4])]
    out += [(ABOVE, F16, BENCH_FORM), (BENCH, F16, BENCH_FORM)]
    return out


def _id(c):
    return "%dx%dx%d-%s-%s" % (c[0] + (NAME[c[1]], c[2].id))


@pytest.fixture(autouse=True)
def _default_arithmetic():
    old, serp, env = dict(ops.CONFIG), ops._SERP[0], os.environ.get(SWITCH)
    ops.set_conv_precision("bf16x3")
    yield
    ops.CONFIG.update(old)
    ops._SERP[0] = serp
    ops._ACT_BF16[0] = False
    ops._TWINS.clear()
    _switch(env)


def _switch(value):
    """The dispatcher reads the variable on every call (getenv): None = unset, the size rule."""
    if value is None:
        os.environ.pop(SWITCH, None)
    else:
        os.environ[SWITCH] = value


@functools.lru_cache(maxsize=8)
def _map(shape, dt, idx):
    """Map `idx` of a shape (0 the source, 1-3 residual maps), values of the format, on the device.  The large maps are drawn on the
    device (seeded), the small ones on the CPU like the other direct kernel tests."""
    B, H, W = shape
    if B * H * W > 200000:
        g = torch.Generator(device=_dev()).manual_seed(7100 + 10 * FCODE[dt] + idx)
        x = torch.randn(B, H, W, 32, generator=g, device=_dev())
    else:
        x = torch.randn(B, H, W, 32, generator=gen(B, H, W, FCODE[dt], idx, base=83)).to(_dev())
    x16 = ops.cast_storage(x, dt)
    assert x16.dtype == dt
    return x16


@functools.lru_cache(maxsize=None)
def _params(dt):
    g = gen(FCODE[dt], base=83)
    w = (torch.randn(32, 32, 3, 3, generator=g) * 0.05).to(dt).float()      # representable: exact products
    return w, torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1


def _desc(dt, nsrc=1, nres=0, kh=3, dil=2, in_act=0, out_f32=False, storage=None, precision=None):
    """The fields the dispatcher reads; only null / non-null matters for the pointers of a name query."""
    d = _lib.ConvDesc()
    one = ctypes.c_void_p(16)
    for i in range(3):
        d.src[i] = one if i < nsrc else None
        d.res[i] = one if i < nres else None
    d.wpk, d.out = one, one
    d.nsrc, d.cin, d.cout, d.kh, d.dil, d.alpha, d.in_act = nsrc, 32, 32, kh, dil, 1.0, in_act
    d.storage = ((4 if out_f32 else 3) if dt is F16 else 1) if storage is None else storage
    d.precision = (4 if dt is F16 else ops.PREC_BF16) if precision is None else precision
    return d


def _new_name(dt, form):
    return "conv3x3_h16_dma_rows<%d, %d, %s>" % (FCODE[dt], form.nres, "true" if form.out_f32 else "false")


def _launch(shape, dt, form, reverse):
    """One ops.conv2d call under the current switch: (out, kernel name).  Checks the guard images."""
    B, H, W = shape
    dev = _dev()
    w, scale, shift = _params(dt)
    src = _map(shape, dt, 0)
    res = [_map(shape, dt, 1 + i) for i in range(form.nres)]
    ops.set_storage(NAME[dt])
    wpk = ops.pack_conv_weight(w.to(dev), 1, 32, 3, precision="f16" if dt is F16 else "bf16x3")
    name = ops.conv2d_kernel_name(_desc(dt, nres=form.nres, out_f32=form.out_f32), B, H, W)
    odt = F32 if form.out_f32 else dt
    big = None
    if B * H * W <= GUARD_PIXELS:
        big = torch.empty((B + 2, H, W, 32), device=dev, dtype=odt)
        big.view(torch.int16).fill_(SENTINEL)
    ops._SERP[0] = reverse ^ 1                          # conv2d flips it: this launch gets reverse_tiles = reverse
    out = ops.conv2d([src], wpk, 3, dil=2, scale=scale.to(dev) if form.affine else None, shift=shift.to(dev) if form.affine else None,
                     act=form.act, prelu=torch.tensor([0.2], device=dev) if form.act == 1 else None, alpha=form.alpha, res=tuple(res),
                     out_f32=form.out_f32, out=None if big is None else big[1:B + 1])
    torch.cuda.synchronize()
    assert ops._SERP[0] == reverse and out.dtype == odt and tuple(out.shape) == (B, H, W, 32)
    if big is not None:
        edge = torch.full(tuple(big[0].view(torch.int16).shape), SENTINEL, dtype=torch.int16)
        _exact("%s rev%d guard image 0" % (name, reverse), big[0].view(torch.int16), edge)
        _exact("%s rev%d guard image B+1" % (name, reverse), big[B + 1].view(torch.int16), edge)
    return out, name


@pytest.mark.parametrize("case", _cases(), ids=_id)
def test_bit_equal_to_the_kernel_it_replaces(case):
    shape, dt, form = case
    tag = _id(case)
    on = None if shape == ABOVE else "1"                # above the size rule the kernel is taken with the switch unset
    _switch("0")
    ref, old_name = _launch(shape, dt, form, 0)
    ref = ref.view(torch.int16).cpu()                    # the raw patterns (fp32 outputs as pairs of 16-bit words)
    ref_rev, _ = _launch(shape, dt, form, 1)
    _exact(tag + " old kernel, reverse walk", ref_rev.view(torch.int16), ref)
    del ref_rev
    assert "h16_dma" not in old_name, old_name
    big = shape[0] * ((shape[1] + 7) // 8) * ((shape[2] + 31) // 32) >= 1024
    code = 15 if form.out_f32 else SCODE[dt]
    assert old_name == ("conv_bf16x3_ws<3, 2, %d>" if big else "conv_mfma_bf16x3<3, 2, false, %d>") % code, old_name
    for reverse in (0, 1):
        _switch(on)
        got, name = _launch(shape, dt, form, reverse)
        assert name == _new_name(dt, form) and name != old_name, name
        got = got.view(torch.int16).cpu()
        ndiff = int((got != ref).sum())
        print("%s rev%d: %d of %d 16-bit words differ from %s" % (tag, reverse, ndiff, got.numel(), old_name))
        _exact("%s rev%d against %s" % (tag, reverse, old_name), got, ref)


@functools.lru_cache(maxsize=2)
def _sum64(shape, dt):
    """The conv sums in float64 (NHWC), once per shape and format."""
    x = ops.cast_storage(_map(shape, dt, 0), F32).cpu().permute(0, 3, 1, 2)
    return F.conv2d(x.double(), _params(dt)[0].double(), None, 1, 2, 2).permute(0, 2, 3, 1).contiguous()


@pytest.mark.parametrize("dt", FMTS, ids=NAME.get)
@pytest.mark.parametrize("shape", F64_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_against_float64(shape, dt):
    _, scale, shift = _params(dt)
    z = _sum64(shape, dt)
    _switch("1")
    for form in _forms(dt):
        tag = _id((shape, dt, form))
        got, name = _launch(shape, dt, form, 0)
        assert name == _new_name(dt, form), name
        v = z
        if form.affine:
            v = v * scale.double() + shift.double()
        if form.act == 1:
            v = torch.where(v >= 0, v, v * torch.tensor([0.2]).double())          # the slope as the kernel holds it: fp32(0.2)
        elif form.act == 2:
            v = v.clamp_min(0)
        v = v * form.alpha
        for i in range(form.nres):
            v = v + ops.cast_storage(_map(shape, dt, 1 + i), F32).cpu().double()
        if form.out_f32:
            _rev(tag, got, v)
        else:
            _h16(tag, got, v, EPS16[dt], REV * float(v.abs().max()))


def test_dispatch_rule():
    name = ops.conv2d_kernel_name
    for dt in FMTS:
        for form in _forms(dt):
            d = _desc(dt, nres=form.nres, out_f32=form.out_f32)
            _switch(None)
            for shape in ((8, 480, 640), (16, 480, 640)):
                assert name(d, *shape) == _new_name(dt, form), (shape, form.id)
            # the pinned shapes keep today's kernel, which is the one the switch at 0 gives everywhere
            for shape in PINNED:
                _switch(None)
                now = name(d, *shape)
                _switch("0")
                assert now == name(d, *shape) and "dma_rows" not in now, (shape, form.id, now)
            for shape in ((8, 480, 640), (16, 480, 640), ABOVE):
                assert "dma_rows" not in name(d, *shape)
        S = SCODE[dt]
        _switch(None)
        d = _desc(dt, nres=2)
        assert name(d, 1, 250, 1030) == "conv_bf16x3_ws<3, 2, %d>" % S
        assert name(d, 2, 64, 96) == "conv_mfma_bf16x3<3, 2, false, %d>" % S
        assert name(d, 3, 130, 4100) == "conv3x3_h16_dma_rows<%d, 2, false>" % FCODE[dt]                  # 50,310 strip-rows
        assert name(d, 8, 63, 640 * 8) == "conv_bf16x3_ws<3, 2, %d>" % S                                   # H below 64
        assert name(d, 4, 480, 544) == "conv_bf16x3_ws<3, 2, %d>" % S                                      # 32,640 strip-rows
        assert name(d, 4, 482, 544) == "conv3x3_h16_dma_rows<%d, 2, false>" % FCODE[dt]                   # 32,776
        _switch("1")
        assert name(d, 1, 1, 1) == "conv3x3_h16_dma_rows<%d, 2, false>" % FCODE[dt]
        assert "dma_rows" not in name(d, 32, 1024, 1024)                                                   # 2 GiB of source: 32-bit offsets
        B, H, W = 8, 480, 640
        for sw in (None, "1"):
            _switch(sw)
            # split-bf16 weights, fp32 storage, two sources, dilation 1, an ECA pool, an input ReLU, a fused ChannelPool: today's kernels
            if dt is BF16:
                assert name(_desc(dt, nres=2, precision=1), B, H, W) == "conv_bf16x3_ws<3, 2, 1>"
            assert name(_desc(dt, nres=2, storage=0, precision=1), B, H, W) == "conv_mfma_bf16x3<3, 2, false, 0>"
            assert "dma_rows" not in name(_desc(dt, nsrc=2, nres=2), B, H, W)
            assert "dma_rows" not in name(_desc(dt, nres=2, dil=1), B, H, W)
            assert name(_desc(dt, nres=1, dil=1), B, H, W) == "conv3x3_h16_dma<1, 1, %d, false, 1, 0>" % FCODE[dt]
            d = _desc(dt, nres=2)
            d.pool_partial = ctypes.c_void_p(16)
            assert "dma_rows" not in name(d, B, H, W)
            assert name(_desc(dt, nres=1, in_act=2), B, H, W) == "conv3x3_h16_dma<1, 1, %d, false, 2, 2>" % FCODE[dt]
            assert name(_desc(dt, nres=3, in_act=2), B, H, W) == "conv3x3_h16_dma<1, 3, %d, false, 2, 2>" % FCODE[dt]
            d = _desc(dt, nres=1)
            d.cpool = ctypes.c_void_p(16)
            assert name(d, B, H, W) == "conv_bf16x3_ws<3, 2, %d>" % S
            assert ops.lib().paif_conv2d_can_cpool(ctypes.byref(d), B, H, W) == 1
    _switch(None)
    os.environ["PAIF_CONV_DMA"] = "0"
    try:
        assert name(_desc(F16, nres=2, out_f32=True), 8, 480, 640) == "conv_bf16x3_ws<3, 2, 15>"
    finally:
        del os.environ["PAIF_CONV_DMA"]
