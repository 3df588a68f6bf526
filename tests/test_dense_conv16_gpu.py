"""Direct float64 tests of the dense conv in 16-bit storage (bf16 and IEEE fp16 maps, weights representable in the format): the
LDS-DMA kernels of csrc/conv_dma.hip and csrc/conv_dma_1x1.hip at the shapes where their schedules change, and the kernels of
csrc/conv_mfma.hip that 16-bit maps take where the LDS-DMA forms are not eligible.

Every case calls `ops.conv2d` once per walk direction, asserts the kernel the dispatcher picks (`ops.conv2d_kernel_name`) and
compares the result with a float64 restatement in plain torch: F.conv2d over the concatenated sources (behind the input
activation where the form has one), then act(scale * z + shift) * alpha + sum(res).  No other kernel of the project serves
as the reference and no share of the elements is exempt.  Maps are randn made representable (cast_storage down and up),
weights randn * 0.05 (0.02 for 7x7) rounded to the format, so the products are exact and fp32 summation is the only
arithmetic error in front of the output rounding.

Bounds (tests/kernel_check.py):
  16-bit output, every element     |got - ref| <= 1.01 * eps16 * |ref| + REV * max|ref|   (h16; REV = 2e-5, the fp32 form's bound)
  fp32 output (fused ChannelPool plane, fp16 in / fp32 out)   max|err| <= REV * max|ref|  (rev); the pool reference is max_c /
                                   mean_c of the un-rounded float64 output; the half of `comp` the kernel does not own stays NaN
  rounding flips, 16-bit output    share of elements that differ from RNE16(ref64) <= 4 x the share of the fp32 CPU evaluation of
                                   the same reference at the same case (F.conv2d in fp32, RNE to the format) + 1e-4; maps under
                                   100,000 values (five of the six tile-per-workgroup shapes) meet it pooled per kernel
  guard images                     `out` is the middle of a (B + 2)-image buffer of sentinels: images 0 and B + 1 bit-equal after
                                   the launch (every LDS-DMA form at <= 80,000 pixels and every cout = 16 case)
  walk direction                   reverse_tiles = 0 and 1 give bit-equal outputs (every LDS-DMA case)

Shapes of the LDS-DMA forms (8 x 32 tiles; eligible from 1024 to 32768 tiles, B < 1024; 256 workgroups, XCD x walks the tile
range [x * ceil(n / 8), ...) with its 32 workgroups interleaved: `_cnts`):
  1023 x 9 x 1     2046 tiles, 7 / 8 per workgroup   one-pixel rows, the second tile row holds one row, every tile is border
  1023 x 1 x 33    2046 tiles, 7 / 8                 H = 1: only the centre row of taps in range; the second tile one column wide
   704 x 9 x 1     1408 tiles, 5 / 6                 6 = 2 mod 4 = 0 mod 3: the residue the other rows leave out (U = 4 and U = 3)
   600 x 3 x 40    1200 tiles, 4 / 5                 the map is smaller than the 3x3 / dilation-2 / 7x7 halo
   512 x 8 x 64    1024 tiles, 4                     exactly at the threshold, no ragged edge (128 x 8 x 64 has 256 tiles: it runs
                                                     with the tile-per-workgroup shapes below)
     1 x 250 x 1030  1056 tiles, 4 / 5               one image, ragged both ways
    31 x 70 x 100  1116 tiles, 4 / 5                 the XCD ranges straddle image boundaries
  1023 x 2 x 545   18414 tiles, 71 / 72              second half of the per-lane tile table (one- and two-source forms)
   512 x 2 x 2017  32768 tiles, 128                  the tile table exactly full (one-source forms)
  1023 x 8 x 32    1023 tiles                        one short of the threshold: not an LDS-DMA kernel, result checked
   513 x 2 x 2017  32832 tiles                       past the cap: the name alone (the query takes no memory)
The tile loop is unrolled by U residual register sets (Sched: U = 4 one source, 2 two / three sources, 3 dilation 2):
test_unroll_residues_are_covered asserts that every residue of (tiles per workgroup) mod U is met for each of them.
conv_h16_dma_1x1 walks 64-pixel runs over 2048 waves: 9,207 = 143 * 64 + 55 pixels (most waves idle, last run partial),
512 x 8 x 64 (divides exactly), 2 x 333 x 517 (every wave has runs).

Kernels this module must see (test_every_listed_kernel_was_seen compares this list with the names asserted above):
    conv3x3_h16_dma<1, 0, F, false, 1, 0>
    conv3x3_h16_dma<1, 1, F, false, 1, 0>
    conv3x3_h16_dma<2, 0, F, false, 1, 0>
    conv3x3_h16_dma<2, 1, F, false, 1, 0>
    conv3x3_h16_dma<2, 2, F, false, 1, 0>
    conv3x3_h16_dma<2, 3, F, false, 1, 0>
    conv3x3_h16_dma<3, 0, F, false, 1, 0>
    conv3x3_h16_dma<3, 1, F, false, 1, 0>
    conv3x3_h16_dma<3, 2, F, false, 1, 0>
    conv3x3_h16_dma<3, 3, F, false, 1, 0>
    conv3x3_h16_dma<3, 1, F, true, 1, 0>
    conv3x3_h16_dma<3, 3, F, true, 1, 0>
    conv3x3_h16_dma<1, 1, F, false, 2, 2>
    conv3x3_h16_dma<1, 3, F, false, 2, 2>
    conv3x3_h16_dma<1, 1, F, true, 2, 2>
    conv3x3_h16_dma<1, 3, F, true, 2, 2>
    conv7x7_h16_dma<F>
    conv_h16_dma_1x1<F>
    conv_mfma_bf16x3<1, 1, false, S>
    conv_mfma_bf16x3<3, 1, false, S>
    conv_mfma_bf16x3<3, 2, false, S>
    conv_mfma_bf16x3<7, 1, false, S>
    conv_mfma_bf16x3<3, 1, false, 6>
    conv_bf16x3_ms<3, 1, 2, 4>
    conv_bf16x3_ms<3, 1, 3, 4>
    conv_bf16x3_ws<1, 1, S>
    conv_bf16x3_ws<3, 2, S>
    conv_bf16x3_wsr<3, 2, S>
    conv_bf16x3_ws<3, 2, 15>
(F = 1 bf16 and 2 fp16; S = 4 bf16 and 12 fp16, the storage code of plain 16-bit weights; 6: bf16 behind an input PReLU; 15:
fp16 in / fp32 out; conv_bf16x3_ms: the kernel bf16 maps with two or three sources take below the LDS-DMA threshold.)
Every check prints its ERR line; the flip shares follow the rounding bound on the same line."""
import ctypes
import functools
import re

import pytest
import torch
import torch.nn.functional as F

from paif_amd import _lib, ops
from tests.kernel_check import REV, dev as _dev, exact as _exact, flips as _flips, flips_pooled as _flips_pooled, gen, h16 as _h16, rev as _rev, rne16 as _rne16

pytestmark = pytest.mark.gpu

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FMTS = [BF16, F16]
EPS16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}
NAME = {BF16: "bf16", F16: "f16"}
FCODE = {BF16: 1, F16: 2}             # template argument F of the LDS-DMA kernels
SCODE = {BF16: 4, F16: 12}            # storage code of the conv_mfma.hip kernels with plain 16-bit weights
ALPHA = 0.5
SENTINEL = 0x5A5B                     # bit pattern of the guard images (a finite value in either format)
GUARD_PIXELS = 80000
SEEN = set()
POOL_VALUES = 100000                # a map with fewer values is held to the flip bound in the pool of its kernel, not alone
POOL = {}                            # kernel name -> flip counts of its cases at TILE_SHAPES

# ---- shapes ----------------------------------------------------------------------------------------------------------------
ROWS1, H1, TINY, HALO, EXACT, ONE, STRADDLE = (1023, 9, 1), (1023, 1, 33), (704, 9, 1), (600, 3, 40), (512, 8, 64), (1, 250, 1030), (31, 70, 100)
SMALL = [ROWS1, H1, TINY, HALO, EXACT, ONE, STRADDLE]      # every LDS-DMA form
TABLE_HI, TABLE_FULL = (1023, 2, 545), (512, 2, 2017)       # one- and two-source forms / one-source forms
BELOW, PAST = (1023, 8, 32), (513, 2, 2017)
RUNS_1X1 = [ROWS1, EXACT, (2, 333, 517)]
TILE_SHAPES = [(2, 37, 53), (1, 1, 1), (1, 3, 3), (3, 8, 32), (1, 9, 33), (128, 8, 64)]
WS_SHAPES = [HALO, ONE]


def _tiles(B, H, W):
    return B * ((H + 7) // 8) * ((W + 31) // 32)


def _cnts(n, grid=256):
    """Tiles per workgroup of the persistent 3x3 / 7x7 LDS-DMA kernels (conv_dma.hip: xcd = block & 7, wg = block >> 3)."""
    nwg, tpx, out = grid >> 3, (n + 7) >> 3, set()
    for x in range(8):
        t_beg = x * tpx
        t_end = min(n, t_beg + tpx)
        out |= {(t_end - t_beg - wg + nwg - 1) // nwg for wg in range(nwg) if t_beg + wg < t_end}
    return out


# ---- cases -----------------------------------------------------------------------------------------------------------------
class Case:
    """One launch: kh x kh conv, dilation dil, nsrc sources, nres residual maps, output activation act (0 none, 1 PReLU, 2 ReLU),
    input activation in_act, cout channels, fused ChannelPool at offset pool (None: no pool), fp32 output from fp16 maps."""

    def __init__(self, shape, dt, kh, dil, nsrc, nres, act, kernel, cout=32, in_act=0, pool=None, out_f32=False, affine=True):
        self.shape, self.dt, self.kh, self.dil, self.nsrc, self.nres, self.act, self.cout = shape, dt, kh, dil, nsrc, nres, act, cout
        self.in_act, self.pool, self.out_f32, self.affine = in_act, pool, out_f32, affine
        self.kernel = kernel.replace("F", str(FCODE[dt])).replace("S", str(SCODE[dt]))
        self.dma = "h16_dma" in self.kernel

    @property
    def id(self):
        B, H, W = self.shape
        s = "%dx%dx%d-%s-k%dd%d-s%dr%d-a%d" % (B, H, W, NAME[self.dt], self.kh, self.dil, self.nsrc, self.nres, self.act)
        return s + ("-c16" if self.cout == 16 else "") + ("-in%d" % self.in_act if self.in_act else "") + \
            ("-pool%d" % self.pool if self.pool is not None else "") + ("-f32" if self.out_f32 else "") + ("" if self.affine else "-noaffine")


# (nsrc, nres, act, cout, pool): every built source / residual count of conv3x3_h16_dma at dilation 1, the activations spread
D1_FORMS = [(1, 0, 1, 32, None), (1, 1, 0, 32, None), (1, 0, 0, 16, None), (2, 0, 2, 32, None), (2, 1, 1, 32, None), (2, 2, 0, 32, None),
            (2, 3, 2, 32, None), (3, 0, 1, 32, None), (3, 1, 0, 32, None), (3, 2, 2, 32, None), (3, 3, 1, 32, None), (3, 1, 1, 32, 0),
            (3, 3, 2, 32, 2)]
D2_FORMS = [(1, 1, None), (3, 0, None), (1, 2, 0), (3, 1, 2)]          # (nres, act, pool) of conv3x3_h16_dma<1, NRES, F, CP, 2, 2>
EPI_1X1 = [(0, False), (1, True), (2, True), (0, True)]                # (act, affine) of the four epilogue variants of the 1x1


def _d1(shape, dt, form, kernel="dma"):
    nsrc, nres, act, cout, pool = form
    if kernel == "dma":
        kernel = "conv3x3_h16_dma<%d, %d, F, %s, 1, 0>" % (nsrc, nres, "true" if pool is not None else "false")
    return Case(shape, dt, 3, 1, nsrc, nres, act, kernel, cout=cout, pool=pool)


def _d2(shape, dt, form):
    nres, act, pool = form
    return Case(shape, dt, 3, 2, 1, nres, act, "conv3x3_h16_dma<1, %d, F, %s, 2, 2>" % (nres, "true" if pool is not None else "false"),
                in_act=2, pool=pool)


def _dma_cases():
    out = []
    for dt in FMTS:                                   # (grouped so that the cached float64 sums are reused)
        for shape in SMALL:
            out += [_d1(shape, dt, f) for f in D1_FORMS]
            out += [_d2(shape, dt, f) for f in D2_FORMS]
            out += [Case(shape, dt, 7, 1, 1, 0, act, "conv7x7_h16_dma<F>") for act in (0, 1, 2)]
        for shape, forms in ((TABLE_HI, [D1_FORMS[0], D1_FORMS[1], D1_FORMS[3], D1_FORMS[6]]), (TABLE_FULL, [D1_FORMS[0], D1_FORMS[1]])):
            out += [_d1(shape, dt, f) for f in forms] + [_d2(shape, dt, D2_FORMS[0])]
        for shape in RUNS_1X1:
            out += [Case(shape, dt, 1, 1, 3, 0, act, "conv_h16_dma_1x1<F>", affine=aff) for act, aff in EPI_1X1]
    return out


def _other_cases():
    out = []
    for dt in FMTS:
        ms = dt is BF16       # bf16 maps with two or three sources: the multi-source kernel; fp16 maps: the tile-per-workgroup kernel
        plain3 = "conv_mfma_bf16x3<3, 1, false, S>"
        # one tile short of the LDS-DMA threshold
        out += [_d1(BELOW, dt, D1_FORMS[0], plain3), _d1(BELOW, dt, D1_FORMS[4], "conv_bf16x3_ms<3, 1, 2, 4>" if ms else plain3),
                _d1(BELOW, dt, D1_FORMS[10], "conv_bf16x3_ms<3, 1, 3, 4>" if ms else plain3),
                Case(BELOW, dt, 3, 2, 1, 1, 1, "conv_mfma_bf16x3<3, 2, false, S>", in_act=2),
                Case(BELOW, dt, 7, 1, 1, 0, 1, "conv_mfma_bf16x3<7, 1, false, S>"),
                Case(BELOW, dt, 1, 1, 3, 0, 1, "conv_mfma_bf16x3<1, 1, false, S>")]
        # the tile-per-workgroup kernel
        for shape in TILE_SHAPES:
            out += [Case(shape, dt, 1, 1, 1, 2, 1, "conv_mfma_bf16x3<1, 1, false, S>"),
                    Case(shape, dt, 3, 1, 1, 1, 1, plain3),
                    Case(shape, dt, 3, 1, 2, 0, 2, "conv_bf16x3_ms<3, 1, 2, 4>" if ms else plain3),
                    Case(shape, dt, 3, 1, 3, 3, 0, "conv_bf16x3_ms<3, 1, 3, 4>" if ms else plain3),
                    Case(shape, dt, 3, 2, 1, 1, 1, "conv_mfma_bf16x3<3, 2, false, S>"),
                    Case(shape, dt, 7, 1, 1, 0, 2, "conv_mfma_bf16x3<7, 1, false, S>"),
                    Case(shape, dt, 3, 1, 1, 0, 0, plain3, cout=16)]
            if dt is BF16:
                out.append(Case(shape, dt, 3, 1, 1, 0, 1, "conv_mfma_bf16x3<3, 1, false, 6>", in_act=1))
        # the wave-specialised persistent kernel
        for shape in WS_SHAPES:
            out += [Case(shape, dt, 1, 1, 1, 0, 1, "conv_bf16x3_ws<1, 1, S>"), Case(shape, dt, 1, 1, 2, 0, 2, "conv_bf16x3_ws<1, 1, S>"),
                    Case(shape, dt, 3, 2, 1, 0, 1, "conv_bf16x3_ws<3, 2, S>"), Case(shape, dt, 3, 2, 1, 2, 0, "conv_bf16x3_ws<3, 2, S>"),
                    Case(shape, dt, 3, 2, 1, 0, 0, "conv_bf16x3_wsr<3, 2, S>", in_act=2),
                    Case(shape, dt, 3, 2, 1, 2, 1, "conv_bf16x3_wsr<3, 2, S>", in_act=2)]
            if dt is F16:
                out.append(Case(shape, dt, 3, 2, 1, 2, 1, "conv_bf16x3_ws<3, 2, 15>", out_f32=True))
    return out


DMA_CASES, OTHER_CASES = _dma_cases(), _other_cases()


# ---- inputs and references -------------------------------------------------------------------------------------------------
def _gen(*key):
    return gen(*key, base=61)


@pytest.fixture(autouse=True)
def _default_arithmetic():
    old, serp = dict(ops.CONFIG), ops._SERP[0]
    ops.set_conv_precision("bf16x3")
    yield
    ops.CONFIG.update(old)
    ops._SERP[0] = serp
    ops._ACT_BF16[0] = False
    ops._TWINS.clear()


@functools.lru_cache(maxsize=8)
def _map(shape, dt, idx):
    """Map `idx` of a shape (0-2 sources, 3-5 residual maps): (the 16-bit map on the device, the values it holds as CPU fp32)."""
    B, H, W = shape
    x = torch.randn(B, H, W, 32, generator=_gen(B, H, W, FCODE[dt], idx)).to(_dev())
    x16 = ops.cast_storage(x, dt)
    assert x16.dtype == dt
    return x16, ops.cast_storage(x16, F32).cpu()


@functools.lru_cache(maxsize=None)
def _params(dt, kh, nsrc, cout):
    g = _gen(FCODE[dt], kh, nsrc, cout)
    w = (torch.randn(cout, 32 * nsrc, kh, kh, generator=g) * (0.02 if kh == 7 else 0.05)).to(dt).float()      # representable: exact products
    return w, torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1


IN_SLOPE = 0.1875     # input PReLU: 3 / 16, so that slope * x is exact in fp32 and float64 alike and is rounded to the format once


@functools.lru_cache(maxsize=3)
def _sums(shape, dt, kh, dil, nsrc, cout, in_act):
    """The conv sums of a case in float64 and, as the yardstick of fp32 arithmetic, in fp32 (NHWC)."""
    x = torch.cat([_map(shape, dt, i)[1] for i in range(nsrc)], dim=-1).permute(0, 3, 1, 2)
    if in_act == 2:
        x = x.clamp_min(0)
    elif in_act == 1:     # the PReLU result is rounded to the format like every other operand (tests/test_bf16_storage_gpu.py)
        x = torch.where(x >= 0, x, x * IN_SLOPE).to(dt).float()
    w = _params(dt, kh, nsrc, cout)[0]
    pad = dil * (kh - 1) // 2
    z64 = F.conv2d(x.double(), w.double(), None, 1, pad, dil).permute(0, 2, 3, 1).contiguous()
    z32 = F.conv2d(x.contiguous(), w, None, 1, pad, dil).permute(0, 2, 3, 1).contiguous()
    return z64, z32


def _epilogue(z, case, scale, shift, slope, res):
    v = z
    if scale is not None:
        v = v * scale[:case.cout].to(z.dtype) + shift[:case.cout].to(z.dtype)
    if case.act == 1:
        v = torch.where(v >= 0, v, v * slope.to(z.dtype))
    elif case.act == 2:
        v = v.clamp_min(0)
    v = v * ALPHA
    for r in res:
        v = v + r.to(z.dtype)
    return v


def _desc(case, res16, comp):
    """The fields the dispatcher reads (plan_conv in csrc/conv_mfma.hip): storage, precision, nsrc, cin, kh, dil,
    cout, alpha, in_act, which res pointers are set, cpool (and pool_partial / the gradient hooks, unset here as in ops.conv2d
    for these calls).  storage and precision restate what ops.conv2d derives from the dtypes and the weight pack."""
    d = _lib.ConvDesc()
    f16 = case.dt is F16
    d.storage, d.precision = ((4 if case.out_f32 else 3), 4) if f16 else (1, ops.PREC_BF16)
    d.nsrc, d.cin, d.kh, d.dil, d.cout, d.alpha, d.in_act = case.nsrc, 32, case.kh, case.dil, case.cout, ALPHA, case.in_act
    for i, r in enumerate(res16):
        d.res[i] = ops._pa(r)
    if comp is not None:
        d.cpool = ctypes.c_void_p(comp.data_ptr() + 4 * case.pool)
    return d


def _check_case(case):
    B, H, W = case.shape
    dt, cout = case.dt, case.cout
    dev = _dev()
    tag = case.id
    w, scale, shift = _params(dt, case.kh, case.nsrc, cout)
    if not case.affine:
        scale = shift = None
    slope = torch.tensor([0.2])
    srcs = [_map(case.shape, dt, i)[0] for i in range(case.nsrc)]
    res16 = [_map(case.shape, dt, 3 + i)[0] for i in range(case.nres)]
    res32 = [_map(case.shape, dt, 3 + i)[1] for i in range(case.nres)]
    ops.set_storage(NAME[dt])
    wpk = ops.pack_conv_weight(w.to(dev), case.nsrc, 32, case.kh, precision="f16" if dt is F16 else "bf16x3")
    comp = torch.full((B, H, W, 4), float("nan"), device=dev) if case.pool is not None else None
    d = _desc(case, res16, comp)
    name = ops.conv2d_kernel_name(d, B, H, W)
    assert name == case.kernel, (tag, name)
    assert ("h16_dma" in name) == case.dma
    if comp is not None:
        assert ops.lib().paif_conv2d_can_cpool(ctypes.byref(d), B, H, W) == 1, tag          # fused, not the stand-alone pass behind the conv
    SEEN.add(name)
    odt = F32 if case.out_f32 else dt
    guard = (case.dma and B * H * W <= GUARD_PIXELS) or cout == 16
    kw = dict(dil=case.dil, cout=cout, in_act=case.in_act, in_prelu=torch.tensor([IN_SLOPE], device=dev) if case.in_act == 1 else None,
              scale=None if scale is None else scale.to(dev), shift=None if shift is None else shift.to(dev), act=case.act,
              prelu=slope.to(dev) if case.act == 1 else None, alpha=ALPHA, res=tuple(res16), out_f32=case.out_f32)
    outs = []
    for reverse in ((0, 1) if case.dma else (0,)):
        big = None
        if guard:
            big = torch.empty((B + 2, H, W, cout), device=dev, dtype=odt)
            big.view(torch.int16).fill_(SENTINEL)
        if comp is not None:
            comp.fill_(float("nan"))
        ops._SERP[0] = reverse ^ 1                      # conv2d flips it: this launch gets reverse_tiles = reverse
        out = ops.conv2d(srcs, wpk, case.kh, out=None if big is None else big[1:B + 1], cpool=None if comp is None else (comp, case.pool), **kw)
        torch.cuda.synchronize()
        assert ops._SERP[0] == reverse and out.dtype == odt and tuple(out.shape) == (B, H, W, cout)
        if big is not None:
            edge = torch.full((H, W, cout), SENTINEL, dtype=torch.int16)
            _exact("%s rev%d guard image 0" % (tag, reverse), big[0].view(torch.int16), edge)
            _exact("%s rev%d guard image B+1" % (tag, reverse), big[B + 1].view(torch.int16), edge)
        outs.append((out.cpu(), None if comp is None else comp.cpu()))
    z64, z32 = _sums(case.shape, dt, case.kh, case.dil, case.nsrc, cout, case.in_act)
    ref = _epilogue(z64, case, scale, shift, slope, res32)
    got, gcomp = outs[0]
    b32 = REV * float(ref.abs().max())
    if odt is F32:
        _rev(tag, got, ref)
    else:
        _h16(tag, got, ref, EPS16[dt], b32)
        ref16 = _rne16(ref, dt)
        cpu16 = _epilogue(z32, case, scale, shift, slope, res32).to(dt)
        counts = _flips(tag, got, cpu16, ref16, check=ref.numel() >= POOL_VALUES)
        if case.shape in TILE_SHAPES:
            POOL.setdefault(name, []).append(counts)
    if gcomp is not None:
        o = case.pool
        _rev(tag + " pool max", gcomp[..., o], ref.amax(dim=-1))
        _rev(tag + " pool mean", gcomp[..., o + 1], ref.mean(dim=-1))
        assert bool(torch.isnan(gcomp[..., 2 - o:4 - o]).all()), tag + ": the other half of comp was written"
    if len(outs) == 2:
        _exact(tag + " reverse walk", outs[1][0].view(torch.int16), got.view(torch.int16))
        if gcomp is not None:
            _exact(tag + " reverse walk pool", outs[1][1][..., o:o + 2], gcomp[..., o:o + 2])


@pytest.mark.parametrize("case", DMA_CASES, ids=lambda c: c.id)
def test_lds_dma_kernels(case):
    """conv3x3_h16_dma (dilation 1 and 2, with and without the fused ChannelPool, cout 32 and 16), conv7x7_h16_dma and
    conv_h16_dma_1x1 in both formats, both walk directions."""
    _check_case(case)


@pytest.mark.parametrize("case", OTHER_CASES, ids=lambda c: c.id)
def test_kernels_below_the_lds_dma_threshold(case):
    """The kernels 16-bit maps take where no LDS-DMA form is eligible: one tile short of the threshold, the tile-per-workgroup
    kernel (and the multi-source kernel of bf16 maps) on small and ragged maps, the wave-specialised persistent kernel."""
    assert not case.dma
    _check_case(case)


@pytest.mark.parametrize("dt", FMTS, ids=NAME.get)
def test_past_the_tile_table_is_not_an_lds_dma_kernel(dt):
    """513 x 2 x 2017 = 32832 tiles do not fit the 128-entry tile table of 256 workgroups; 512 images (32768) do."""
    for form in (D1_FORMS[0], D1_FORMS[1]):
        case = _d1(PAST, dt, form)
        assert _tiles(*PAST) == 32832 and _tiles(*TABLE_FULL) == 128 * 256
        d = _desc(case, [torch.empty(4, device=_dev(), dtype=dt)] * case.nres, None)
        assert "h16_dma" not in ops.conv2d_kernel_name(d, *PAST)
        assert ops.conv2d_kernel_name(d, *TABLE_FULL) == case.kernel
    assert _tiles(*BELOW) == 1023 and _tiles(*EXACT) == 1024


def test_unroll_residues_are_covered():
    """Every residue of (tiles per workgroup) mod U, U the number of residual register sets the tile loop is unrolled by
    (conv_dma.hip Sched: 4 for one source, 2 for two and three, 3 for the dilation-2 form), is met by each form's shapes.
    U and the 256 workgroups of `_cnts` restate the build as it is (CD_PF = 4, dim3(256) in launch_n / launch_d2): a build with
    another prefetch depth or grid needs them restated here."""
    assert _cnts(2046) == {7, 8} and _cnts(1408) == {5, 6} and _cnts(1200) == {4, 5} and _cnts(1024) == {4}
    assert _cnts(1056) == {4, 5} and _cnts(1116) == {4, 5} and _cnts(18414) == {71, 72} and _cnts(32768) == {128}
    met = {}
    for c in DMA_CASES:
        if c.kh == 3:
            u = 3 if c.dil == 2 else (4 if c.nsrc == 1 else 2)
            met.setdefault((c.dt, c.nsrc, c.nres, c.dil, c.cout, c.pool, u), set()).update(n % u for n in _cnts(_tiles(*c.shape)))
    assert len(met) == 2 * (len(D1_FORMS) + len(D2_FORMS))
    for key, residues in met.items():
        assert residues == set(range(key[-1])), (key, residues)
    hi = {(c.dt, c.nsrc, c.dil) for c in DMA_CASES if c.kh == 3 and max(_cnts(_tiles(*c.shape))) > 64}      # kk >= 64 of the tile table
    assert hi == {(dt, n, dl) for dt in FMTS for n, dl in ((1, 1), (2, 1), (1, 2))}


def test_pooled_flips_of_the_small_maps():
    """Runs behind the cases: a 1 x 1 x 1 map has 32 values and one flip there is a share of 3e-2, so maps under 100,000 values
    are held to the flip bound together with the other maps of the same kernel (all six tile-per-workgroup shapes, 2.2 M values)."""
    assert POOL
    for name, counts in sorted(POOL.items()):
        assert len(counts) >= len(TILE_SHAPES)
        _flips_pooled(name, counts)


def test_every_listed_kernel_was_seen():
    """Runs last: the names asserted by the cases above are the list in the module docstring, both formats."""
    listed = set()
    for line in re.findall(r"^    (conv\S.*)$", __doc__, flags=re.M):
        for dt in FMTS:
            listed.add(line.strip().replace("F", str(FCODE[dt])).replace("S", str(SCODE[dt])))
    assert {c.kernel for c in DMA_CASES + OTHER_CASES} == listed
    assert SEEN == listed, (sorted(listed - SEEN), sorted(SEEN - listed))
