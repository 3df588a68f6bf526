"""Direct float64 tests of the slab conv (csrc/conv_slab.h: conv_k, pack_ops_k, head32_fwd_k, head32_bwd_k; csrc/bffusion.hip: fold_k),
the exact-fp32 MFMA kernel under U2Fusion, SeAFusion, DIDFuse, BFFusion, DRDB / Fusion_Network and Fusion_Network2.

Every test drives ONE launch (the reflected transpose: the ring launch and its fold) through the entry point that reaches the form, on
signed random maps and weights, and compares it with plain torch in float64 on the CPU: F.conv2d, F.conv_transpose2d,
F.pad(mode="reflect"), tanh, where, and float64 autograd through the reflection pad for its transpose.  No reference restates tiles,
quads, the ring or the fold.  The branch of a masked reverse form is read off the taped map the test supplies (`where(taped > 0, 1,
slope)`, `(1 - t)(1 + t)`), so no element is near a switch and none is excluded.

Per case:
  1. value: max|err| <= 2e-5 * max|float64 conv sum| (kernel_check.REV; the pre-activation, the transposed sum, the conv part of an adding
     form).  The fp32 CPU evaluation of the same reference is printed beside it (`CPU32 | ...`).
  2. nothing else is written: every map is the middle of a buffer with one guard image before and after, every channel the launch does
     not own holds the bit pattern SENT and is compared through an int32 view afterwards (`GUARD | ...`) -- the input maps too.
  3. nothing else is read: SENT is a NaN, so a staged channel outside the form's slice (the K padding of a ragged chunk, which for
     U2Fusion is the slice being written) makes the output non-finite, which kernel_check.err refuses.  Slices a launch STORES start as
     SENT as well.
  4. exact zeros: the taped maps carry +0.0 and -0.0 (a border pixel and the last channel quad among them), the tanh tapes +-1.0 too;
     the `one_hot` tests put the whole cotangent on one planted element at a time.
  5. determinism: at 2x19x35 (2x18x31 reflected) every form runs twice, bit-equal.
  6. repack: test_bff_repack.

Shapes: a tile is 16 x 16 pixels and a wave owns four rows; the lists hold the smallest maps at which each edge exists (one pixel, less
than a tile, three images smaller than a tile, an exact tile, a second tile one pixel deep either way, 2 x 3 ragged tiles of two images;
for dilation 2 a map smaller than the dilation; for reflection 2x2, 3x3 where row 1 is also row H - 2, ring grids of exactly one tile
and one more)."""
import math

import pytest
import torch
import torch.nn.functional as F

from paif_amd import _lib, ops, synthetic
from tests.kernel_check import REV, dev as _dev, err as _err, exact as _exact, gen as _gen, rev as _rev, to_dev as _d

pytestmark = pytest.mark.gpu

BASE = 9176                      # this module's seed stream
SENT = 0x7FC5A5A5                # a quiet NaN with a payload: what an unowned channel holds before and after a launch

ZP = [(1, 1, 1), (1, 4, 5), (3, 5, 3), (1, 16, 16), (1, 17, 16), (1, 16, 17), (2, 19, 35)]
DIL = ZP + [(1, 2, 3)]
RF = [(1, 2, 2), (1, 3, 3), (1, 2, 17), (1, 17, 2), (1, 14, 14), (1, 15, 15), (2, 18, 31)]
DID = [(1, 2, 2)] + [s for s in ZP if s[1] >= 2 and s[2] >= 2]
TWICE = {(2, 19, 35), (2, 18, 31)}
# launch (M outputs, K inputs): every MB, more than one group, a padded block, more than one chunk
MK = [(16, 16), (32, 48), (48, 16), (64, 32), (80, 16), (112, 32), (144, 16)]


def _tag(*a):
    return "x".join(str(v) for v in a)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


def _lk(v, s):
    return torch.where(v > 0, v, s * v)


def _dlk(t, s):
    """LeakyReLU' off the taped output: exactly zero (either sign) takes the slope."""
    return torch.where(t > 0, torch.ones_like(t), torch.full_like(t, s))


def _conv(x, w, b=None, dil=1, refl=False):
    if w.shape[-1] == 1:
        return F.conv2d(x, w, b)
    if refl:
        return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"), w, b)
    return F.conv2d(x, w, b, padding=dil, dilation=dil)


def _conv_t(dz, w, dil=1, refl=False):
    """The transpose of _conv with respect to its input."""
    if w.shape[-1] == 1:
        return F.conv_transpose2d(dz, w)
    if refl:
        x = torch.zeros(dz.shape[0], w.shape[1], dz.shape[2], dz.shape[3], dtype=dz.dtype, requires_grad=True)
        (_conv(x, w, refl=True) * dz).sum().backward()
        return x.grad
    return F.conv_transpose2d(dz, w, padding=dil, dilation=dil)


class _Map:
    """An NHWC fp32 map as the middle B images of a (B + 2)-image buffer of SENT; `put` fills a channel slice from a CPU NCHW tensor."""

    def __init__(self, B, H, W, C):
        self.cpu = torch.full((B + 2, H, W, C), SENT, dtype=torch.int32).view(torch.float32)
        self.C = C

    def put(self, off, x):
        assert off % 4 == 0 and off + x.shape[1] <= self.C
        self.cpu[1:-1, :, :, off:off + x.shape[1]] = x.float().permute(0, 2, 3, 1)
        return self

    def up(self):
        self.full = self.cpu.to(_dev())
        self.d = self.full[1:-1]
        return self.d

    def get(self, off, n):
        return self.d[..., off:off + n].permute(0, 3, 1, 2).cpu()

    def rest(self, name, written=()):
        """Everything but the written channel slices of the middle images is bit-equal to what was uploaded."""
        after, before = self.full.cpu().view(torch.int32), self.cpu.view(torch.int32)
        keep = torch.ones(self.C, dtype=torch.bool)
        for off, n in written:
            keep[off:off + n] = False
        same = torch.equal(after[0], before[0]) and torch.equal(after[-1], before[-1]) and torch.equal(after[1:-1][..., keep], before[1:-1][..., keep])
        count = 2 * before[0].numel() + before[1:-1][..., keep].numel()
        print("GUARD | %s | %d values | %s" % (name, count, "bit-equal" if same else "CHANGED"))
        assert same, name


def _value(name, got, fn):
    """fn(dtype) -> (reference, the conv sum that scales the bound); float64 is the reference, float32 the CPU yardstick."""
    ref, scale = fn(torch.float64)
    c32 = fn(torch.float32)[0]
    bound = REV * float(scale.abs().max())
    print("CPU32 | %s | %.3e | %.3e" % (name, float((c32.double() - ref).abs().max()), bound))
    if scale is ref:
        _rev(name, got, ref)
    else:
        _err(name, got, ref, bound)


def _bits(name, a, b):
    _exact(name, a.full.view(torch.int32), b.full.cpu().view(torch.int32))


def _tape(g, B, C, H, W, tanh=False):
    """A signed randn tape with exact zeros of both signs planted (a border pixel, the last channel quad), +-1.0 too for a tanh tape.
    -> (tape, the planted (b, c, y, x))."""
    t = _randn(g, B, C, H, W)
    assert float(t.abs().min()) > 0
    plants = [((0, C - 1, 0, 0), -0.0), ((B - 1, 0, H - 1, W - 1), 0.0), ((0, max(C - 2, 0), H // 2, W // 2), 0.0), ((B - 1, min(1, C - 1), H // 2, W - 1), -0.0)]
    if tanh:
        plants += [((0, max(C - 3, 0), 0, W - 1), 1.0), ((B - 1, min(2, C - 1), H - 1, 0), -1.0)]
    if C == 1:      # a one-channel plane: one planted value per pixel, as many as the plane has room for
        pix = [(b, 0, y, x) for b in (0, B - 1) for y in sorted({0, H // 2, H - 1}) for x in sorted({0, W // 2, W - 1})]
        pix = list(dict.fromkeys(pix))
        plants = [(p, v) for p, (_, v) in zip(pix, plants)]
    for p, v in plants:
        t[p] = v
    z = t == 0
    if C > 1:
        assert bool((z & torch.signbit(t)).any()) and bool((z & ~torch.signbit(t)).any())
        assert not tanh or (bool((t == 1).any()) and bool((t == -1).any()))
    return t, [p for p, _ in plants]


def _cot(g, shape, plants, hot):
    """The cotangent: signed randn, or (hot = k) all of it on planted element k."""
    c = _randn(g, *shape)
    if hot is not None:
        c = torch.zeros(shape)
        c[plants[hot % len(plants)]] = 1.5
    return c


L = ops.lib
_p, _po, _st = ops._p, ops._po, ops._stream


def _call(fn_name, *args):
    _lib.check(getattr(L(), fn_name)(*args, _st()), fn_name)


# ---------------------------------------------------------------------------------------------
# the generic forms through ops._BffConv / _bff_conv / _bff_conv_t
# ---------------------------------------------------------------------------------------------
BFF_FWD = {"3x3 EPI_ACT": (9, 0, True, 0.2), "3x3 REFL_STAGE EPI_ACT": (9, 1, True, 0.01), "1x1 EPI_ACT": (1, 0, True, 0.1),
           "1x1 EPI_STORE": (1, 0, False, 1.0)}
BFF_T = {"1x1 MASK EPI_STORE": (1, 0, False), "3x3 MASK EPI_ADD": (9, 0, True), "3x3 MASK REFL_RING + fold": (9, 1, False)}
FORM_ID = {f: i for i, f in enumerate(list(BFF_FWD) + list(BFF_T))}
SLOPE_T = 0.2


def _bff_make(w, b, slope, refl):
    """w [co][K][k][k] in the order of the map's channels -> _BffConv; from K = 32 on it is packed from two weight parts given in swapped
    order (the second half first), as the BFFusion decoder packs (fused | earlier outputs | upsampled) into (upsampled | ...)."""
    co, K, taps = w.shape[0], w.shape[1], w.shape[2] * w.shape[3]
    cut = K // 2 + 4
    parts = [(_d(w), 0)] if K < 32 else [(_d(w[:, cut:]), cut), (_d(w[:, :cut]), 0)]
    return ops._BffConv(parts, co, K, taps, None if b is None else _d(b), slope, refl)


def _bff_fwd_params():
    return [pytest.param(f, M, K, B, H, W, id="%s-%dx%d-%s" % (f.replace(" ", "_"), M, K, _tag(B, H, W)))
            for f, v in BFF_FWD.items() for M, K in MK for B, H, W in (RF if v[1] else ZP)]


@pytest.mark.parametrize("form,M,K,B,H,W", _bff_fwd_params())
def test_bff_forward_forms(form, M, K, B, H, W):
    taps, refl, has_b, slope = BFF_FWD[form]
    g = _gen(FORM_ID[form], M, K, B, H, W, base=BASE)
    k = 3 if taps == 9 else 1
    w, b, x = _randn(g, M, K, k, k) / math.sqrt(K * taps), (_randn(g, M) if has_b else None), _randn(g, B, K, H, W)
    cv = _bff_make(w, b, slope, refl)
    soff, doff = 8, 12
    name = "bff %s @ %dx%d %s" % (form, M, K, _tag(B, H, W))

    def fn(dt):
        pre = _conv(x.to(dt), w.to(dt), None if b is None else b.to(dt), refl=bool(refl))
        return (_lk(pre, slope), pre) if has_b else (pre, pre)

    def run():
        src, dst = _Map(B, H, W, K + 12).put(soff, x), _Map(B, H, W, M + 20)
        ops._bff_conv(cv, src.up(), soff, dst.up(), doff, B, H, W)
        return src, dst

    src, dst = run()
    _value(name, dst.get(doff, M), fn)
    dst.rest(name + " out", [(doff, M)])
    src.rest(name + " in")
    if (B, H, W) in TWICE:
        _bits(name + " twice", run()[1], dst)


def _bff_t(form, Ml, Kl, B, H, W, n_store=0, hot=None):
    """The launch has Ml outputs and Kl inputs: the transpose of a conv with co = Kl and K = Ml."""
    taps, refl, add = BFF_T[form]
    co, K = Kl, Ml
    g = _gen(FORM_ID[form], Ml, Kl, B, H, W, n_store, base=BASE)
    k = 3 if taps == 9 else 1
    w = _randn(g, co, K, k, k) / math.sqrt(co * taps)
    cv = _bff_make(w, None, SLOPE_T, refl)
    t, plants = _tape(g, B, co, H, W)
    cot = _cot(g, (B, co, H, W), plants, hot)
    prior = _randn(g, B, K, H, W)
    first = 0 if add else (n_store if refl else K)        # channels from `first` on are added to
    ooff, ioff = 8, 12
    name = "bff %s%s @ %dx%d %s" % (form, (" n_store %d" % n_store if refl else "") + ("" if hot is None else " one-hot %d" % hot), Ml, Kl, _tag(B, H, W))

    def fn(dt):
        s = _conv_t(cot.to(dt) * _dlk(t.to(dt), SLOPE_T), w.to(dt), refl=bool(refl))
        r = s.clone()
        r[:, first:] += prior.to(dt)[:, first:]
        return r, s

    def ring_fn(dt):     # the gradient with respect to the PADDED plane: the zero-pad transpose on the (H + 2) x (W + 2) grid
        r = F.conv_transpose2d(cot.to(dt) * _dlk(t.to(dt), SLOPE_T), w.to(dt))
        return r, r

    def run():
        tp, do, di = _Map(B, H, W, co + 12).put(ooff, t), _Map(B, H, W, co + 12).put(ooff, cot), _Map(B, H, W, K + 20)
        if first < K:
            di.put(ioff + first, prior[:, first:])
        ring = _Map(B, H + 2, W + 2, K) if refl else None
        ops._bff_conv_t(cv, tp.up(), do.up(), ooff, di.up(), ioff, None if ring is None else ring.up(), add, n_store, B, H, W)
        return tp, do, di, ring

    tp, do, di, ring = run()
    _value(name, di.get(ioff, K), fn)
    if ring is not None:
        _value(name + " ring", ring.get(0, K), ring_fn)
        ring.rest(name + " ring", [(0, K)])
    di.rest(name + " out", [(ioff, K)])
    tp.rest(name + " tape")
    do.rest(name + " in")
    if (B, H, W) in TWICE and hot is None:
        _bits(name + " twice", run()[2], di)


def _bff_t_params():
    out = []
    for f, v in BFF_T.items():
        for M, K in MK:
            for i, (B, H, W) in enumerate(RF if v[1] else ZP):
                ns = (0, 4 * ((M // 2 + 3) // 4), M)[(i + M // 16) % 3] if v[1] else 0      # n_store: none, a part, all
                out.append(pytest.param(f, M, K, B, H, W, ns, id="%s-%dx%d-%s-%d" % (f.replace(" ", "_"), M, K, _tag(B, H, W), ns)))
    return out


@pytest.mark.parametrize("form,M,K,B,H,W,n_store", _bff_t_params())
def test_bff_transposed_forms(form, M, K, B, H, W, n_store):
    _bff_t(form, M, K, B, H, W, n_store)


def test_bff_fold_takes_every_n_store():
    """none, a part and all of the channels stored, at one shape per fold edge."""
    for B, H, W in [(1, 2, 2), (1, 3, 3), (2, 18, 31)]:
        for ns in (0, 16, 36, 48):
            _bff_t("3x3 MASK REFL_RING + fold", 48, 16, B, H, W, ns)


@pytest.mark.parametrize("form", list(BFF_T))
@pytest.mark.parametrize("hot", [0, 1, 2, 3])
def test_bff_zero_tape_one_hot(form, hot):
    """The whole cotangent on one planted +-0.0 of the tape: the launch gives slope times that element's column of the weight."""
    B, H, W = (2, 18, 31) if BFF_T[form][1] else (2, 19, 35)
    _bff_t(form, 80, 16, B, H, W, 40, hot=hot)


def test_bff_repack():
    """paif_bffusion_pack_ops a second time into the same zero-initialised pack: elements outside [off, off + n) stay as they were, and the
    run gives the new weights' result."""
    g = _gen(77, base=BASE)
    M, K, B, H, W, cut = 48, 32, 2, 19, 35, 20
    w, w2 = (_randn(g, M, K, 3, 3) / math.sqrt(9 * K) for _ in range(2))
    b, x = _randn(g, M), _randn(g, B, K, H, W)
    cv = _bff_make(w, b, 0.2, 0)                                   # parts (w[:, cut:], cut), (w[:, :cut], 0)
    only_low = ops._BffConv([(_d(w[:, :cut]), 0)], M, K, 9, _d(b), 0.2, 0)
    zero_hi = _d(torch.zeros(M, K - cut, 3, 3))
    for tr, pack, ref in ((0, cv.fwd, only_low.fwd), (1, cv.tr, only_low.tr)):
        Mp, Kp = (K, M) if tr else (M, K)
        _call("paif_bffusion_pack_ops", _p(zero_hi), M, K - cut, cut, Mp, Kp, 9, tr, _p(pack))
        _exact("repack: zeros into [cut, K) leave [0, cut) alone, %s" % ("transposed" if tr else "forward"), pack, ref.cpu())
    new_hi = _d(w2[:, cut:])
    _call("paif_bffusion_pack_ops", _p(new_hi), M, K - cut, cut, M, K, 9, 0, _p(cv.fwd))
    weff = torch.cat([w[:, :cut], w2[:, cut:]], 1)

    def fn(dt):
        pre = _conv(x.to(dt), weff.to(dt), b.to(dt))
        return _lk(pre, 0.2), pre

    src, dst = _Map(B, H, W, K), _Map(B, H, W, M)
    src.put(0, x)
    ops._bff_conv(cv, src.up(), 0, dst.up(), 0, B, H, W)
    _value("bff repack @ 48x32 2x19x35", dst.get(0, M), fn)


# ---------------------------------------------------------------------------------------------
# shared runners of the per-network entry points
# ---------------------------------------------------------------------------------------------
def _run_fwd(name, call, maps, out, out_slice, fn, B, H, W, extra=()):
    """maps: {key: _Map}; call(dev) launches on the uploaded maps; out: key of the written map, out_slice its (off, n);
    extra: [(key, off, n, fn)] further written slices.  Everything else must stay as uploaded."""
    def run():
        ms = maps()
        call({k: m.up() for k, m in ms.items()})
        return ms

    ms = run()
    written = {out: [out_slice]}
    _value(name, ms[out].get(*out_slice), fn)
    for key, off, n, f in extra:
        _value("%s %s" % (name, key), ms[key].get(off, n), f)
        written.setdefault(key, []).append((off, n))
    for k, m in ms.items():
        m.rest("%s %s" % (name, k), written.get(k, ()))
    if (B, H, W) in TWICE:
        again = run()
        for k in written:
            _bits("%s %s twice" % (name, k), again[k], ms[k])


def _convs(spec, g):
    """[(cout, cin, k, has_bias)] -> [(w, b or None)] CPU fp32: randn / sqrt(fan_in), randn."""
    return [(_randn(g, co, ci, k, k) / math.sqrt(ci * k * k), _randn(g, co) if hb else None) for co, ci, k, hb in spec]


def _dev_convs(convs):
    return [(_d(w), None if b is None else _d(b)) for w, b in convs]


# ---------------------------------------------------------------------------------------------
# U2Fusion: channel counts that are no multiple of 16, in place in the 264-wide slab; head32 with tanh
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def u2():
    convs = _convs([(co, ci, 3, True) for _, co, ci in synthetic.U2FUSION_CONVS], _gen(1, base=BASE))
    return convs, ops.u2fusion_pack(_dev_convs(convs))


U2_IN_C = {6: 264, 7: 128, 8: 64}


def _u2_fwd(u2, layer, B, H, W):
    convs, pack = u2
    w, b = convs[layer]
    cout, cin = w.shape[:2]
    g = _gen(100, layer, B, H, W, base=BASE)
    x = _randn(g, B, cin, H, W)
    name = "u2 3x3 EPI_ACT layer %d (%d -> %d) @ %s" % (layer, cin, cout, _tag(B, H, W))

    def fn(dt):
        pre = _conv(x.to(dt), w.to(dt), b.to(dt))
        return _lk(pre, 0.2), pre

    if layer <= 5:      # in place: the slice being written, and everything above it, starts as NaN
        maps = lambda: {"cat": _Map(B, H, W, 264).put(0, x)}
        call = lambda d: _call("paif_u2fusion_conv_fwd", _p(pack), layer, _p(d["cat"]), _p(d["cat"]), B, H, W)
        _run_fwd(name, call, maps, "cat", (cin, cout), fn, B, H, W)
    else:
        maps = lambda: {"in": _Map(B, H, W, U2_IN_C[layer]).put(0, x), "out": _Map(B, H, W, cout)}
        call = lambda d: _call("paif_u2fusion_conv_fwd", _p(pack), layer, _p(d["in"]), _p(d["out"]), B, H, W)
        _run_fwd(name, call, maps, "out", (0, cout), fn, B, H, W)


def _u2_bwd(u2, layer, B, H, W, hot=None):
    convs, pack = u2
    w = convs[layer][0]
    cout, cin = w.shape[:2]
    g = _gen(101, layer, B, H, W, base=BASE)
    t, plants = _tape(g, B, cout, H, W)
    cot = _cot(g, (B, cout, H, W), plants, hot)
    prior = _randn(g, B, cin, H, W)
    dense = layer <= 5
    name = "u2 3x3 MASK %s layer %d (%d -> %d)%s @ %s" % ("EPI_ADD" if dense else "EPI_STORE", layer, cout, cin, "" if hot is None else " one-hot %d" % hot,
                                                         _tag(B, H, W))

    def fn(dt):
        s = _conv_t(cot.to(dt) * _dlk(t.to(dt), 0.2), w.to(dt))
        return (s + prior.to(dt), s) if dense else (s, s)

    if dense:
        maps = lambda: {"tape": _Map(B, H, W, 264).put(cin, t), "d_cat": _Map(B, H, W, 264).put(0, prior).put(cin, cot)}
        call = lambda d: _call("paif_u2fusion_conv_bwd", _p(pack), layer, _p(d["tape"]), _p(d["d_cat"]), _p(d["d_cat"]), B, H, W)
        _run_fwd(name, call, maps, "d_cat", (0, cin), fn, B, H, W)
    else:
        maps = lambda: {"tape": _Map(B, H, W, cout).put(0, t), "d_out": _Map(B, H, W, cout).put(0, cot), "d_in": _Map(B, H, W, U2_IN_C[layer])}
        call = lambda d: _call("paif_u2fusion_conv_bwd", _p(pack), layer, _p(d["tape"]), _p(d["d_out"]), _p(d["d_in"]), B, H, W)
        _run_fwd(name, call, maps, "d_in", (0, cin), fn, B, H, W)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("layer", range(1, 9))
def test_u2_layer_forward(u2, layer, B, H, W):
    _u2_fwd(u2, layer, B, H, W)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("layer", range(1, 9))
def test_u2_layer_reverse(u2, layer, B, H, W):
    _u2_bwd(u2, layer, B, H, W)


@pytest.mark.parametrize("layer", [1, 3, 7])
@pytest.mark.parametrize("hot", [0, 1, 2, 3])
def test_u2_zero_tape_one_hot(u2, layer, hot):
    _u2_bwd(u2, layer, 2, 19, 35, hot=hot)


def _head(name, fwd_call, bwd_call, w, b, act, dact, B, H, W, g, hot=None, tanh=False):
    """head32_fwd_k / head32_bwd_k: 3 x 3, 32 -> 1, bias, activation; the reverse reads the branch off the taped plane."""
    x = _randn(g, B, 32, H, W)
    t, plants = _tape(g, B, 1, H, W, tanh=tanh)
    cot = _cot(g, (B, 1, H, W), plants, hot)

    def ffn(dt):
        pre = _conv(x.to(dt), w.to(dt), b.to(dt))
        return act(pre), pre

    def bfn(dt):
        s = _conv_t(cot.to(dt) * dact(t.to(dt)), w.to(dt))
        return s, s

    if hot is None:
        _run_fwd(name % "fwd", lambda d: fwd_call(d["in"], d["out"]), lambda: {"in": _Map(B, H, W, 32).put(0, x), "out": _Map(B, H, W, 1)}, "out", (0, 1),
                 ffn, B, H, W)
    _run_fwd((name % "bwd") + ("" if hot is None else " one-hot %d" % hot), lambda d: bwd_call(d["tape"], d["g"], d["d_in"]),
             lambda: {"tape": _Map(B, H, W, 1).put(0, t), "g": _Map(B, H, W, 1).put(0, cot), "d_in": _Map(B, H, W, 32)}, "d_in", (0, 32), bfn, B, H, W)
    return t, plants


def _u2_head(u2, B, H, W, hot=None):
    convs, pack = u2
    w, b = convs[9]
    return _head("u2 head32_%s_k<ACT_TANH> @ " + _tag(B, H, W),
                 lambda i, o: _call("paif_u2fusion_head_fwd", _p(pack), _p(i), _p(o), B, H, W),
                 lambda t, g, o: _call("paif_u2fusion_head_bwd", _p(pack), _p(t), _p(g), _p(o), B, H, W),
                 w, b, torch.tanh, lambda t: (1 - t) * (1 + t), B, H, W, _gen(102, B, H, W, base=BASE), hot, tanh=True)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
def test_u2_head(u2, B, H, W):
    _u2_head(u2, B, H, W)


@pytest.mark.parametrize("hot", range(6))
def test_u2_head_one_hot(u2, hot):
    """On a planted +-1.0 of the taped tanh plane the cotangent contributes exactly 0; on a planted zero all of it."""
    _u2_head(u2, 2, 19, 35, hot=hot)


# ---------------------------------------------------------------------------------------------
# DRDB: dilation 2, the residual epilogue, the five-group 1 x 1 with the mask at its own stride, head32 with LeakyReLU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def drdb():
    convs = _convs([(co, ci, k, True) for _, co, ci, k in synthetic.DRDB_CONVS], _gen(2, base=BASE))
    return convs, ops.drdb_pack(_dev_convs(convs), 0.25).weights


@pytest.mark.parametrize("B,H,W", DIL, ids=lambda s: str(s))
@pytest.mark.parametrize("k", range(1, 6))
def test_drdb_dcov_forward(drdb, k, B, H, W):
    convs, pack = drdb
    block = k & 1
    w, b = convs[1 + 6 * block + k - 1]
    cin = w.shape[1]
    x = _randn(_gen(200, k, B, H, W, base=BASE), B, cin, H, W)

    def fn(dt):
        pre = _conv(x.to(dt), w.to(dt), b.to(dt), dil=2)
        return _lk(pre, 0.0), pre

    _run_fwd("drdb dil2 EPI_ACT Dcov%d (%d -> 32) @ %s" % (k, cin, _tag(B, H, W)),
             lambda d: _call("paif_drdb_dcov_fwd", _p(pack), block, k, _p(d["slab"]), B, H, W), lambda: {"slab": _Map(B, H, W, 224).put(0, x)},
             "slab", (cin, 32), fn, B, H, W)


def _drdb_dcov_bwd(drdb, k, B, H, W, hot=None):
    convs, pack = drdb
    block = k & 1
    w = convs[1 + 6 * block + k - 1][0]
    cin = w.shape[1]
    g = _gen(201, k, B, H, W, base=BASE)
    t, plants = _tape(g, B, 32, H, W)
    cot, prior = _cot(g, (B, 32, H, W), plants, hot), _randn(g, B, cin, H, W)

    def fn(dt):
        s = _conv_t(cot.to(dt) * _dlk(t.to(dt), 0.0), w.to(dt), dil=2)
        return s + prior.to(dt), s

    _run_fwd("drdb dil2 MASK EPI_ADD Dcov%d (32 -> %d)%s @ %s" % (k, cin, "" if hot is None else " one-hot %d" % hot, _tag(B, H, W)),
             lambda d: _call("paif_drdb_dcov_bwd", _p(pack), block, k, _p(d["tape"]), _p(d["d_slab"]), B, H, W),
             lambda: {"tape": _Map(B, H, W, 224).put(cin, t), "d_slab": _Map(B, H, W, 224).put(0, prior).put(cin, cot)}, "d_slab", (0, cin), fn, B, H, W)


@pytest.mark.parametrize("B,H,W", DIL, ids=lambda s: str(s))
@pytest.mark.parametrize("k", range(1, 6))
def test_drdb_dcov_reverse(drdb, k, B, H, W):
    _drdb_dcov_bwd(drdb, k, B, H, W)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("block,out_cs", [(0, 224), (1, 64)])
def test_drdb_tail_forward(drdb, block, out_cs, B, H, W):
    """1 x 1 EPI_RES: r6 = ReLU(conv + b), out = x + r6, both outputs."""
    convs, pack = drdb
    w, b = convs[1 + 6 * block + 5]
    x = _randn(_gen(202, block, B, H, W, base=BASE), B, 224, H, W)

    def r_fn(dt):
        pre = _conv(x.to(dt), w.to(dt), b.to(dt))
        return _lk(pre, 0.0), pre

    def fn(dt):
        r, pre = r_fn(dt)
        return x.to(dt)[:, :64] + r, pre

    _run_fwd("drdb 1x1 EPI_RES out_cs %d @ %s" % (out_cs, _tag(B, H, W)),
             lambda d: _call("paif_drdb_tail_fwd", _p(pack), block, _p(d["slab"]), _p(d["out"]), out_cs, _p(d["r6"]), B, H, W),
             lambda: {"slab": _Map(B, H, W, 224).put(0, x), "out": _Map(B, H, W, out_cs), "r6": _Map(B, H, W, 64)}, "out", (0, 64), fn, B, H, W,
             extra=[("r6", 0, 64, r_fn)])


def _drdb_tail_bwd(drdb, block, cs, B, H, W, hot=None):
    convs, pack = drdb
    w = convs[1 + 6 * block + 5][0]
    g = _gen(203, block, B, H, W, base=BASE)
    t, plants = _tape(g, B, 64, H, W)
    cot = _cot(g, (B, 64, H, W), plants, hot)

    def fn(dt):
        s = _conv_t(cot.to(dt) * _dlk(t.to(dt), 0.0), w.to(dt))
        r = s.clone()
        r[:, :64] += cot.to(dt)
        return r, s

    _run_fwd("drdb 1x1 MB3 XIN_SCALED + resid_add d_out_cs %d%s @ %s" % (cs, "" if hot is None else " one-hot %d" % hot, _tag(B, H, W)),
             lambda d: _call("paif_drdb_tail_bwd", _p(pack), block, _p(d["r6"]), _p(d["d_out"]), cs, _p(d["d_slab"]), B, H, W),
             lambda: {"r6": _Map(B, H, W, 64).put(0, t), "d_out": _Map(B, H, W, cs).put(0, cot), "d_slab": _Map(B, H, W, 224)}, "d_slab", (0, 224), fn,
             B, H, W)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("block,cs", [(0, 224), (1, 64)])
def test_drdb_tail_reverse(drdb, block, cs, B, H, W):
    _drdb_tail_bwd(drdb, block, cs, B, H, W)


def _drdb_conv2(drdb, slope, B, H, W, hot=None):
    convs, pack = drdb
    w, b = convs[13]
    g = _gen(204, int(slope * 100), B, H, W, base=BASE)
    x = _randn(g, B, 64, H, W)
    t, plants = _tape(g, B, 32, H, W)
    cot = _cot(g, (B, 32, H, W), plants, hot)

    def ffn(dt):
        pre = _conv(x.to(dt), w.to(dt), b.to(dt))
        return _lk(pre, slope), pre

    def bfn(dt):
        s = _conv_t(cot.to(dt) * _dlk(t.to(dt), slope), w.to(dt))
        return s, s

    tag = "slope %g%s @ %s" % (slope, "" if hot is None else " one-hot %d" % hot, _tag(B, H, W))
    if hot is None:
        _run_fwd("drdb conv2 3x3 EPI_ACT " + tag, lambda d: _call("paif_drdb_conv2_fwd", _p(pack), slope, _p(d["in"]), _p(d["c2"]), B, H, W),
                 lambda: {"in": _Map(B, H, W, 64).put(0, x), "c2": _Map(B, H, W, 32)}, "c2", (0, 32), ffn, B, H, W)
    _run_fwd("drdb conv2 3x3 MASK EPI_STORE " + tag,
             lambda d: _call("paif_drdb_conv2_bwd", _p(pack), slope, _p(d["tape"]), _p(d["g"]), _p(d["d_in"]), B, H, W),
             lambda: {"tape": _Map(B, H, W, 32).put(0, t), "g": _Map(B, H, W, 32).put(0, cot), "d_in": _Map(B, H, W, 64)}, "d_in", (0, 64), bfn, B, H, W)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("slope", [0.0, 0.25])
def test_drdb_conv2(drdb, slope, B, H, W):
    _drdb_conv2(drdb, slope, B, H, W)


def _drdb_head(drdb, slope, B, H, W, hot=None):
    convs, pack = drdb
    w, b = convs[14]
    return _head("drdb head32_%%s_k<ACT_LEAKY> slope %g @ %s" % (slope, _tag(B, H, W)),
                 lambda i, o: _call("paif_drdb_head_fwd", _p(pack), slope, _p(i), _p(o), B, H, W),
                 lambda t, g, o: _call("paif_drdb_head_bwd", _p(pack), slope, _p(t), _p(g), _p(o), B, H, W),
                 w, b, lambda v: _lk(v, slope), lambda t: _dlk(t, slope), B, H, W, _gen(205, int(slope * 100), B, H, W, base=BASE), hot)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("slope", [0.0, 0.25])
def test_drdb_head(drdb, slope, B, H, W):
    _drdb_head(drdb, slope, B, H, W)


@pytest.mark.parametrize("hot", [0, 1, 2, 3])
def test_drdb_zero_tape_one_hot(drdb, hot):
    """At slope 0 (ReLU) a planted zero passes nothing; at a positive slope, the slope."""
    _drdb_dcov_bwd(drdb, 3, 2, 19, 35, hot=hot)
    _drdb_tail_bwd(drdb, 0, 224, 2, 19, 35, hot=hot)
    for slope in (0.0, 0.25):
        _drdb_conv2(drdb, slope, 2, 19, 35, hot=hot)
        _drdb_head(drdb, slope, 2, 19, 35, hot=hot)


# ---------------------------------------------------------------------------------------------
# DIDFuse: the tanh epilogue, PAIR, XIN_SCALED with the tanh mask and the 0.5, XIN_SUM; BatchNorm folded on the device
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def did():
    """Non-trivial BatchNorm statistics; the float64 side folds them itself (and keeps the folded weights in float64), which also covers
    the device-side fold.  -> ({matrix-core layer: (folded weight, shift)}, the device pack)."""
    g = _gen(3, base=BASE)
    raw = []
    for _, _, co, ci, _ in synthetic.DIDFUSE_CONVS:
        w, b = _randn(g, co, ci, 3, 3) / math.sqrt(9 * ci), _randn(g, co)
        gamma, beta, mu, var = 0.5 + torch.rand(co, generator=g), _randn(g, co), _randn(g, co), 0.5 + torch.rand(co, generator=g)
        raw.append((w, b, gamma, beta, mu, var, 1e-3))
    pack = ops.didfuse_pack([tuple(_d(v) for v in c[:6]) + (c[6],) for c in raw], (0.1, 0.15, 0.2, 0.25, 0.3, 0.35)).weights

    def fold(i):
        w, b, gamma, beta, mu, var, eps = (v.double() if torch.is_tensor(v) else v for v in raw[i])
        sc = gamma / torch.sqrt(var + eps)
        return w * sc[:, None, None, None], beta + (b - mu) * sc

    layers = {}
    for s in range(2):
        layers[2 * s] = fold(4 * s + 1)
        (w3, b3), (w4, b4) = fold(4 * s + 2), fold(4 * s + 3)
        layers[2 * s + 1] = (torch.cat([w3, w4]), torch.cat([b3, b4]))
    layers[4], layers[5] = fold(8), fold(9)
    return layers, pack


DID_SLOPE = {0: 0.15, 2: 0.25, 4: 0.3, 5: 0.35}


@pytest.mark.parametrize("B,H,W", DID, ids=lambda s: str(s))
@pytest.mark.parametrize("layer", range(6))
def test_didfuse_forward(did, layer, B, H, W):
    layers, pack = did
    w, b = layers[layer]
    cout, cin = w.shape[:2]
    wide, paired, enc = layer < 4 and layer & 1, layer in (2, 3), layer < 4
    slope = 0.0 if wide else DID_SLOPE[layer]
    g = _gen(300, layer, B, H, W, base=BASE)
    x, u = _randn(g, B, cin, H, W), _randn(g, B, cout, H, W)
    ioff, ooff = (64 if wide else 0), (128 if wide else 64) if enc else 0
    aoff = 0 if wide else 64

    def fn(dt):
        pre = _conv(x.to(dt), w.to(dt), b.to(dt))
        return (torch.tanh(pre) if wide else _lk(pre, slope)), pre

    def avg_fn(dt):
        f, pre = fn(dt)
        return 0.5 * (u.to(dt) + f), pre

    def maps():
        m = {"in": _Map(B, H, W, 256 if enc else 128).put(ioff, x)}
        if not enc:
            m["out"] = _Map(B, H, W, 128)
        if paired:
            m["pair"], m["avg"] = _Map(B, H, W, 256).put(ooff, u), _Map(B, H, W, 128)
        return m

    def call(d):
        out = d["in"] if enc else d["out"]
        _call("paif_didfuse_conv_fwd", _p(pack), layer, slope, _p(d["in"]), _p(out), _p(d["pair"]) if paired else None, _p(d["avg"]) if paired else None,
              B, H, W)

    form = "3x3 %s%s" % ("ACT_TANH" if wide else "EPI_ACT", " PAIR" if paired else "")
    _run_fwd("did %s layer %d @ %s" % (form, layer, _tag(B, H, W)), call, maps, "in" if enc else "out", (ooff, cout), fn, B, H, W,
             extra=[("avg", aoff, cout, avg_fn)] if paired else ())


def _did_bwd(did, layer, B, H, W, hot=None):
    layers, pack = did
    w = layers[layer][0]
    cout, cin = w.shape[:2]
    cov34, cov2 = layer < 4 and layer & 1, layer < 4 and not layer & 1
    slope = 0.0 if cov34 else DID_SLOPE[layer]
    g = _gen(301, layer, B, H, W, base=BASE)
    t, plants = _tape(g, B, cout, H, W, tanh=bool(cov34))
    cot, skip = _cot(g, (B, cout, H, W), plants, hot), _randn(g, B, cout, H, W)
    if hot is not None:
        skip = torch.zeros_like(skip)
        if cov2 and hot % 2:     # the second input alone carries the cotangent
            cot, skip = skip, 2 * cot

    def fn(dt):
        c, tt = cot.to(dt), t.to(dt)
        dz = 0.5 * c * ((1 - tt) * (1 + tt)) if cov34 else ((c + 0.5 * skip.to(dt)) if cov2 else c) * _dlk(tt, slope)
        s = _conv_t(dz, w.to(dt))
        return s, s

    h = "" if hot is None else " one-hot %d" % hot
    if cov34:
        name, out = "did 3x3 MASK XIN_SCALED tanh layer %d%s @ %s" % (layer, h, _tag(B, H, W)), ("d_in", (64, 64))
        maps = lambda: {"tape": _Map(B, H, W, 256).put(128, t), "d_out": _Map(B, H, W, 128).put(0, cot), "d_in": _Map(B, H, W, 128)}
        call = lambda d: _call("paif_didfuse_conv_bwd", _p(pack), layer, slope, _p(d["tape"]), _p(d["d_out"]), _p(d["d_in"]), None, B, H, W)
    elif cov2:
        name, out = "did 3x3 MASK XIN_SUM layer %d%s @ %s" % (layer, h, _tag(B, H, W)), ("dg", (0, 64))
        maps = lambda: {"tape": _Map(B, H, W, 256).put(64, t), "dg": _Map(B, H, W, 128).put(64, cot), "skip": _Map(B, H, W, 128).put(64, skip)}
        call = lambda d: _call("paif_didfuse_conv_bwd", _p(pack), layer, slope, _p(d["tape"]), _p(d["dg"]), _p(d["dg"]), _p(d["skip"]), B, H, W)
    else:
        name, out = "did 3x3 MASK EPI_STORE layer %d%s @ %s" % (layer, h, _tag(B, H, W)), ("d_in", (0, 128))
        maps = lambda: {"tape": _Map(B, H, W, 128).put(0, t), "d_out": _Map(B, H, W, 128).put(0, cot), "d_in": _Map(B, H, W, 128)}
        call = lambda d: _call("paif_didfuse_conv_bwd", _p(pack), layer, slope, _p(d["tape"]), _p(d["d_out"]), _p(d["d_in"]), None, B, H, W)
    _run_fwd(name, call, maps, out[0], out[1], fn, B, H, W)
    return fn


@pytest.mark.parametrize("B,H,W", DID, ids=lambda s: str(s))
@pytest.mark.parametrize("layer", range(6))
def test_didfuse_reverse(did, layer, B, H, W):
    _did_bwd(did, layer, B, H, W)


@pytest.mark.parametrize("layer", [1, 2, 5])
@pytest.mark.parametrize("hot", range(6))
def test_didfuse_one_hot(did, layer, hot):
    """Planted zeros take the PReLU slope; planted +-1.0 of the tanh tape (hot 4, 5 of layer 1) give exactly zero."""
    fn = _did_bwd(did, layer, 2, 19, 35, hot=hot)
    if layer == 1 and hot >= 4:
        assert float(fn(torch.float64)[0].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------
# SeAFusion: two biases over a pack filled from two weights side by side
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sea():
    convs = _convs([(co, ci, k, hb) for _, co, ci, k, hb in synthetic.SEAFUSION_CONVS], _gen(4, base=BASE))
    return convs, ops.seafusion_pack(_dev_convs(convs))


def _sea_tail(sea, block):
    """-> ([convdown | convup] weight [cout][4C][1][1], the two biases, C, cout, the stride and offset of the block's output)."""
    convs, _ = sea
    base = 13 * (block >> 1) + 1 + 6 * (block & 1)
    (wd, bd), (wu, bu) = convs[base + 2], convs[base + 5]
    C = wu.shape[1]
    assert wd.shape[1] == 3 * C and wd.shape[-1] == 1
    return torch.cat([wd, wu], 1), bd, bu, C, wd.shape[0], (96 if block & 1 else 128), (48 * (block >> 1) if block & 1 else 0)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("block", range(4))
def test_seafusion_tail_forward(sea, block, B, H, W):
    w, bd, bu, C, cout, cs, off = _sea_tail(sea, block)
    x = _randn(_gen(400, block, B, H, W, base=BASE), B, 4 * C, H, W)

    def fn(dt):
        pre = _conv(x.to(dt), w.to(dt), bd.to(dt) + bu.to(dt))
        return _lk(pre, 0.1), pre

    _run_fwd("sea 1x1 EPI_ACT bias2 block %d (%d -> %d) @ %s" % (block, 4 * C, cout, _tag(B, H, W)),
             lambda d: _call("paif_seafusion_tail_fwd", _p(sea[1]), block, _p(d["slab"]), _p(d["out"]), B, H, W),
             lambda: {"slab": _Map(B, H, W, 4 * C).put(0, x), "out": _Map(B, H, W, cs)}, "out", (off, cout), fn, B, H, W)


def _sea_tail_bwd(sea, block, B, H, W, hot=None):
    w, _, _, C, cout, cs, off = _sea_tail(sea, block)
    g = _gen(401, block, B, H, W, base=BASE)
    t, plants = _tape(g, B, cout, H, W)
    cot = _cot(g, (B, cout, H, W), plants, hot)

    def fn(dt):
        s = _conv_t(cot.to(dt) * _dlk(t.to(dt), 0.1), w.to(dt))
        return s, s

    _run_fwd("sea 1x1 MASK EPI_STORE block %d (%d -> %d)%s @ %s" % (block, cout, 4 * C, "" if hot is None else " one-hot %d" % hot, _tag(B, H, W)),
             lambda d: _call("paif_seafusion_tail_bwd", _p(sea[1]), block, _p(d["tape"]), _p(d["d_out"]), _p(d["d_slab"]), B, H, W),
             lambda: {"tape": _Map(B, H, W, cs).put(off, t), "d_out": _Map(B, H, W, cs).put(off, cot), "d_slab": _Map(B, H, W, 4 * C)}, "d_slab",
             (0, 4 * C), fn, B, H, W)


@pytest.mark.parametrize("B,H,W", ZP, ids=lambda s: str(s))
@pytest.mark.parametrize("block", range(4))
def test_seafusion_tail_reverse(sea, block, B, H, W):
    _sea_tail_bwd(sea, block, B, H, W)


@pytest.mark.parametrize("hot", [0, 1, 2, 3])
def test_seafusion_zero_tape_one_hot(sea, hot):
    _sea_tail_bwd(sea, 3, 2, 19, 35, hot=hot)
