#!/usr/bin/env python3
"""SHA-256 digests of the raw output bytes of the LDS-DMA convs, case by case, with the loaded library (PAIF_LIB= selects a build).

    PAIF_LIB=<library of the commit to pin> python3 tools/conv_epilogue_digests.py tests/golden/conv_epilogue_digests.json [per-launch.json]

writes the fixture that tests/test_conv_swap_epilogue_gpu.py recomputes with the product library: a change of the epilogue that only
moves data (the half-wave swap in place of the LDS park, conv_rows.h) must leave every digest as it was.  One digest per case: the
SHA-256 over the digests of the case's launches in order; the optional second file keeps the launches apart (to compare two builds by
hand).  The test imports the case lists and the runners from this file, so fixture and test cannot drift apart.

Cases (inputs seeded on the CPU, tests/kernel_check.gen; every output is written into the middle of a (B + 2)-image buffer of
sentinels, whose guard images must come back untouched):
  tile   conv3x3_h16_dma / conv7x7_h16_dma through ops.conv2d at the smallest shapes that reach 1,024 tiles and put every edge on the
         per-pixel output masks: 1023x9x1, 1023x1x33, 120x17x95 (W mod 32 = 31), 130x30x49 (17), 1x250x1030 (6, B = 1).  Forms:
         (sources, residual maps) in (1,0) (1,1) (2,0) (2,2) (3,1) (3,3), (1,0) with 16 output channels, the dilation-2 ReLU-input
         forms with 1 and 3 residual maps, 7x7; each with activation none / PReLU / ReLU x with / without scale and shift, alpha
         0.5 / 1 / 1.5 by turns, both walk directions, fp16 and bf16; the fused-ChannelPool forms (map and pool plane).
  rows   conv3x3_h16_dma_rows (PAIF_CONV_DMA_ROWS=1), 0-3 residual maps, 16-bit and fp32 output, at 1x1x1, 1x2x33, 1x5x31, 2x7x70,
         3x37x53, 1x400x33, 2x64x96.
  eca    paif_eca_conv2_gated_fwd_f16 (the entry behind ops.eca_block_tail, PAIF_ECA_ROWS=1): pool partials, gate and output.
  1x1    conv_h16_dma_1x1 at 1023x9x1, 512x8x64, 2x333x517, its four epilogue variants.
  net    Network_Fusion_Searched under fp16 storage at 1x97x131 and 2x64x96: the fused image.
"""
import ctypes
import functools
import hashlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from paif_amd import _lib, ops  # noqa: E402
from tests.kernel_check import gen  # noqa: E402

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FMTS = [F16, BF16]
NAME = {BF16: "bf16", F16: "f16"}
FCODE = {BF16: 1, F16: 2}
SENTINEL = 0x5A5B
BASE = 131                                   # this module's generator stream

TILE_SHAPES = [(1023, 9, 1), (1023, 1, 33), (120, 17, 95), (130, 30, 49), (1, 250, 1030)]
ROW_SHAPES = [(1, 1, 1), (1, 2, 33), (1, 5, 31), (2, 7, 70), (3, 37, 53), (1, 400, 33), (2, 64, 96)]
RUNS_1X1 = [(1023, 9, 1), (512, 8, 64), (2, 333, 517)]
NET_SHAPES = [(1, 97, 131), (2, 64, 96)]
# (kh, dil, nsrc, nres, cout, in_act, pool): the tile forms
D1 = [(3, 1, 1, 0, 32, 0, None), (3, 1, 1, 1, 32, 0, None), (3, 1, 2, 0, 32, 0, None), (3, 1, 2, 2, 32, 0, None), (3, 1, 3, 1, 32, 0, None),
      (3, 1, 3, 3, 32, 0, None), (3, 1, 1, 0, 16, 0, None)]
D2 = [(3, 2, 1, 1, 32, 2, None), (3, 2, 1, 3, 32, 2, None)]
K7 = [(7, 1, 1, 0, 32, 0, None)]
POOLED = [(3, 1, 3, 1, 32, 0, 0), (3, 1, 3, 3, 32, 0, 2), (3, 2, 1, 1, 32, 2, 0), (3, 2, 1, 3, 32, 2, 2)]
TILE_FORMS = D1 + D2 + K7 + POOLED
# (act, affine, alpha): every activation with and without scale / shift; alpha by turns
VARIANTS = [(0, False, 1.0), (1, False, 0.5), (2, False, 1.5), (0, True, 0.5), (1, True, 1.5), (2, True, 1.0)]
K7_VARIANTS = [(0, False, 1.0), (1, True, 0.5)]
EPI_1X1 = [(0, False), (1, True), (2, True), (0, True)]
ECA_SLOPES = [0.25, 0.1]


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def sha(*tensors):
    h = hashlib.sha256()
    for x in tensors:
        h.update(x.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=8)
def cpu_map(shape, dt, idx):
    """Map `idx` of a shape (0-2 sources, 3-5 residual maps) as CPU fp32 values of the format."""
    B, H, W = shape
    return torch.randn(B, H, W, 32, generator=gen(B, H, W, FCODE[dt], idx, base=BASE)).to(dt).float()


@functools.lru_cache(maxsize=8)
def dev_map(shape, dt, idx):
    return cpu_map(shape, dt, idx).to(dev()).to(dt).contiguous()


@functools.lru_cache(maxsize=None)
def params(dt, kh, nsrc, cout):
    g = gen(FCODE[dt], kh, nsrc, cout, base=BASE)
    w = (torch.randn(cout, 32 * nsrc, kh, kh, generator=g) * (0.02 if kh == 7 else 0.05)).to(dt).float()
    return w, torch.rand(32, generator=g) + 0.5, torch.randn(32, generator=g) * 0.1


def guarded(B, H, W, C, dt):
    big = torch.empty((B + 2, H, W, C), device=dev(), dtype=dt)
    big.view(torch.int16).fill_(SENTINEL)
    return big


def guards_intact(big):
    B = big.shape[0] - 2
    v = big.view(torch.int16)
    return bool((v[0] == SENTINEL).all()) and bool((v[B + 1] == SENTINEL).all())


def conv_launch(shape, dt, form, variant, reverse, out_f32=False):
    """One ops.conv2d call: (output, pool plane or None, guards intact)."""
    kh, dil, nsrc, nres, cout, in_act, pool = form
    act, affine, alpha = variant
    B, H, W = shape
    d = dev()
    w, scale, shift = params(dt, kh, nsrc, cout)
    srcs = [dev_map(shape, dt, i) for i in range(nsrc)]
    res = [dev_map(shape, dt, 3 + i) for i in range(nres)]
    ops.set_storage(NAME[dt])
    wpk = ops.pack_conv_weight(w.to(d), nsrc, 32, kh, precision="f16" if dt is F16 else "bf16x3")
    big = guarded(B, H, W, cout, F32 if out_f32 else dt)
    comp = torch.full((B, H, W, 4), float("nan"), device=d) if pool is not None else None
    ops._SERP[0] = reverse ^ 1                          # conv2d flips it: this launch gets reverse_tiles = reverse
    out = ops.conv2d(srcs, wpk, kh, dil=dil, cout=cout, in_act=in_act, scale=scale.to(d) if affine else None,
                     shift=shift.to(d) if affine else None, act=act, prelu=torch.tensor([0.2], device=d) if act == 1 else None, alpha=alpha,
                     res=tuple(res), out_f32=out_f32, out=big[1:B + 1], cpool=None if comp is None else (comp, pool))
    torch.cuda.synchronize()
    return out, (None if comp is None else comp[..., pool:pool + 2]), guards_intact(big)


def kernel_name(shape, dt, form, out_f32=False):
    kh, dil, nsrc, nres, cout, in_act, pool = form
    d = _lib.ConvDesc()
    one = ctypes.c_void_p(16)
    for i in range(3):
        d.src[i] = one if i < nsrc else None
        d.res[i] = one if i < nres else None
    d.wpk, d.out = one, one
    d.nsrc, d.cin, d.cout, d.kh, d.dil, d.alpha, d.in_act = nsrc, 32, cout, kh, dil, 0.5, in_act
    d.storage, d.precision = ((4 if out_f32 else 3), 4) if dt is F16 else (1, ops.PREC_BF16)
    if pool is not None:
        d.cpool = one
    return ops.conv2d_kernel_name(d, *shape)


def form_id(form):
    kh, dil, nsrc, nres, cout, in_act, pool = form
    return "k%dd%d-s%dr%d" % (kh, dil, nsrc, nres) + ("-c16" if cout == 16 else "") + ("-in%d" % in_act if in_act else "") + \
        ("-pool%d" % pool if pool is not None else "")


def variants_of(form):
    if form[0] == 7:
        return K7_VARIANTS
    return VARIANTS[1::2] if form[6] is not None else VARIANTS       # pooled forms: unchanged code, three variants


def tile_case(shape, dt, form):
    """{key: digest} of one (shape, format, form): every variant in both walk directions; a broken guard image poisons the digest."""
    out = {}
    for variant in variants_of(form):
        for reverse in (0, 1):
            o, comp, ok = conv_launch(shape, dt, form, variant, reverse)
            key = "tile/%dx%dx%d/%s/%s/a%d-%s-alpha%g/rev%d" % (shape + (NAME[dt], form_id(form), variant[0], "aff" if variant[1] else "noaff",
                                                                          variant[2], reverse))
            out[key] = sha(o) if ok else "guard image overwritten"
            if comp is not None:
                out[key + "/pool"] = sha(comp)
    return out


def rows_case(shape, dt, nres, out_f32):
    out = {}
    form = (3, 2, 1, nres, 32, 0, None)
    for variant in VARIANTS[nres % 2::2]:
        for reverse in (0, 1):
            o, _, ok = conv_launch(shape, dt, form, variant, reverse, out_f32=out_f32)
            key = "rows/%dx%dx%d/%s/r%d%s/a%d-%s-alpha%g/rev%d" % (shape + (NAME[dt], nres, "-f32" if out_f32 else "", variant[0],
                                                                          "aff" if variant[1] else "noaff", variant[2], reverse))
            out[key] = sha(o) if ok else "guard image overwritten"
    return out


def one_by_one_case(shape, dt):
    out = {}
    form = (1, 1, 3, 0, 32, 0, None)
    for act, affine in EPI_1X1:
        o, _, ok = conv_launch(shape, dt, form, (act, affine, 0.5), 0)
        out["1x1/%dx%dx%d/%s/a%d-%s" % (shape + (NAME[dt], act, "aff" if affine else "noaff"))] = sha(o) if ok else "guard image overwritten"
    return out


def eca_case(shape):
    """paif_eca_conv2_gated_fwd_f16: pool partials, gate, out."""
    B, H, W = shape
    d = dev()
    out = {}
    ops.set_storage("f16")
    g = gen(3, base=BASE)
    w = (torch.randn(32, 32, 3, 3, generator=g) * 0.05).to(F16).float()
    w1d = torch.randn(1, 1, 3, generator=g).to(d)
    wpk = ops.pack_conv_weight(w.to(d), 1, 32, 3, precision="f16")
    r = dev_map(shape, F16, 0)
    L = ops.lib()
    assert L.paif_eca_conv2_gated_fits(B, H, W) == 1
    nt = L.paif_conv2d_blocks(B, H, W) * 32
    for a in ECA_SLOPES:
        sl = torch.tensor([a], dtype=F32, device=d)
        partial, gate = torch.zeros(nt, dtype=F32, device=d), torch.zeros(B * 32, dtype=F32, device=d)
        big = guarded(B, H, W, 32, F16)
        _lib.check(L.paif_eca_conv2_gated_fwd_f16(ops._pa(r), ops._p(wpk.data), ops._p(sl), ops._p(partial), ops._p(w1d.contiguous()), 3, ops._p(sl),
                                                  ops._p(gate), ops._pa(big[1:B + 1]), B, H, W, ops._stream()), "eca_conv2_gated")
        torch.cuda.synchronize()
        key = "eca/%dx%dx%d/slope%g/" % (shape + (a,))
        ok = guards_intact(big)
        out[key + "pool"], out[key + "gate"] = sha(partial), sha(gate)
        out[key + "out"] = sha(big[1:B + 1]) if ok else "guard image overwritten"
    return out


def net_case(shape):
    from paif_amd import synthetic as S
    from paif_amd.core.model_fusion_auto import Network_Fusion_Searched
    from paif_amd.genotypes import FUSION_AT
    from tests.helpers import t

    ops.set_storage("f16")
    net = Network_Fusion_Searched(32, None, FUSION_AT).eval()
    net.load_state_dict({k: t(S.formula_tensor("enhance_net." + k, tuple(v.shape))).to(v.dtype) for k, v in net.state_dict().items()}, strict=True)
    net = net.to(dev())
    ir, vis, _ = S.make_batch(*shape)
    with torch.no_grad():
        out = net(t(ir).to(dev()), ops.rgb2ycrcb(t(vis).to(dev())))
    torch.cuda.synchronize()
    return {"net/%dx%dx%d/fused" % shape: sha(out)}


def case_digest(launches):
    """One SHA-256 per case over its launches {key: digest}."""
    return hashlib.sha256("\n".join("%s %s" % kv for kv in sorted(launches.items())).encode()).hexdigest()


def case_list():
    """(id, runner, environment) of every case, in the order that reuses the cached maps."""
    rows_env, eca_env = {"PAIF_CONV_DMA_ROWS": "1"}, {"PAIF_ECA_ROWS": "1"}
    out = []
    for dt in FMTS:
        for shape in TILE_SHAPES:
            for form in TILE_FORMS:
                out.append(("tile-%dx%dx%d-%s-%s" % (shape + (NAME[dt], form_id(form))), functools.partial(tile_case, shape, dt, form), {}))
        for shape in ROW_SHAPES:
            for nres in range(4):
                out.append(("rows-%dx%dx%d-%s-r%d" % (shape + (NAME[dt], nres)), functools.partial(rows_case, shape, dt, nres, False), rows_env))
                if dt is F16:
                    out.append(("rows-%dx%dx%d-f16-r%d-f32" % (shape + (nres,)), functools.partial(rows_case, shape, dt, nres, True), rows_env))
        for shape in RUNS_1X1:
            out.append(("1x1-%dx%dx%d-%s" % (shape + (NAME[dt],)), functools.partial(one_by_one_case, shape, dt), {}))
    for shape in ROW_SHAPES:
        out.append(("eca-%dx%dx%d" % shape, functools.partial(eca_case, shape), eca_env))
    for shape in NET_SHAPES:
        out.append(("net-%dx%dx%d" % shape, functools.partial(net_case, shape), eca_env))
    return out


def run_case(runner, env):
    """Run one case under its environment switches (the dispatchers read them per call) and the suite's default arithmetic."""
    old_env = {k: os.environ.get(k) for k in env}
    old_cfg, serp = dict(ops.CONFIG), ops._SERP[0]
    os.environ.update(env)
    ops.set_conv_precision("bf16x3")
    try:
        return runner()
    finally:
        ops.set_storage("f32")
        ops.CONFIG.update(old_cfg)
        ops._SERP[0] = serp
        ops._ACT_BF16[0] = False
        ops._TWINS.clear()
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def main():
    path = sys.argv[1]
    digests, launches = {}, {}
    for cid, runner, env in case_list():
        got = run_case(runner, env)
        digests[cid] = case_digest(got)
        launches.update(got)
        print(cid, len(got), digests[cid][:16], flush=True)
    rec = {"_note": "tools/conv_epilogue_digests.py: SHA-256 of the raw output bytes per case, computed with the library of _commit",
           "_commit": os.environ.get("PAIF_DIGEST_COMMIT", ""), "_library": os.path.basename(_lib.LIB_PATH), "cases": digests}
    with open(path, "w") as f:
        json.dump(rec, f, indent=0, sort_keys=True)
        f.write("\n")
    if len(sys.argv) > 2:
        with open(sys.argv[2], "w") as f:
            json.dump(launches, f, indent=0, sort_keys=True)
    print("wrote %s: %d cases, %d launches" % (path, len(digests), len(launches)))


if __name__ == "__main__":
    main()
