"""The LDS-DMA convs must compute the bits they computed before their epilogue changed (csrc/conv_rows.h: the half-wave swap in place of
the LDS park, on pixel-per-lane accumulators).

tests/golden/conv_epilogue_digests.json holds one SHA-256 per case, written by tools/conv_epilogue_digests.py on an MI355X with the
library of the commit in front of that change (`_commit` in the file).  Each test recomputes the digest of its case with the product
library -- the case lists, the seeded inputs and the runners are the tool's own, imported from it -- and compares.  A case is one
(shape, format, form) with all its epilogue variants in both walk directions; every output is written into the middle of a (B + 2)-image
buffer of sentinels, and an overwritten guard image changes the digest.

Shapes of the tile kernels (8 x 32 tiles, eligible from 1,024 tiles): the smallest that reach the threshold and put every edge on the
per-pixel output masks of the swap epilogue -- 1023x9x1 (one column, a one-row second tile row), 1023x1x33 (H = 1, second strip one
column wide), 120x17x95 (W mod 32 = 31), 130x30x49 (17), 1x250x1030 (6, one image).  The row kernels, the ECA tail and the streaming 1x1
run at the small shapes of their own test files with their switches forced on; the whole forward at 1x97x131 and 2x64x96.

On a mismatch a conv case is run again, launch by launch, against the float64 restatement of tests/test_dense_conv16_gpu.py (F.conv2d over
the concatenated sources, then act(scale * z + shift) * alpha + sum(res)), and the first element outside the `h16` / `rev` bound of
tests/kernel_check.py is reported as (launch, image, row, column, channel)."""
import importlib.util
import json
import os

import pytest
import torch
import torch.nn.functional as F

from tests.kernel_check import REV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("conv_epilogue_digests", os.path.join(ROOT, "tools", "conv_epilogue_digests.py"))
D = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(D)

FIXTURE = json.load(open(os.path.join(ROOT, "tests", "golden", "conv_epilogue_digests.json")))
CASES = D.case_list()
EPS16 = {D.BF16: 2.0 ** -8, D.F16: 2.0 ** -11}


def _first_bad(shape, dt, form, variants, out_f32=False):
    """Run every launch of a conv case against float64; the first element outside its bound, or None."""
    kh, dil, nsrc, nres, cout, in_act, pool = form
    w, scale, shift = D.params(dt, kh, nsrc, cout)
    x = torch.cat([D.cpu_map(shape, dt, i) for i in range(nsrc)], dim=-1).permute(0, 3, 1, 2).double()
    if in_act == 2:
        x = x.clamp_min(0)
    z = F.conv2d(x, w.double(), None, 1, dil * (kh - 1) // 2, dil).permute(0, 2, 3, 1).contiguous()
    for variant in variants:
        act, affine, alpha = variant
        v = z
        if affine:
            v = v * scale[:cout].double() + shift[:cout].double()
        if act == 1:
            v = torch.where(v >= 0, v, v * torch.tensor([0.2]).double())          # the slope as the kernel holds it: fp32(0.2)
        elif act == 2:
            v = v.clamp_min(0)
        v = v * alpha
        for i in range(nres):
            v = v + D.cpu_map(shape, dt, 3 + i).double()
        b32 = REV * float(v.abs().max())
        tol = b32 + (0 if out_f32 else 1.01 * EPS16[dt]) * v.abs()
        for reverse in (0, 1):
            got, _, ok = D.conv_launch(shape, dt, form, variant, reverse, out_f32=out_f32)
            if not ok:
                return "a%d affine=%s alpha=%g reverse=%d: a guard image was overwritten" % (act, affine, alpha, reverse)
            bad = ((got.cpu().double() - v).abs() > tol).nonzero()
            if len(bad):
                b, y, xx, c = (int(i) for i in bad[0])
                return "a%d affine=%s alpha=%g reverse=%d: (image %d, row %d, column %d, channel %d) got %r, float64 %r; %d elements outside" % (
                    act, affine, alpha, reverse, b, y, xx, c, float(got[b, y, xx, c]), float(v[b, y, xx, c]), len(bad))
    return None


def _locate(cid, runner):
    """What the float64 restatement says about a conv case whose digest differs."""
    fn, args = runner.func, runner.args
    if fn is D.tile_case:
        shape, dt, form = args
        return _first_bad(shape, dt, form, D.variants_of(form))
    if fn is D.rows_case:
        shape, dt, nres, out_f32 = args
        return _first_bad(shape, dt, (3, 2, 1, nres, 32, 0, None), D.VARIANTS[nres % 2::2], out_f32=out_f32)
    if fn is D.one_by_one_case:
        shape, dt = args
        return _first_bad(shape, dt, (1, 1, 3, 0, 32, 0, None), [(a, aff, 0.5) for a, aff in D.EPI_1X1])
    return "(no float64 restatement for this case: compare the launches with the tool's second output file)"


def _expected_kernel(runner):
    fn, args = runner.func, runner.args
    if fn is D.tile_case:
        shape, dt, form = args
        kh, dil, nsrc, nres, cout, in_act, pool = form
        if kh == 7:
            return shape, dt, form, False, "conv7x7_h16_dma<%d>" % D.FCODE[dt]
        return shape, dt, form, False, "conv3x3_h16_dma<%d, %d, %d, %s, %d, %d>" % (nsrc, nres, D.FCODE[dt], "true" if pool is not None else "false", dil, in_act)
    if fn is D.rows_case:
        shape, dt, nres, out_f32 = args
        return shape, dt, (3, 2, 1, nres, 32, 0, None), out_f32, "conv3x3_h16_dma_rows<%d, %d, %s>" % (D.FCODE[dt], nres, "true" if out_f32 else "false")
    if fn is D.one_by_one_case:
        shape, dt = args
        return shape, dt, (1, 1, 3, 0, 32, 0, None), False, "conv_h16_dma_1x1<%d>" % D.FCODE[dt]
    return None


def test_fixture_lists_exactly_the_cases():
    assert set(FIXTURE["cases"]) == {c[0] for c in CASES}
    assert len(FIXTURE["_commit"]) >= 7, "the fixture names the commit whose library wrote it"


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_digest_equals_the_parents(case):
    cid, runner, env = case
    exp = _expected_kernel(runner)
    if exp is not None:                                   # the case must reach the kernel it is about
        shape, dt, form, out_f32, kernel = exp
        name = D.run_case(lambda: D.kernel_name(shape, dt, form, out_f32=out_f32), env)
        assert name == kernel, (cid, name)
    launches = D.run_case(runner, env)
    assert not any(v == "guard image overwritten" for v in launches.values()), (cid, [k for k, v in launches.items() if len(v) != 64])
    got, want = D.case_digest(launches), FIXTURE["cases"][cid]
    print("DIGEST | %s | %s | %s" % (cid, got[:16], "equal" if got == want else "differs from " + want[:16]))
    if got != want:
        where = D.run_case(lambda: _locate(cid, runner), env)
        pytest.fail("%s: digest %s, the parent's %s; float64 restatement: %s" % (cid, got, want, where or "every launch within its bound"))
