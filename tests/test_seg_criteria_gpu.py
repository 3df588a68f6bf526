"""GPU: the segmentation criteria (paif_amd/core/loss.py: OhemCELoss, SoftmaxFocalLoss, NormalLoss on csrc/seg_criteria.hip) against the
reference's float64 results (tests/golden/gc_seg_*.npz, tools/make_golden_seg_criteria.py) and against the float64 restatement
tests/seg_criteria_eager.py where a test changes the inputs.

BOUNDS, those ops.upsample_ce is held to (tests/test_train_kernels_gpu.py, the same bilinear + softmax arithmetic in float32):
value within 1e-5 * max(1, |ref|), gradient within 2e-5 * max|ref|.  Every comparison prints its error and the ratio to its bound first;
no pixel and no element is left out.  The fixtures' margins (every valid l at least 1e-4 from T and, in mode B, l_(n_min) from
l_(n_min+1)) make the float32 selection the float64 one, so one bound serves every OHEM regime."""
import math

import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S
from paif_amd.core import loss as L
from tests import seg_criteria_eager as E
from tests.helpers import t

pytestmark = pytest.mark.gpu

TAGS = ("1x9x1x1_1x1", "1x9x3x5_12x20", "2x9x6x8_24x32", "1x19x5x7_13x29", "2x3x8x8_8x8", "1x32x4x4_16x16", "2x9x17x33_68x132",
        "2x9x6x8_24x32_ign7")
IDENTITY = "2x3x8x8_8x8"          # goes through forward(logits, labels)
VALUE_TOL, GRAD_TOL = 1e-5, 2e-5
WORST = {}                         # criterion -> worst error / bound seen in this session (printed by every check)


def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def inputs(fx):
    return torch.from_numpy(fx["seg_map"]).to(dev()), torch.from_numpy(fx["labels"]).to(dev()), int(fx["ignore_lb"])


def make(family, fx, case, ign):
    if family == "ohem":
        return L.OhemCELoss(float(fx[case + "/thresh"]), int(fx[case + "/n_min"]), ignore_lb=ign)
    if family == "focal":
        return L.SoftmaxFocalLoss(float(fx[case + "/gamma"]), ignore_lb=ign)
    return L.NormalLoss(ignore_lb=ign)


def run(crit, seg, lab, identity=False, scale=None):
    """-> (value, d value / d seg_map) through the module and its autograd node."""
    x = seg.clone().requires_grad_(True)
    v = crit(x, lab) if identity else crit.from_seg_map(x, lab)
    (v if scale is None else scale * v).backward()
    return v.detach(), x.grad


def check(what, key, value, grad, ref_v, ref_g):
    ref_v, ref_g = float(ref_v), np.asarray(ref_g, dtype=np.float64)
    ev = abs(float(value) - ref_v)
    bv = VALUE_TOL * max(1.0, abs(ref_v))
    eg = float(np.abs(grad.detach().cpu().numpy().astype(np.float64) - ref_g).max())
    bg = GRAD_TOL * float(np.abs(ref_g).max())
    ratio = max(ev / bv, eg / bg if bg > 0 else (0.0 if eg == 0 else math.inf))
    WORST[key] = max(WORST.get(key, 0.0), ratio)
    print("%-44s value %.9g  err %.2e / %.2e   grad err %.2e / %.2e   worst ratio of %s so far %.3f"
          % (what, float(value), ev, bv, eg, bg, key, WORST[key]))
    assert ev <= bv, (what, ev, bv)
    assert eg <= bg, (what, eg, bg)


@pytest.mark.parametrize("tag", TAGS)
def test_ohem_against_float64(golden, tag):
    fx = golden("gc_seg_ohem_" + tag)
    seg, lab, ign = inputs(fx)
    nv = int((fx["labels"] != ign).sum())
    for case in fx["cases"]:
        crit = make("ohem", fx, case, ign)
        v, g = run(crit, seg, lab, tag == IDENTITY)
        check("ohem %s %s" % (tag, case), "ohem", v, g, fx[case + "/value64"], fx[case + "/dseg64"])
        # the device's decisions: the mode, and in mode B exactly the n_min-th largest of the device's own l plane
        coef, lplane, _ = ops.seg_criterion_fwd(ops.to_nhwc(seg), lab, "ohem", T=crit.thresh, n_min=crit.n_min, ignore_index=ign)
        c = coef.cpu().tolist()
        assert c[0] == float(v) and int(c[1]) == int(fx[case + "/mode"]) and int(c[5]) == nv and c[6] == 0.0, (case, c)
        flat = lplane.flatten()
        if int(c[1]) == 2:
            kth = torch.sort(flat, descending=True).values[crit.n_min - 1]
            assert c[2] == float(kth) and int(c[7]) == int((flat > kth).sum()), (case, c, float(kth))
        else:
            assert np.float32(c[2]) == fx[case + "/T"] and int(c[7]) == int((flat > c[2]).sum()) >= crit.n_min, (case, c)


@pytest.mark.parametrize("tag", TAGS)
def test_focal_against_float64(golden, tag):
    fx = golden("gc_seg_focal_" + tag)
    seg, lab, ign = inputs(fx)
    for case in fx["cases"]:
        crit = make("focal", fx, case, ign)
        v, g = run(crit, seg, lab, tag == IDENTITY)
        check("focal %s %s" % (tag, case), "focal", v, g, fx[case + "/value64"], fx[case + "/dseg64"])
    # gamma 0 is the cross entropy over the valid pixels
    v0, _ = run(make("focal", fx, "g0", ign), seg, lab, tag == IDENTITY)
    ce = float(ops.upsample_ce(seg, lab, ignore_index=ign))
    print("focal gamma 0 %.9g   upsample_ce %.9g" % (float(v0), ce))
    assert abs(float(v0) - ce) <= VALUE_TOL * max(1.0, abs(ce))


@pytest.mark.parametrize("tag", TAGS)
def test_normal_against_float64(golden, tag):
    fx = golden("gc_seg_normal_" + tag)
    seg, lab, ign = inputs(fx)
    v, g = run(make("normal", fx, "n", ign), seg, lab, tag == IDENTITY)
    check("normal %s" % tag, "normal", v, g, fx["n/value64"], fx["n/dseg64"])
    # without an ignored label the divisor is the number of valid pixels: ops.upsample_ce
    full = torch.where(lab == ign, torch.zeros_like(lab), lab)
    a = float(L.NormalLoss(ignore_lb=ign).from_seg_map(seg, full))
    b = float(ops.upsample_ce(seg, full, ignore_index=ign))
    print("normal, no ignored label %.9g   upsample_ce %.9g" % (a, b))
    assert abs(a - b) <= VALUE_TOL * max(1.0, abs(b))


def test_no_valid_label(golden):
    fx = golden("gc_seg_ohem_1x9x3x5_12x20")
    seg, lab, ign = inputs(fx)
    none = torch.full_like(lab, ign)
    for crit in (L.NormalLoss(), L.OhemCELoss(0.7, 17), L.OhemCELoss(0.7, lab.numel())):
        v, g = run(crit, seg, none)
        print(type(crit).__name__, float(v), float(g.abs().max()))
        assert float(v) == 0.0 and float(g.abs().max()) == 0.0
    v, g = run(L.SoftmaxFocalLoss(2.0), seg, none)
    print("focal", float(v), float(g.abs().max()))
    assert math.isnan(float(v)) and float(g.abs().max()) == 0.0       # 0 / 0 as in torch; no valid pixel, so no gradient anywhere


def test_out_of_range_labels_are_counted_not_indexed(golden):
    fx = golden("gc_seg_ohem_1x9x3x5_12x20")
    seg, lab, ign = inputs(fx)
    C = seg.shape[1]
    spots = (lab == ign).flatten().nonzero().flatten()[:2]
    odd = lab.clone()
    odd.view(-1)[spots[0]] = C
    odd.view(-1)[spots[1]] = -1
    logits = ops.to_nhwc(seg)
    for kind, kw in (("normal", {}), ("focal", dict(gamma=2.0)), ("ohem", dict(T=E.ohem_T(0.7), n_min=int(fx["A/n_min"]))),
                     ("ohem", dict(T=E.ohem_T(0.02), n_min=int(fx["Bzero/n_min"])))):
        c0, l0, s0 = ops.seg_criterion_fwd(logits, lab, kind, ignore_index=ign, **kw)
        c1, l1, s1 = ops.seg_criterion_fwd(logits, odd, kind, ignore_index=ign, **kw)
        print(kind, kw, c0.tolist(), c1.tolist())
        assert float(c0[6]) == 0.0 and float(c1[6]) == 2.0
        assert torch.equal(c0[:6], c1[:6]) and torch.equal(l0, l1) and torch.equal(s0, s1)
        up = torch.ones(1, device=dev())
        d0, _ = ops.seg_criterion_bwd(logits, lab, l0, s0, c0, up, kind, kw.get("gamma", 0.0), ign)
        d1, _ = ops.seg_criterion_bwd(logits, odd, l1, s1, c1, up, kind, kw.get("gamma", 0.0), ign)
        assert torch.equal(d0, d1)


def test_ties_share_the_remaining_weight(golden):
    """seg_map = 0: every valid l is log C in any arithmetic.  Mode B with n_min below #valid: all valid pixels tie at v."""
    fx = golden("gc_seg_ohem_2x9x6x8_24x32")
    seg, lab, ign = inputs(fx)
    seg = torch.zeros_like(seg)
    C, nv = seg.shape[1], int((lab != ign).sum())
    n_min, T = nv // 3, E.ohem_T(0.02)                       # T = 3.9 > log 9: cnt = 0
    crit = L.OhemCELoss(0.02, n_min)
    v, g = run(crit, seg, lab)
    ulp = float(np.spacing(np.float32(math.log(C))))
    print("ties: value %.9g  log C %.9g  err %.2e (ulp %.2e)" % (float(v), math.log(C), abs(float(v) - math.log(C)), ulp))
    # log(9.0f) rounded by logf (1 ulp) and nothing else: exp(0) = 1, the sum 9 and (n_min * v) / n_min are exact
    assert abs(float(v) - math.log(C)) <= ulp
    logits = ops.to_nhwc(seg)
    coef, lplane, lse = ops.seg_criterion_fwd(logits, lab, "ohem", T=T, n_min=n_min)
    c = coef.cpu().tolist()
    assert int(c[1]) == 2 and c[2] == float(v) and c[7] == 0.0 and c[3] == np.float32(1.0 / n_min), c
    _, dfull = ops.seg_criterion_bwd(logits, lab, lplane, lse, coef, torch.ones(1, device=dev()), "ohem")
    valid = (lab != ign)
    rows = dfull[valid]                                      # [#valid, cp]
    onehot = torch.nn.functional.one_hot(lab[valid], dfull.shape[-1]).bool()
    at_label, elsewhere = rows[onehot], rows[~onehot].view(nv, -1)[:, :C - 1]
    assert bool((at_label == at_label[0]).all()) and bool((elsewhere == elsewhere[0, 0]).all())      # every valid pixel: the same gradient
    assert float(dfull[~valid].abs().max()) == 0.0
    w = -at_label.double() / (1.0 - 1.0 / C)                 # d_label = w * (1/C - 1)
    print("ties: weight %.9g  1/#valid %.9g  sum %.9f" % (float(w[0]), 1.0 / nv, float(w.sum())))
    assert abs(float(w.sum()) - 1.0) <= 1e-5
    ref_v, ref_g = E.value_and_grad(seg.cpu(), lab.cpu(), "ohem", T=T, n_min=n_min)
    check("ohem ties", "ohem", v, g, ref_v, ref_g.numpy())


def test_upstream_gradient_scales_the_result(golden):
    for family, case in (("ohem", "A"), ("ohem", "Bpos"), ("focal", "g2"), ("normal", "n")):
        fx = golden("gc_seg_%s_1x19x5x7_13x29" % family)
        seg, lab, ign = inputs(fx)
        v, g = run(make(family, fx, case, ign), seg, lab, scale=3.0)
        check("3 * %s %s" % (family, case), family, v, g, fx[case + "/value64"], 3.0 * fx[case + "/dseg64"])


@pytest.mark.parametrize("tag", ("1x9x3x5_12x20", "2x9x17x33_68x132", IDENTITY))
def test_bit_equal_without_a_node_and_between_runs(golden, tag):
    for family in ("ohem", "focal", "normal"):
        fx = golden("gc_seg_%s_%s" % (family, tag))
        seg, lab, ign = inputs(fx)
        for case in fx["cases"]:
            crit = make(family, fx, case, ign)
            v1, g1 = run(crit, seg, lab, tag == IDENTITY)
            v2, g2 = run(crit, seg, lab, tag == IDENTITY)
            with torch.no_grad():
                v3 = crit(seg, lab) if tag == IDENTITY else crit.from_seg_map(seg, lab)
            v4 = crit.from_seg_map(seg, lab)                 # nothing requires grad: no node either
            assert v3.grad_fn is None and v4.grad_fn is None and not v4.requires_grad
            assert torch.equal(v1, v2) and torch.equal(g1, g2) and torch.equal(v1, v3) and torch.equal(v1, v4), (family, case)


@pytest.mark.parametrize("tag", ("1x9x3x5_12x20", "1x19x5x7_13x29", IDENTITY, "1x32x4x4_16x16"))
def test_pad_channels_are_zero(golden, tag):
    for family, case in (("ohem", "Bpos"), ("focal", "g0.5"), ("normal", "n")):
        fx = golden("gc_seg_%s_%s" % (family, tag))
        seg, lab, ign = inputs(fx)
        C = seg.shape[1]
        kw = dict(T=float(fx[case + "/T"]), n_min=int(fx[case + "/n_min"])) if family == "ohem" else {}
        gamma = float(fx[case + "/gamma"]) if family == "focal" else 0.0
        logits = ops.to_nhwc(seg)
        coef, lplane, lse = ops.seg_criterion_fwd(logits, lab, family, gamma=gamma, ignore_index=ign, **kw)
        d, dfull = ops.seg_criterion_bwd(logits, lab, lplane, lse, coef, torch.ones(1, device=dev()), family, gamma, ign)
        cp = (C + 3) // 4 * 4                                 # the narrowest pad the adjoint kernel takes
        assert tuple(dfull.shape) == tuple(lab.shape) + (cp,) and tuple(d.shape) == tuple(logits.shape[:3]) + (cp,)
        assert (d is dfull) == (tag == IDENTITY)
        if cp > C:
            assert float(dfull[..., C:].abs().max()) == 0.0 and float(d[..., C:].abs().max()) == 0.0
        assert float(d[..., :C].abs().max()) > 0.0
        ref = fx[case + "/dseg64"]
        got = d[..., :C].permute(0, 3, 1, 2).cpu().numpy().astype(np.float64)
        assert np.abs(got - ref).max() <= GRAD_TOL * np.abs(ref).max()


def test_inside_the_composite_model():
    from paif_amd.core.model_fusion_auto import Network_MM_Searched
    from paif_amd.genotypes import FUSION_AT

    n_min = 2 * 64 * 96 // 16
    crit = L.OhemCELoss(0.7, n_min)
    m = Network_MM_Searched(32, FUSION_AT, L.Fusionloss_grad2(), crit, "mit_b0", num_classes=9).eval()
    S.load_formula_weights(m)
    m = m.to(dev())
    ir, vis, lab = S.make_batch(2, 64, 96)
    mask = np.maximum(ir, vis[:, :1]).astype(np.float32)
    ir, vis, mask, lab = (t(a).to(dev()) for a in (ir, vis, mask, lab))
    with torch.no_grad():
        loss = m._loss(ir, vis, mask, lab)
        fused, seg = m(ir, vis)
        ref = m._criterion(ir, ops.rgb2ycrcb(vis), fused, mask) * 0.1 + crit.from_seg_map(seg, lab.long()) * 4
        assert tuple(seg.shape) == (2, 9, 16, 24)
        seg_term = float(crit.from_seg_map(seg, lab.long()))
    print("_loss %.7f   0.1 criterion + 4 seg term %.7f   seg term %.7f" % (float(loss), float(ref), seg_term))
    assert torch.equal(loss, ref) and seg_term > 0.0
    irg = ir.clone().requires_grad_(True)
    m._loss(irg, vis, mask, lab).backward()
    assert irg.grad is not None and float(irg.grad.abs().max()) > 0.0 and bool(torch.isfinite(irg.grad).all())
    print("d loss / d ir: max %.3e" % float(irg.grad.abs().max()))


def test_linear_graph_capture_replays_on_new_inputs(golden):
    """Value and gradient in one captured graph on a single stream; the replay runs on other logits AND other labels, which moves OHEM from
    mode A to mode B: the decision is the device's."""
    tag = "2x9x6x8_24x32"
    fo = golden("gc_seg_ohem_" + tag)
    seg0, lab0, ign = inputs(fo)
    seg1 = -0.5 * seg0.flip(0)
    lab1 = lab0.clone()
    lab1[0] = ign
    T, n_min = E.ohem_T(0.7), (3 * int((fo["l64"] > E.ohem_T(0.7)).sum())) // 4
    modes = [int(ops.seg_criterion_fwd(ops.to_nhwc(s), l, "ohem", T=T, n_min=n_min)[0][1]) for s, l in ((seg0, lab0), (seg1, lab1))]
    print("OHEM modes at capture and at replay:", modes)
    assert modes == [1, 2]
    for crit in (L.OhemCELoss(0.7, n_min), L.SoftmaxFocalLoss(2.0), L.NormalLoss()):
        seg = seg0.clone().requires_grad_(True)
        lab = lab0.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            torch.autograd.grad(crit.from_seg_map(seg, lab), seg)               # warm-up outside the capture
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            value = crit.from_seg_map(seg, lab)
            grad, = torch.autograd.grad(value, seg)
        with torch.no_grad():
            seg.copy_(seg1)
            lab.copy_(lab1)
        graph.replay()
        torch.cuda.synchronize()
        v_e, g_e = run(crit, seg1, lab1)
        print(type(crit).__name__, "replayed %.9g eager %.9g" % (float(value.detach()), float(v_e)))
        assert torch.equal(value.detach(), v_e) and torch.equal(grad, g_e)
