"""GPU: the BFFusion baseline (paif_amd/fusion_model/bffusion.py, csrc/bffusion.hip, csrc/conv_slab.h) against the reference's own outputs
and autograd (tests/golden/gb_bffusion*.npz, generated on the CPU by tools/make_golden_bffusion.py, the reference in .eval() mode), and
inside the composite model / attack / harness flow of the searched network.

Bound of the kernel parity checks (tests/baseline_common.py: bound): with floor = max|ref32 - ref64| of the same tensor,
max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  One kernel form exists (exact fp32, the convs on v_mfma_f32_16x16x4_f32,
BatchNorm folded into the weights, the context reduction accumulated in float64); it is the default build.

In the fixtures i1 is the infrared plane and enters image_vis_y (the `_vi` modules and attn2), i2 is the visible Y plane and enters
image_ir: the order inside the composite model.

Cases: 1x16x16 is the smallest input (level 4 is 2 x 2: every reflected read and every fold lands on a border row, no fringe); 1x17x23 has
two ragged tiles each way at level 1, a pool that drops a row at level 1 and a column at levels 1-3, every upsample pads a column and the
top one a row; 1x22x16 is odd at levels 2 and 3 only; 2x16x20 has two images (per-image context matrices, batch strides); 1x40x56 and
2x35x50 have several tile rows and columns at level 1, more than one at level 2, and three chunks of the context reduction.

The reference's autograd is the yardstick of the input gradients only where no sign point (62 activation inputs, every pooling window's
gap between its two largest entries) is within fp32 reach of its switch (the gradient cases, see the tool).  At the large cases the
reverse pass is tested against a float64 restatement (tests/bffusion_eager.py) that takes every LeakyReLU / ReLU branch and every pool
choice from the tape and nothing else: softmax, LayerNorm, tanh and the gate are torch's own.  No pixel is excluded."""
import numpy as np
import pytest
import torch

from paif_amd import ops, synthetic as S
from tests import baseline_common as C
from tests.baseline_common import check, dev, exact_arithmetic, floor  # noqa: F401  (exact_arithmetic is a fixture)
from tests.bffusion_eager import eager, taped_maps
from tests.helpers import t

pytestmark = pytest.mark.gpu

GRAD_CASES = ("1x16x16", "1x17x23", "1x22x16")
TWO_IMAGES = "2x16x20"
LARGE = ("1x40x56", "2x35x50")
RESTATED = (TWO_IMAGES,) + LARGE
SMALL = ("1x16x16", "1x17x23")
HALO = 8            # full-resolution pixels the border check covers: one level-4 pixel
EPS, ALPHA = 8 / 255., 2 / 255.
_SD = {}


def _sd(golden):
    """The fixture weights, rebuilt once from the 97 scales and shifts."""
    if not _SD:
        g = golden("gb_bffusion")
        _SD.update({k: torch.from_numpy(np.asarray(v)) for k, v in S.bffusion_state_dict(g["scales"], g["shift"]).items()})
    return _SD


def _net(golden):
    from paif_amd.fusion_model.bffusion import BFFR

    net = BFFR().eval()
    net.load_state_dict(_sd(golden), strict=True)
    return net.requires_grad_(False).to(dev())


def _inputs(golden, case):
    g = golden("gb_bffusion_" + case)
    cot = g["cot"] if "cot" in g else S.make_feature(900 + len(case), g["i1"].shape)
    return t(g["i1"]).to(dev()), t(g["i2"]).to(dev()), t(cot).to(dev())


@pytest.mark.parametrize("case", GRAD_CASES + RESTATED)
def test_fused_plane_matches_the_reference(golden, case):
    g = golden("gb_bffusion_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    check("fused", case, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]), halo=HALO if case in LARGE else None)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The 98 taped maps (BFFR._map_list), each against its own floor."""
    parts = [golden("gb_bffusion_%s_maps%d" % (case, p)) for p in range(int(golden("gb_bffusion")["maps_" + case]))]
    ref = {k: v for p in parts for k, v in p.items()}
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert len(maps) == 98
    for k, m in enumerate(maps):
        check("maps", case, "map%d" % k, m, ref["map%d" % k], float(ref["map_floor"][k]))


def _gradient_parity(golden, case):
    g = golden("gb_bffusion_" + case)
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    a, b = i1.clone().requires_grad_(True), i2.clone().requires_grad_(True)
    out = net(a, b)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for name, mine in (("d_i1", a.grad), ("d_i2", b.grad)):
        assert float(np.abs(g[name + "64"]).max()) > 1e-4
        check("grad", case, name, mine, g[name + "64"], floor(g[name], g[name + "64"]))


@pytest.mark.parametrize("case", GRAD_CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    _gradient_parity(golden, case)


def test_input_gradients_of_two_images_match_float64_autograd(golden):
    """2x16x20 where the tool found a start that meets the margin condition (the fixture says which)."""
    assert bool(golden("gb_bffusion")["case_" + TWO_IMAGES][7]) == ("d_i164" in golden("gb_bffusion_" + TWO_IMAGES))
    if "d_i164" in golden("gb_bffusion_" + TWO_IMAGES):
        _gradient_parity(golden, TWO_IMAGES)


def _restated(net, taped, i1, i2, cot, dtype):
    a, b = i1.to(dtype).clone().requires_grad_(True), i2.to(dtype).clone().requires_grad_(True)
    out = eager(net, a, b, taped=taped, dtype=dtype)
    (out * cot.to(dtype)).sum().backward()
    return out.detach(), a.grad.cpu().numpy(), b.grad.cpu().numpy()


@pytest.mark.parametrize("case", RESTATED)
def test_reverse_pass_matches_its_float64_restatement_on_the_taped_branches(golden, case):
    """Sizes the margin condition cannot reach.  Only what is discontinuous is frozen from the tape; the floor is the same restatement in
    float32.  A wrong tap, slice offset, fold, pool choice, per-image index or a missing 0.5 shows at order 0.1.  The restatement runs
    through torch's own float64 ops and autograd on the device the maps are on."""
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    tape = {}
    with torch.no_grad():
        net.forward_impl(i1, i2, tape=tape)
        d1, d2 = net.backward_impl(cot, tape)
    taped = taped_maps(tape["maps"], dev())
    f64, a64, b64 = _restated(net, taped, i1, i2, cot, torch.float64)
    _, a32, b32 = _restated(net, taped, i1, i2, cot, torch.float32)
    assert float((f64 - tape["out"].double()).abs().max()) <= 1e-5      # the frozen forward is the taped one
    for name, mine, r64, r32 in (("d_i1", d1, a64, a32), ("d_i2", d2, b64, b32)):
        assert float(np.abs(r64).max()) > 1e-4
        check("taped-branch reverse", case, name, mine, r64, floor(r32, r64), halo=HALO if case in LARGE else None)


def _flat(tape):
    m = tape["maps"]
    out = [tape["out"]] + [x for s in range(2) for x in m["E"][s] + m["EN"][s]] + m["D"]
    return out + [a[k] for row in m["A"] for a in row for k in ("p1", "p2", "qkv", "ctx", "y", "z", "f1", "f2")]


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding: within 1e-4 of the largest gradient
    (tests/baseline_common.py says why)."""
    C.reverse_pass_is_linear_in_the_cotangent(_net(golden), *_inputs(golden, "1x22x16"), rtol=1e-4)


def test_two_runs_are_bit_identical(golden):
    """The whole tape and both gradients, at a size with three chunks of the context reduction."""
    run = C.two_runs_are_bit_identical(_net(golden), *_inputs(golden, "2x35x50"), taped=_flat)
    assert len(run) == 1 + (1 + 16 + 4 + 64) + 2


def test_channel_slices_are_taken_without_a_copy(golden):
    C.channel_slices_are_taken_without_a_copy(_net(golden), *_inputs(golden, TWO_IMAGES))


def test_settings_that_do_not_apply_change_nothing(golden):
    C.settings_that_do_not_apply_change_nothing(_net(golden), *_inputs(golden, "1x17x23"), fp32_maps=_flat)


def test_wrong_planes_and_modes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 16, 16, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 16, 17, device=dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(torch.zeros(1, 3, 16, 16, device=dev()), torch.zeros(1, 3, 16, 16, device=dev()))
    for shape in ((1, 1, 15, 16), (1, 1, 16, 15)):
        with pytest.raises(ValueError, match="16"):
            net(torch.zeros(shape, device=dev()), torch.zeros(shape, device=dev()))
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = z.clone().requires_grad_(True)
        out = trainable(a, z)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())
    before = {k: v.clone() for k, v in net.state_dict().items()}
    net.train()
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        with torch.no_grad():
            net(z, z)
    with pytest.raises(NotImplementedError, match="BatchNorm"):
        net.forward_impl(z, z, tape={})
    for k, v in net.state_dict().items():
        assert torch.equal(v, before[k]), k


def test_reference_initialisation_matches_torch_eager(golden):
    """A net as the constructor leaves it: torch's default conv and linear initialisation, identity BatchNorm and LayerNorm."""
    from paif_amd.fusion_model.bffusion import BFFR

    torch.manual_seed(20)
    net = BFFR().eval().requires_grad_(False).to(dev())
    i1, i2, _ = _inputs(golden, "1x17x23")
    with torch.no_grad():
        mine, ref = net(i1, i2), eager(net, i1, i2)
    err = float((mine - ref).abs().max())
    print("reference initialisation: err %.3e (fused in [%.3f, %.3f])" % (err, float(ref.min()), float(ref.max())))
    assert float(ref.max() - ref.min()) > 1e-3
    assert err <= 1e-5


def test_in_place_changes_and_eps_rebuild_the_pack(golden):
    """The pack's key holds the used BatchNorm buffers and the LayerNorm affine, and the eps floats are compared per call: a change of a
    used running_var, a LayerNorm weight, a BatchNorm eps and the LayerNorm eps each changes the output, and it is torch eager's again
    (1e-5, the bound of the test above).  A change of a ConvLayer.bn buffer -- never applied -- changes no bit."""
    net = _net(golden)
    i1, i2, _ = _inputs(golden, "1x17x23")
    at = net.fusion_block1.attn2
    steps = (("running_var", lambda: at.conv_pre[1].batch_norm.running_var[::2].mul_(4.0)),
             ("LayerNorm weight", lambda: net.fusion_block2.attn1.norm1.weight[::2].mul_(-1.5)),
             ("BatchNorm eps", lambda: setattr(net.fusion_block1.attn1.ffn[0].batch_norm, "eps", 1.0)),
             ("LayerNorm eps", lambda: setattr(net.fusion_block3.attn2.norm1, "eps", 2.0)))
    with torch.no_grad():
        last = net(i1, i2)
        assert float((last - eager(net, i1, i2)).abs().max()) <= 1e-5
        for what, change in steps:
            change()
            out = net(i1, i2)
            err, moved = float((out - eager(net, i1, i2)).abs().max()), float((out - last).abs().max())
            print("%s changed: moved %.3e, err %.3e" % (what, moved, err))
            assert moved > 1e-4 and err <= 1e-5, what
            last = out
        net.DB1_2.bn.running_var.mul_(9.0), net.conv1_ir.bn.weight.fill_(7.0), net.DB3_1.bn.running_mean.add_(1.0)
        net.DB2_2.bn.eps = 3.0
        assert torch.equal(net(i1, i2), last)


# ---- inside the composite model ------------------------------------------------------------------------------------------------
def _in_composite(golden):
    """The network with the fixture's weights as the fusion module of Network_MM_CompModel."""
    from paif_amd.fusion_model.bffusion import BFFR

    return C.composite(BFFR(), _sd(golden))


def test_composite_clean_forward(golden):
    """fused within 1e-4, logits within 2e-4 x scale, argmax agreement 99.9 %: the tolerances of
    tests/test_seg_gpu.py::test_full_model_config1_4x64x96."""
    g = golden("gb_bffusion_attack")
    C.composite_clean_forward(_in_composite(golden), g, start=int(g["start"]), fused_atol=1e-4, logits_rtol=2e-4, agreement=0.999)


def test_attack_both_pgd_through_the_baseline(golden, exact_arithmetic):
    """Limits: losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace on
    the batch the tool chose on the reference alone (tools/make_golden_didfuse.py, THE ATTACK BATCH)."""
    g = golden("gb_bffusion_attack")
    C.attack_both_pgd(_in_composite(golden), g, start=int(g["start"]), eps=EPS, alpha=ALPHA, loss_rtol=1e-4, frac=2e-3)


def _delta0(ir, vis):
    """The start perturbations of the graph test: its batch is batch 0, not the attack fixture's."""
    return [t(S.make_delta0(k, tuple(x.shape), EPS)) for k, x in enumerate((ir, vis))]


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop.  Single stream, no parallel branches; every
    weight pack is built before the capture."""
    C.pgd_iterations_replayed_from_a_graph_are_bit_identical(_in_composite(golden), start=0, delta0=_delta0, eps=EPS, alpha=ALPHA)


def test_robustness_harnesses_run_with_the_baseline(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    C.robustness_harnesses_run(_in_composite(golden), miou_atol=1e-12, attack_iters=2)
