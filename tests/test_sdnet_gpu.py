"""GPU: the SDNet baseline (paif_amd/fusion_model/sdnet.py, csrc/sdnet.hip) against the reference's own outputs and autograd
(tests/golden/gs_sdnet*.npz, generated on the CPU by tools/make_golden_sdnet.py), and inside the composite model / attack / harness flow
of the searched network.

Bound of the kernel parity checks (the form of tests/test_training_gpu.py's stage-gradient bound): with floor = max|ref32 - ref64| of the
same tensor, max|hip - ref64| <= 1.5 * floor + 1e-5 * max(1, max|ref64|).  The gradients reach about 8 and their floor is about 8e-6: the
scale term allows roughly 80 fp32 ulps of reordering, a wrong tap or a dropped term shows at order 0.1.  One kernel form exists (exact
fp32, the dense convs on v_mfma_f32_16x16x4_f32); it is the default build."""
import numpy as np
import pytest
import torch

from paif_amd import ops
from tests import baseline_common as C
from tests.baseline_common import check, dev, exact_arithmetic, floor  # noqa: F401  (exact_arithmetic is a fixture)
from tests.helpers import t

pytestmark = pytest.mark.gpu

CASES = ("2x24x32", "1x37x53", "1x13x17", "1x4x5")
LARGE = ("2x24x32", "1x37x53")
SMALL = ("1x13x17", "1x4x5")
HALO = 5            # 2 + 1 + 1 + 1: the 5 x 5 conv and three 3 x 3
EPS, ALPHA = 8 / 255., 2 / 255.


def _net(golden):
    from paif_amd.fusion_model.sdnet import SDNet

    net = SDNet().eval()
    net.load_state_dict(_sd(golden), strict=True)
    return net.requires_grad_(False).to(dev())


def _sd(golden):
    return {k[3:]: torch.from_numpy(np.asarray(v)) for k, v in golden("gs_sdnet").items() if k.startswith("sd/")}


def _inputs(golden, case):
    g = golden("gs_sdnet_" + case)
    return t(g["i1"]).to(dev()), t(g["i2"]).to(dev()), t(g["cot"]).to(dev())


@pytest.mark.parametrize("case", CASES)
def test_fused_plane_matches_the_reference(golden, case):
    """1x4x5 is smaller than the 5x5 kernel and than the halo, 1x13x17 and 1x37x53 are ragged (no multiple of the 16 x 16 and 32 x 8
    tiles, more than one workgroup), 2x24x32 has two images."""
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    with torch.no_grad():
        out = net(i1, i2)
    assert out.grad_fn is None and out.shape == i1.shape
    g = golden("gs_sdnet_" + case)
    check("fused", case, "fused", out, g["fused64"], floor(g["fused"], g["fused64"]), halo=HALO if case in LARGE else None)


@pytest.mark.parametrize("case", SMALL)
def test_feature_maps_match_the_reference(golden, case):
    """The eight LeakyReLU maps x11 .. x14, x21 .. x24, each against its own floor."""
    g = golden("gs_sdnet_" + case)
    net = _net(golden)
    i1, i2, _ = _inputs(golden, case)
    maps = net._features(i1, i2)
    assert len(maps) == 8
    for k, m in enumerate(maps):
        got = m.cpu().numpy().astype(np.float64)
        ref32, ref64 = g["maps"][k], g["maps64"][k]
        assert got.shape == ref64.shape
        bound = C.bound(floor(ref32, ref64), ref64)
        err = float(np.abs(got - ref64).max())
        print("maps %s x%d%d: err %.3e bound %.3e ratio %.3f" % (case, k // 4 + 1, k % 4 + 1, err, bound, err / bound))
        assert err <= bound, (k, err, bound)


@pytest.mark.parametrize("case", CASES)
def test_input_gradients_match_float64_autograd(golden, case):
    """d_i1, d_i2 for the fixture's cotangent on the fused plane, through forward + .backward()."""
    g = golden("gs_sdnet_" + case)
    net = _net(golden)
    i1, i2, cot = _inputs(golden, case)
    a, b = i1.clone().requires_grad_(True), i2.clone().requires_grad_(True)
    out = net(a, b)
    assert out.grad_fn is not None
    (out * cot).sum().backward()
    for name, mine in (("d_i1", a.grad), ("d_i2", b.grad)):    # on the large cases the outermost 5 rows / columns taken alone as well
        check("grad", case, name, mine, g[name + "64"], floor(g[name], g[name + "64"]), halo=HALO if case in LARGE else None)


def test_reverse_pass_is_linear_in_the_cotangent(golden):
    """backward_impl(g1) + backward_impl(g2) = backward_impl(g1 + g2) to fp32 rounding: within 1e-4 of the largest gradient
    (tests/baseline_common.py says why)."""
    C.reverse_pass_is_linear_in_the_cotangent(_net(golden), *_inputs(golden, "1x37x53"), rtol=1e-4)


def test_two_runs_are_bit_identical(golden):
    C.two_runs_are_bit_identical(_net(golden), *_inputs(golden, "2x24x32"), taped=lambda tape: [tape["feat"]])


def test_channel_slices_are_taken_without_a_copy(golden):
    """The composite hands over ir[:, 0:1] and ycc of multi-channel tensors: planes addressed through their batch stride."""
    C.channel_slices_are_taken_without_a_copy(_net(golden), *_inputs(golden, "2x24x32"))


def test_settings_that_do_not_apply_change_nothing(golden):
    """One arithmetic: the storage mode, the conv / GEMM precision and two_stream leave every bit where it is."""
    C.settings_that_do_not_apply_change_nothing(_net(golden), *_inputs(golden, "1x13x17"), fp32_maps=lambda tape: [tape["feat"]])


def test_wrong_planes_are_refused_on_the_device(golden):
    net = _net(golden)
    z = torch.zeros(1, 1, 8, 8, device=dev())
    with pytest.raises(TypeError, match="fp32"):
        net(z.half(), z.half())
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(z, torch.zeros(1, 1, 8, 9, device=dev()))
    with pytest.raises(ValueError, match=r"\[B,1,H,W\]"):
        net(torch.zeros(1, 3, 8, 8, device=dev()), torch.zeros(1, 3, 8, 8, device=dev()))
    trainable = _net(golden).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="[Pp]arameter gradients"):
        trainable(z, z)
    with ops.no_param_grads():                                  # an attack's forward: input gradients only
        a = z.clone().requires_grad_(True)
        out = trainable(a, z)
        out.sum().backward()
    assert a.grad is not None and all(p.grad is None for p in trainable.parameters())


# ---- inside the composite model ------------------------------------------------------------------------------------------------
def _in_composite(golden):
    """The network with the fixture's weights as the fusion module of Network_MM_CompModel."""
    from paif_amd.fusion_model.sdnet import SDNet

    return C.composite(SDNet(), _sd(golden))


def test_composite_clean_forward(golden):
    """fused within 1e-4, logits within 2e-4 x scale, argmax agreement 99.9 %: the tolerances of
    tests/test_seg_gpu.py::test_full_model_config1_4x64x96."""
    g = golden("gs_sdnet_attack")
    C.composite_clean_forward(_in_composite(golden), g, start=0, fused_atol=1e-4, logits_rtol=2e-4, agreement=0.999)


def test_attack_both_pgd_through_the_baseline(golden, exact_arithmetic):
    """Losses rtol 1e-4, sign and delta mismatch <= 2e-3, against the reference's float32 trace."""
    g = golden("gs_sdnet_attack")
    C.attack_both_pgd(_in_composite(golden), g, start=0, eps=EPS, alpha=ALPHA, loss_rtol=1e-4, frac=2e-3)


def test_pgd_iterations_replayed_from_a_graph_are_bit_identical(golden):
    """Three PGD iterations captured once with torch.cuda.graph and replayed = the eager loop (tests/baseline_common.py: one
    eager pass first, one side stream, no parallel branches)."""
    g = golden("gs_sdnet_attack")
    C.pgd_iterations_replayed_from_a_graph_are_bit_identical(_in_composite(golden), start=0,
                                                             delta0=lambda ir, vis: (t(g["d0_ir"]), t(g["d0_vis"])), eps=EPS, alpha=ALPHA)


def test_robustness_harnesses_run_with_the_baseline(golden):
    """val_segformer_robust2 (clean) and val_segformer_robust (PGD, 2 iterations) on two 2x64x96 batches: finite mIoU, and the clean one is
    what the confusion matrix of the model's own seg_map argmax gives."""
    C.robustness_harnesses_run(_in_composite(golden), miou_atol=1e-12, attack_iters=2)
